"""The per-tile primitive mask of the camera-ray pre-trace (csrc/ssx_kernels.hip ssx_tile_mask_kernel), restated in plain numpy
binary64 from its documented rule, and the ground truth it has to respect.  TEST INFRASTRUCTURE.

The rule.  A tile is an 8 x 8 pixel rectangle [x0, x0 + 8] x [y0, y0 + 8].  Its frustum is bounded by four planes through the camera
position, each spanned by two neighbouring corner rays of the rectangle (the unnormalised binary64 directions of camera_dir:
renderer.cpp:114-131), with the unit normal turned so that the ray through the rectangle's centre lies on its positive side.  With
v = a stored vertex minus the camera position, dist = |v| and sd = n . v, a primitive is DROPPED if and only if, for one of the four
planes, all four stored vertices have sd < -1e-4 * dist (a PrimTri stores its first vertex again as the fourth).  Everything else,
a comparison with a NaN included, keeps the primitive.

Two things are computed here: the mask by that rule (`reference_mask`, with every sd and dist, so that a test can name the entries
within rounding of the threshold), and what no rule may contradict -- the primitives that rays through the tile really hit
(`tile_rays`, `hit_prims`: the oracle's intersection on float rays built the way generate_sample builds them)."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from simple_spectral_amd import dist as sdist

TILE = sdist.TILE
THRESHOLD = 1.0e-4      # of the vertex's distance from the camera
BAND = 1.0e-12          # |sd + THRESHOLD * dist| <= BAND * dist: binary64 rounding over the ~50 operations is ~1e-14 relative; 100 times that


def scene_arrays(desc):
    """(pv_inv float64[16] column-major, cam_pos float32[3], vertices float32[n, 4, 3]) of an ssx_scene_desc (or a pointer to one)."""
    d = desc.contents if hasattr(desc, "contents") else desc
    pv_inv = np.array(d.pv_inv[:], dtype=np.float64)
    cam_pos = np.array(d.cam_pos[:], dtype=np.float32)
    verts = np.array([[getattr(d.quads[q], name).pos[:] for name in ("v00", "v10", "v11", "v01")] for q in range(d.n_quads)], dtype=np.float32)
    return pv_inv, cam_pos, verts


def slot_tiles(width, height, tile_first=0, tile_stride=1, tile_skew=0):
    """[(tx, ty)] per tile slot of a device: slot s is place tile_first + s * tile_stride of the shared-out tile list.  Which tile sits at
    which place is dist.tile_owner_mask's business (a world of one tile per rank: rank = the place), the skew included."""
    tiles_x, tiles_y = sdist.tile_grid(width, height)
    n = tiles_x * tiles_y
    out = []
    for place in range(tile_first, n, tile_stride):
        jj, ii = np.nonzero(sdist.tile_owner_mask(width, height, place, n, tile_skew % tiles_x))
        assert len(ii) and len({(i // TILE, j // TILE) for i, j in zip(ii.tolist(), jj.tolist())}) == 1
        out.append((int(ii.min()) // TILE, int(jj.min()) // TILE))
    return out


def camera_dir(pv_inv, cam_pos, width, height, x, y):
    """renderer.cpp:114-131 up to the normalisation, binary64: the direction from the camera through the image point (x, y), in pixel
    units; x and y may be arrays.  Returns [..., 3]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    ndc_x = x / np.float64(width) * 2.0 - 1.0
    ndc_y = y / np.float64(height) * 2.0 - 1.0
    m = np.asarray(pv_inv, dtype=np.float64).reshape(4, 4)   # m[c][r]
    q = [(m[0][r] * ndc_x + m[1][r] * ndc_y) + (m[2][r] * 0.0 + m[3][r] * 1.0) for r in range(4)]
    cam = np.asarray(cam_pos, dtype=np.float32).astype(np.float64)
    return np.stack([q[0] / q[3] - cam[0], q[1] / q[3] - cam[1], q[2] / q[3] - cam[2]], axis=-1)


def tile_planes(pv_inv, cam_pos, width, height, tx, ty):
    """unit normals [4, 3] of the tile's frustum planes, turned towards the centre ray"""
    x0, y0 = float(tx * TILE), float(ty * TILE)
    corners = camera_dir(pv_inv, cam_pos, width, height, [x0, x0 + 8.0, x0 + 8.0, x0], [y0, y0, y0 + 8.0, y0 + 8.0])
    centre = camera_dir(pv_inv, cam_pos, width, height, x0 + 4.0, y0 + 4.0)
    n = np.zeros((4, 3))
    for k in range(4):
        p, q = corners[k], corners[(k + 1) & 3]
        c = np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])
        inv = 1.0 / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        n[k] = c * (-inv if (c[0] * centre[0] + c[1] * centre[1] + c[2] * centre[2]) < 0.0 else inv)
    return n


class Mask:
    """words uint32 [slots, 4]; keep bool [slots, n]; sd [slots, n, 4 planes, 4 vertices] and dist [n, 4]; banded = the entries whose comparison
    with the threshold lies within rounding (BAND)"""

    def __init__(self, words, keep, sd, dist):
        self.words, self.keep, self.sd, self.dist = words, keep, sd, dist
        with np.errstate(invalid="ignore"):
            self.banded = np.abs(sd + THRESHOLD * dist[None, :, None, :]) <= BAND * dist[None, :, None, :]

    def kept_per_tile(self):
        return self.keep.sum(axis=1)


def unpack(words, n_prims):
    """uint32 [slots, 4] -> bool [slots, n_prims]"""
    w = np.asarray(words, dtype=np.uint32)
    q = np.arange(n_prims)
    return ((w[:, q >> 5] >> (q & 31).astype(np.uint32)) & 1).astype(bool)


def pack(keep):
    keep = np.asarray(keep, dtype=bool)
    words = np.zeros((keep.shape[0], 4), dtype=np.uint32)
    for q in range(keep.shape[1]):
        words[:, q >> 5] |= keep[:, q].astype(np.uint32) << np.uint32(q & 31)
    return words


def reference_mask(pv_inv, cam_pos, verts, width, height, tile_first=0, tile_stride=1, tile_skew=0):
    verts = np.asarray(verts, dtype=np.float32)
    assert verts.ndim == 3 and verts.shape[1:] == (4, 3) and len(verts) <= 128
    v = verts.astype(np.float64) - np.asarray(cam_pos, dtype=np.float32).astype(np.float64)          # [n, 4, 3]
    dist = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])        # [n, 4]
    tiles = slot_tiles(width, height, tile_first, tile_stride, tile_skew)
    sd = np.zeros((len(tiles), len(verts), 4, 4))
    for s, (tx, ty) in enumerate(tiles):
        n = tile_planes(pv_inv, cam_pos, width, height, tx, ty)
        for k in range(4):
            sd[s, :, k, :] = n[k][0] * v[..., 0] + n[k][1] * v[..., 1] + n[k][2] * v[..., 2]
    with np.errstate(invalid="ignore"):
        out = sd < -THRESHOLD * dist[None, :, None, :]       # (NaN compares false: the primitive stays)
    keep = ~out.all(axis=3).any(axis=2)                       # dropped: all four vertices outside ONE plane
    return Mask(pack(keep), keep, sd, dist)


# ---- ground truth -------------------------------------------------------------------------------------------------------------------------
def tile_points(tx, ty):
    """The image points (x, y) [129, 2] whose rays stand for a tile's: an 11 x 11 grid over [x0, x0 + 8) x [y0, y0 + 8), the four corners at
    offsets 0 and nextafter(8, 0) -- the largest offset a sample of the tile's last pixel can have is 7 + (1 - 2^-53) -- and the
    midpoints of the four borders."""
    x0, y0 = float(tx * TILE), float(ty * TILE)
    last = float(np.nextafter(8.0, 0.0))
    g = np.arange(11) * (8.0 / 11.0)
    pts = [(x0 + a, y0 + b) for b in g for a in g]
    pts += [(x0 + a, y0 + b) for b in (0.0, last) for a in (0.0, last)]
    pts += [(x0 + 4.0, y0), (x0 + 4.0, y0 + last), (x0, y0 + 4.0), (x0 + last, y0 + 4.0)]
    return np.array(pts, dtype=np.float64)


def tile_rays(pv_inv, cam_pos, width, height, tx, ty):
    """float32 unit directions [129, 3] through tile_points, as generate_sample makes a sample's ray: binary64 direction, normalised
    in binary64 (renderer.cpp:132), rounded to float."""
    p = tile_points(tx, ty)
    d = camera_dir(pv_inv, cam_pos, width, height, p[:, 0], p[:, 1])
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (d * inv[:, None]).astype(np.float32)


def hit_prims(orc, cam_pos, dirs, depth=3):
    """The primitives the oracle's Scene::intersect (orc_scene_intersect) reports along each ray: the closest hit, then the closest hit
    with each primitive found so far ignored in its turn, `depth` rounds in all.  Returns a list of sets."""
    lib, hit = orc.lib, ol.Hit()
    o = ol.V3(*[float(x) for x in np.asarray(cam_pos, dtype=np.float32)])
    out = []
    for d in np.asarray(dirs, dtype=np.float32):
        ray = ol.Ray(o, ol.V3(float(d[0]), float(d[1]), float(d[2])))
        found, frontier = set(), [-1]
        for _ in range(depth):
            new = []
            for ign in frontier:
                if lib.orc_scene_intersect(orc.scene, C.byref(ray), C.byref(hit), int(ign), None) and hit.prim not in found:
                    found.add(int(hit.prim)); new.append(int(hit.prim))
            frontier = new
        out.append(found)
    return out


def tiles_hit(orc, pv_inv, cam_pos, width, height, tiles, depth=3):
    """bool [slots, n_prims]: primitive q is hit by one of the tile's rays (tile_rays, hit_prims)"""
    n = C.c_int()
    orc.lib.orc_scene_counts(orc.scene, C.byref(n), None, None)
    must = np.zeros((len(tiles), n.value), dtype=bool)
    for s, (tx, ty) in enumerate(tiles):
        for found in hit_prims(orc, cam_pos, tile_rays(pv_inv, cam_pos, width, height, tx, ty), depth):
            must[s, list(found)] = True
    return must
