"""The cases of the sample-generation tests (tests/test_generate_cpu.py, tests/test_generate_gpu.py): contexts, image sizes, sample ranges, seeds and
tile layouts for ssx_debug_generate, and per case the records ssx_generate_kernel has to write, word for word, built from the oracle:
orc_seed_sample(seed, j * W + i, k), orc_camera_sample, orc_debug_camera_hit.  TEST INFRASTRUCTURE; everything here is computed on the CPU, once per
process.

The record order is the kernel's: [tile slot][k - k0][lane], lane = 8 * row + column of the 8 x 8 tile.  The map from a slot to its tile is restated here
from the documented rule (csrc/ssx_kernels.hip tile_of_slot): slot s is place t = tile_first + s * tile_stride of the row-major tile list, whose row
ty = t // tiles_x is rotated by (ty * tile_skew) % tiles_x columns: tx = (t % tiles_x - rot) mod tiles_x.  tests/tile_mask_ref.slot_tiles builds the same list
from dist.tile_owner_mask; the CPU test holds the two together on every case small enough for whole-image masks."""
import collections
import ctypes as C
import functools

import numpy as np

import custom_scene as cs
import oracle_lib as ol
import pretrace_cases as pc
import tile_mask_ref as tm
from simple_spectral_amd import _capi

FILL = np.uint32(_capi.SSX_GENERATE_FILL_BYTE * 0x01010101)   # a word no lane wrote (include/ssx.h SSX_GENERATE_FILL_BYTE)
NO_SLOT = 0x1FFF                                              # csrc/ssx_blob.h SSX_NO_SLOT
# the tail word of a path that ends at level 0 without a hit (csrc/ssx_blob.h: hit_anything | emission << 1 | D << 2 | slot of level D-1's entry << 6 |
# slot of level D's next-event term << 19): no hit, no emission, D = 0, neither slot
MISS_TAIL = np.uint32((NO_SLOT << 6) | (NO_SLOT << 19))
MISS_HIT = (np.float32(np.inf).view(np.uint32), np.uint32(0), np.uint32(0), np.uint32(0xFFFFFFFF))   # SSX_DBG_TRACE's miss: dist +inf, st 0, no primitive
K_TOP = (1 << 32) - 4
SEED_TOP = (1 << 64) - 1


# ---- contexts -------------------------------------------------------------------------------------------------------------------------------
class Context:
    """One scene and camera on both sides: `oracle`, `renderer()` (a fresh context of the device library), and what the reference needs beside them:
    pv_inv / cam_pos as both sides received them, albedo_mode per primitive, rgb."""

    def __init__(self, name, custom=None, builtin=None, observer=1931, rgb=False):
        self.name, self.rgb, self.observer = name, rgb, observer
        self._custom, self._builtin = custom, builtin
        if custom is not None:
            self.oracle = custom.oracle()
        else:
            self.oracle = ol.Oracle(builtin, observer=observer, texture="test-img.png", rgb=rgb)
        lib, sc = self.oracle.lib, self.oracle.scene
        n = C.c_int()
        lib.orc_scene_counts(sc, C.byref(n), None, None)
        self.n_prims = n.value
        self.pv_inv = np.array(lib.orc_scene_pv_inv(sc)[:16], dtype=np.float64)
        self.cam_pos = np.array(lib.orc_scene_cam_pos(sc)[:3], dtype=np.float32)
        six = (C.c_float * 6)()
        self.albedo_mode = np.array([lib.orc_scene_material_rgb(sc, lib.orc_scene_quad_material(sc, q), six) for q in range(self.n_prims)], dtype=np.int64)
        assert (self.albedo_mode >= 0).all()

    def renderer(self):
        from simple_spectral_amd import Options, Renderer
        if self._custom is None:
            return Renderer(Options(scene_name=self._builtin, res=(8, 8), spp=1, observer=self.observer, texture="test-img.png",
                                    render_mode="rgb" if self.rgb else "spectral"))
        r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, observer=self.observer))
        r.upload_scene_desc(self._custom.desc(self.oracle))
        return r


_CONTEXTS = {
    # the two built-in topologies, as scene descriptions (the corner pattern decides the topology, not the name), under both observers
    "cornell-srgb": lambda n: Context(n, custom=cs.CustomScene("cornell-srgb")),
    "cornell-srgb-2006": lambda n: Context(n, custom=cs.CustomScene("cornell-srgb", observer=2006), observer=2006),
    "plane-srgb": lambda n: Context(n, custom=cs.CustomScene("plane-srgb")),
    # the crafted contexts of the pre-trace tests: 33, 70 and 128 primitives, triangle primitives, primitives behind the camera
    "prims33": lambda n: Context(n, custom=pc.MASK_CASES["prims33"][0]()),
    "prims70": lambda n: Context(n, custom=pc.MASK_CASES["prims70"][0]()),
    "prims128-2006": lambda n: Context(n, custom=pc.MASK_CASES["prims128-2006"][0](), observer=2006),
    "triangles": lambda n: Context(n, custom=pc.MASK_CASES["triangles"][0]()),
    "prims70-inside": lambda n: Context(n, custom=pc.MASK_CASES["prims70-inside"][0]()),
    # RENDER_MODE_RGB: no wavelength draw
    "cornell-srgb-rgb": lambda n: Context(n, builtin="cornell-srgb", rgb=True),
}
CONTEXTS = tuple(_CONTEXTS)
OPEN_SCENES = ("cornell-srgb", "cornell-srgb-2006", "cornell-srgb-rgb")   # the box's open front: camera rays leave the scene


@functools.lru_cache(maxsize=None)
def context(name):
    return _CONTEXTS[name](name)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name W H k0 n_k seed first stride skew")

# The largest image check_params admits has 2^28 pixels, so no pixel index reaches 2^32 (profiles/r30/NOTES.md); this one has 268 434 675 (one more
# tile column would pass 2^28), is ragged on both sides and more than 65 535 tiles wide; the 14 places its layout owns end in the last tile of the last row.
LARGE = (600525, 447)
LARGE_LAYOUT = (300263, 300264, 0)

SIZE_CASES = (
    Case("8x8", 8, 8, 0, 1, 0, 0, 1, 0),                           # one full tile; both sides a power of two
    Case("16x8", 16, 8, 5, 3, 3, 0, 1, 0),                         # power of two, two tiles
    Case("64x32", 64, 32, 0, 1, SEED_TOP, 0, 1, 0),                # power of two, 8 x 4 tiles
    Case("24x16", 24, 16, K_TOP, 3, SEED_TOP, 0, 1, 0),            # only the height a power of two: division; k + 1 up to 2^32 - 1 with a seed of 2^64 - 1
    Case("13x11", 13, 11, 5, 1, 3, 0, 1, 0),                       # ragged on both sides
    Case("1x1", 1, 1, K_TOP, 1, 0, 0, 1, 0),
    Case("1x37", 1, 37, 0, 3, 3, 0, 1, 0),
    Case("37x1", 37, 1, 5, 3, SEED_TOP, 0, 1, 0),
    Case("large", LARGE[0], LARGE[1], 5, 1, SEED_TOP, *LARGE_LAYOUT),
)
# 29 x 23: 4 x 3 tiles, ragged on both sides
LAYOUTS = ((0, 1, 0), (1, 3, 0), (0, 2, 1), (2, 3, 5), (0, 1, 7), (1, 2, 9))   # (tile_first, tile_stride, tile_skew); 5, 7 and 9 exceed tiles_x = 4
LAYOUT_CASES = tuple(Case("29x23/%d,%d,%d" % lay, 29, 23, 0, 1, 3, *lay) for lay in LAYOUTS)
# a launch that starts at k0 = 5 against sample 5 of a launch that starts at 0
K_CASES = (Case("16x8/k5", 16, 8, 5, 1, 3, 0, 1, 0), Case("16x8/k0-7", 16, 8, 0, 8, 3, 0, 1, 0))
# Where the division path shows in a record.  x / W and x * (1 / W) differ by at most one unit in the last place of a binary64; behind the projection, the
# normalisation and the rounding to float that changes a word of about one record in 10^8 (numpy, 2 x 10^7 random image points per size: none at 24 x 16,
# 13 x 11, 37 x 1, 600 x 400, one at 3 x 3) -- no image of a few thousand records does it at the k0 above.  These two do, under the Cornell box's camera: found
# by walking k upwards from 0 at seed 3 with the stream restated in numpy, each the first k of its size at which a record differs (pixel (12, 8) resp.
# (9, 12): a direction component near zero, where a float's unit in the last place is as small as the binary64 difference).  16 x 24 is the size a test
# of the width alone gets wrong, 24 x 16 the size a test of the height alone gets wrong; tests/test_generate_cpu.py confirms both against the oracle.
RECIPROCAL_CASES = (Case("24x16/k708528", 24, 16, 708528, 1, 3, 0, 1, 0), Case("16x24/k124628", 16, 24, 124628, 1, 3, 0, 1, 0))
CASES = SIZE_CASES + LAYOUT_CASES + K_CASES + RECIPROCAL_CASES


def tiles_of(W, H):
    return (W + 7) // 8, (H + 7) // 8


def slot_tiles(case):
    """[(tx, ty)] per tile slot, by the documented rule (module docstring)"""
    tiles_x, tiles_y = tiles_of(case.W, case.H)
    out = []
    for t in range(case.first, tiles_x * tiles_y, case.stride):
        ty, txr = divmod(t, tiles_x)
        rot = (ty * case.skew) % tiles_x
        out.append(((txr - rot) % tiles_x, ty))
    return out


def record_pixels(case):
    """(i, j, k, inside) of every record in device order, int64 / bool [slots, n_k, 64]"""
    tiles = np.array(slot_tiles(case), dtype=np.int64).reshape(-1, 2)
    lane = np.arange(64)
    i = tiles[:, 0, None, None] * 8 + (lane & 7)[None, None, :] + np.zeros((1, case.n_k, 1), dtype=np.int64)
    j = tiles[:, 1, None, None] * 8 + (lane >> 3)[None, None, :] + np.zeros((1, case.n_k, 1), dtype=np.int64)
    k = case.k0 + np.arange(case.n_k, dtype=np.int64)[None, :, None] + np.zeros_like(i)
    return i, j, k, (i < case.W) & (j < case.H)


@functools.lru_cache(maxsize=None)
def _samples(ctx_name, W, H, seed, pix_key):
    """the oracle's camera samples for the records `pix_key` = bytes of an int64 [n, 3] array of (i, j, k): shared by the cases that cover the same
    pixels and samples in another order (layouts)"""
    ijk = np.frombuffer(pix_key, dtype=np.int64).reshape(-1, 3)
    ref = context(ctx_name).oracle.camera_samples(ijk[:, :2], ijk[:, 2], W, H, seed=seed)
    for a in ref.values():
        a.setflags(write=False)
    return ref


class Reference:
    """What the oracle says about a case's records, in device order: `inside` bool [slots, n_k, 64]; for the inside records (flattened in that order)
    `ijk` int64 [n, 3] and the arrays of Oracle.camera_samples; `words(pre_hits)` = the three arrays ssx_debug_generate has to return."""

    def __init__(self, ctx_name, case):
        self.ctx, self.case = context(ctx_name), case
        i, j, k, self.inside = record_pixels(case)
        self.ijk = np.ascontiguousarray(np.stack([i[self.inside], j[self.inside], k[self.inside]], axis=1))
        # (sorted, so that two layouts of one image share the oracle's work)
        order = np.lexsort((self.ijk[:, 2], self.ijk[:, 0], self.ijk[:, 1]))
        ref = _samples(ctx_name, case.W, case.H, case.seed, np.ascontiguousarray(self.ijk[order]).tobytes())
        back = np.empty_like(order); back[order] = np.arange(len(order))
        self.s = {name: a[back] for name, a in ref.items()}
        self.hit = self.s["prim"] >= 0

    def words(self, pre_hits):
        """(ray, st, hit) uint32 [slots, n_k, 64, 4]"""
        s, n = self.s, len(self.ijk)
        shape = self.inside.shape + (4,)
        ray, st, hit = (np.full(shape, FILL, dtype=np.uint32) for _ in range(3))
        r = np.zeros((n, 4), dtype=np.uint32)
        r[:, :3] = s["dir"].view(np.uint32); r[:, 3] = s["lambda_0"].view(np.uint32)
        ray[self.inside] = r
        live = np.stack([s["state"] & 0xFFFFFFFF, s["state"] >> 32, s["inc"] & 0xFFFFFFFF, s["inc"] >> 32], axis=1).astype(np.uint32)
        if not pre_hits:
            st[self.inside] = live
            return ray, st, hit
        ended = np.stack([r[:, 3], np.full(n, MISS_TAIL), live[:, 0], live[:, 1]], axis=1).astype(np.uint32)
        st[self.inside] = np.where(self.hit[:, None], live, ended)
        h = np.tile(np.array(MISS_HIT, dtype=np.uint32), (n, 1))
        textured = self.hit & (self.ctx.albedo_mode[np.maximum(s["prim"], 0)] != 0)
        h[self.hit, 0] = s["dist"][self.hit].view(np.uint32)
        h[textured, 1:3] = s["st"][textured].view(np.uint32)          # (+0 where the quad's albedo is no texture: hit_st is not computed there)
        h[self.hit, 3] = (2 * s["prim"][self.hit].astype(np.int64) + s["which"][self.hit]).astype(np.uint32)
        hit[self.inside] = h
        return ray, st, hit


@functools.lru_cache(maxsize=None)
def reference(ctx_name, case):
    return Reference(ctx_name, case)


def cases_of(ctx_name):
    """Every context runs every case.  (The large image costs 14 tiles.)"""
    return CASES


# ---- the second opinion on the arithmetic ----------------------------------------------------------------------------------------------------
def subpixels(case, ijk):
    """(sub_x, sub_y) binary64 [n] of the records: the stream's first two draws, y first (orc_seed_sample, orc_rand_1d)"""
    lib, rng = ol.load(), ol.Rng()
    sx, sy = np.zeros(len(ijk)), np.zeros(len(ijk))
    for r, (i, j, k) in enumerate(ijk.tolist()):
        lib.orc_seed_sample(case.seed, j * case.W + i, k, C.byref(rng))
        sy[r] = lib.orc_rand_1d(C.byref(rng)); sx[r] = lib.orc_rand_1d(C.byref(rng))
    return sx, sy


def numpy_dirs(ctx, case, ijk, sx, sy, reciprocal=False):
    """float32 [n, 3]: tile_mask_ref.camera_dir (numpy binary64, division by the image size) normalised as generate_sample normalises, rounded once.
    reciprocal=True: (i + sub) * (1 / W) in place of the division -- the power-of-two shortcut applied where it is not exact."""
    x, y = ijk[:, 0].astype(np.float64) + sx, ijk[:, 1].astype(np.float64) + sy
    if reciprocal:
        # camera_dir divides by the size it is given: hand it x * (1 / W) with a size of 1
        d = tm.camera_dir(ctx.pv_inv, ctx.cam_pos, 1, 1, x * (1.0 / np.float64(case.W)), y * (1.0 / np.float64(case.H)))
    else:
        d = tm.camera_dir(ctx.pv_inv, ctx.cam_pos, case.W, case.H, x, y)
    inv = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return (d * inv[:, None]).astype(np.float32)


# ---- fused generation ------------------------------------------------------------------------------------------------------------------------
FUSED_RES, FUSED_SPP, FUSED_SEED = (21, 13), 3, 3
FUSED_LAYOUT = dict(tile_first=1, tile_stride=2, tile_skew=1)      # 3 x 2 tiles, three of them owned: an uneven share
FUSED_MODES = {"default": "fused", "0": "generate kernel"}         # SSX_FUSE_GEN -> what the launches have to report
