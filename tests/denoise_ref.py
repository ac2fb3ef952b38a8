"""The denoising definitions of include/ssx.h restated on the CPU: `atrous` is the filter in numpy float32, tap by tap in the stated order; `guides_ref`
traces the pixel-centre rays with the oracle (camera_dir restated in float64).  The GPU results are compared with these bit for bit.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import oracle_lib as ol

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
H5 = (F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16))
DEFAULTS = dict(levels=5, sigma_l=1.0, sigma_a=0.1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def valid_mask(c, var):
    return np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2]) & np.isfinite(var)


def _tap(H, W, dy, dx):
    """(inside [H, W], qy, qx clipped) of the neighbour at offset (dx, dy)"""
    qy = np.arange(H)[:, None] + dy + np.zeros((1, W), dtype=np.int64)
    qx = np.arange(W)[None, :] + dx + np.zeros((H, 1), dtype=np.int64)
    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    return inside, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)


def atrous_level(c, var, prim, albedo, step, sigma_l, sigma_a):
    """One level: (c', var') from float32 c [H, W, 4], var [H, W], uint32 prim [H, W], float32 albedo [H, W, 4]."""
    H, W = var.shape
    valid = valid_mask(c, var)
    sigma_l, sigma_a = F(sigma_l), F(sigma_a)
    inv_sa2 = F(1) / (sigma_a * sigma_a)
    with np.errstate(all="ignore"):
        gs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, qy, qx = _tap(H, W, dy, dx)
                m = inside & valid[qy, qx]
                k3 = F((2 if dy == 0 else 1) * (2 if dx == 0 else 1))
                gs = np.where(m, gs + k3 * var[qy, qx], gs)
                ks = np.where(m, ks + k3, ks)
        g = gs / ks
        den = sigma_l * np.sqrt(g) + F(1e-6)
        sw, sv = np.zeros((H, W), F), np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inside, qy, qx = _tap(H, W, step * dy, step * dx)
                m = inside & valid[qy, qx] & (prim[qy, qx] == prim)
                k = H5[dy + 2] * H5[dx + 2]
                cq, vq = c[qy, qx], var[qy, qx]
                x = np.abs(cq[..., 1] - c[..., 1]) / den
                wl = F(1) / (F(1) + x * x)
                d = albedo[qy, qx] - albedo
                da2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
                wa = F(1) / (F(1) + da2 * inv_sa2)
                w = (k * wl) * wa
                sw = np.where(m, sw + w, sw)
                sc = np.where(m[..., None], sc + w[..., None] * cq[..., :3], sc)
                sv = np.where(m, sv + (w * w) * vq, sv)
        c2 = np.concatenate([sc / sw[..., None], c[..., 3:]], axis=-1)
        v2 = sv / (sw * sw)
    assert c2.dtype == F and v2.dtype == F
    return np.where(valid[..., None], c2, c), np.where(valid, v2, var)


def atrous(c, var, prim, albedo, levels=5, sigma_l=1.0, sigma_a=0.1):
    c = np.ascontiguousarray(c, dtype=F); var = np.ascontiguousarray(var, dtype=F)
    prim = np.ascontiguousarray(prim, dtype=np.uint32); albedo = np.ascontiguousarray(albedo, dtype=F)
    for l in range(levels):
        c, var = atrous_level(c, var, prim, albedo, 1 << l, sigma_l, sigma_a)
    return c, var


def variance_in_image_units(v, rgb=False):
    """var = (float)(v * (s * s)) in binary64; s = 1000, or 1 in RGB mode"""
    s = 1.0 if rgb else 1000.0
    return (np.asarray(v, dtype=np.float64) * (s * s)).astype(F)


# ---- the guide buffers from the oracle ----------------------------------------------------------------------------------------------------------------

class _OrcSpectrum(C.Structure):  # oracle/oracle.h orc_spectrum
    _fields_ = [("data", C.c_void_p), ("n", C.c_int), ("low", C.c_float), ("high", C.c_float), ("delta_lambda", C.c_float), ("delta_lambda_recip", C.c_float)]


class _OrcMaterial(C.Structure):  # orc_material
    _fields_ = [("kind", C.c_int), ("albedo_mode", C.c_int), ("emission", _OrcSpectrum), ("albedo", _OrcSpectrum), ("texture", C.c_void_p),
                ("rgb_emission", C.c_float * 3), ("rgb_albedo", C.c_float * 3)]


class _OrcCamera(C.Structure):  # orc_camera
    _fields_ = [("pos", ol.V3), ("dir", ol.V3), ("up", ol.V3), ("res", C.c_size_t * 2), ("near_", C.c_float), ("far_", C.c_float), ("vfov_deg", C.c_float),
                ("matr_P", C.c_double * 16), ("matr_V", C.c_double * 16), ("matr_PV_inv", C.c_double * 16)]


class _OrcSceneHead(C.Structure):  # the first members of orc_scene
    _fields_ = [("camera", _OrcCamera), ("materials", C.POINTER(_OrcMaterial)), ("n_materials", C.c_int)]


class _OrcColorHead(C.Structure):  # the first members of orc_color
    _fields_ = [("observer", C.c_int), ("lambda_min", C.c_float), ("lambda_max", C.c_float), ("lambda_step", C.c_float)]


def camera_rays(orc, W, H):
    """Pixel-centre ray directions float32 [H, W, 3]: camera_dir (csrc/ssx_kernels.hip; reference renderer.cpp:114-131) and the normalisation of
    generate_sample, in float64 operation by operation."""
    pv = np.array(orc.lib.orc_scene_pv_inv(orc.scene)[:16], dtype=np.float64)      # column-major m[col * 4 + row]
    cam = np.array(orc.lib.orc_scene_cam_pos(orc.scene)[:3], dtype=np.float32).astype(np.float64)
    x = (np.arange(W, dtype=np.float64) + 0.5)[None, :] + np.zeros((H, 1))
    y = (np.arange(H, dtype=np.float64) + 0.5)[:, None] + np.zeros((1, W))
    ndc_x = (x / np.float64(W)) * 2.0 - 1.0
    ndc_y = (y / np.float64(H)) * 2.0 - 1.0
    q = [(pv[0 * 4 + r] * ndc_x + pv[1 * 4 + r] * ndc_y) + (pv[2 * 4 + r] * 0.0 + pv[3 * 4 + r] * 1.0) for r in range(4)]
    d = [q[k] / q[3] - cam[k] for k in range(3)]
    inv = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return np.stack([(d[k] * inv).astype(F) for k in range(3)], axis=-1), cam.astype(F)


def guides_ref(orc, W, H, rgb=False):
    """{"prim", "depth", "normal", "albedo"} as ssx_guides defines them, from orc_scene_intersect and orc_material_albedo.  The observer (lambda_min and
    lambda_step of lambda_g) and the uplift are those of `orc`'s colour tables: an Oracle made with observer=2006, jh= or meng= needs nothing more."""
    lib = orc.lib
    lib.orc_material_albedo.restype = None
    lib.orc_material_albedo.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_OrcMaterial), ol.V2, C.c_float, C.POINTER(C.c_float), C.c_void_p]
    head = C.cast(orc.scene, C.POINTER(_OrcSceneHead)).contents
    col = C.cast(orc.color, C.POINTER(_OrcColorHead)).contents
    lambda_g = F(0) if rgb else F(col.lambda_min) + F(0.5) * F(col.lambda_step)
    dirs, cam = camera_rays(orc, W, H)
    g = {"prim": np.full((H, W), MISS, dtype=np.uint32), "depth": np.zeros((H, W), F), "normal": np.zeros((H, W, 3), F), "albedo": np.zeros((H, W, 4), F)}
    hit, out = ol.Hit(), (C.c_float * 4)()
    for j in range(H):
        for i in range(W):
            ray = ol.Ray(ol.V3(*[float(v) for v in cam]), ol.V3(*[float(v) for v in dirs[j, i]]))
            if not lib.orc_scene_intersect(orc.scene, C.byref(ray), C.byref(hit), -1, None):
                continue
            m = lib.orc_scene_quad_material(orc.scene, hit.prim)
            assert 0 <= m < head.n_materials
            lib.orc_material_albedo(orc.color, orc.scene, C.byref(head.materials[m]), hit.st, C.c_float(float(lambda_g)), out, None)
            g["prim"][j, i] = hit.prim
            g["depth"][j, i] = hit.dist
            g["normal"][j, i] = (hit.normal.x, hit.normal.y, hit.normal.z)
            g["albedo"][j, i] = out[:]
    return g


def synthetic(W, H, seed):
    """Inputs that reach every branch of the filter: blobs of three primitive ids plus misses, random colour and albedo, variances including 0, a
    denormal and inf, one NaN colour pixel.  Returns (c, var, prim, albedo)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    prim = np.full((H, W), MISS, dtype=np.uint32)
    for k, (cx, cy, r) in enumerate(((0.25, 0.3, 0.35), (0.7, 0.6, 0.4), (0.5, 0.95, 0.3))):
        prim[(xx - cx * W) ** 2 + (yy - cy * H) ** 2 <= (r * max(W, H)) ** 2] = k * 5 + 1
    c = g.uniform(0, 4, size=(H, W, 4)).astype(F)
    c[..., 3] = g.integers(0, 2, size=(H, W)).astype(F)
    albedo = (g.uniform(0, 1, size=(H, W, 4)) * (0.2 + 0.8 * (prim[..., None] % 3 == 1))).astype(F)
    var = (g.uniform(0, 0.5, size=(H, W)) ** 2).astype(F)
    flat = g.permutation(W * H)
    var.flat[flat[0]] = F(0)
    var.flat[flat[1]] = np.uint32(0x00000123).view(F)     # a denormal
    var.flat[flat[2]] = F(np.inf)
    c.reshape(-1, 4)[flat[3], g.integers(0, 3)] = F(np.nan)
    if W * H > 8:
        var.flat[flat[4:6]] = F(0)
    return c, var, prim, albedo


def sample_first_hits(orc, W, H, spp, seed):
    """int32 [H, W, spp]: the primitive the camera ray of sample k of pixel (i, j) hits first (-1: none) -- the sub-pixel offset as orc_render_sample draws
    it (two doubles, y first) and the direction as camera_rays states it."""
    lib = orc.lib
    pv = np.array(lib.orc_scene_pv_inv(orc.scene)[:16], dtype=np.float64)
    cam32 = np.array(lib.orc_scene_cam_pos(orc.scene)[:3], dtype=np.float32)
    cam = cam32.astype(np.float64)
    out = np.full((H, W, spp), -1, dtype=np.int32)
    rng, hit = ol.Rng(), ol.Hit()
    for j in range(H):
        for i in range(W):
            for k in range(spp):
                lib.orc_seed_sample(seed, j * W + i, k, C.byref(rng))
                sy = lib.orc_rand_1d(C.byref(rng)); sx = lib.orc_rand_1d(C.byref(rng))
                nx, ny = ((i + sx) / float(W)) * 2.0 - 1.0, ((j + sy) / float(H)) * 2.0 - 1.0
                q = [(pv[0 * 4 + r] * nx + pv[1 * 4 + r] * ny) + (pv[2 * 4 + r] * 0.0 + pv[3 * 4 + r] * 1.0) for r in range(4)]
                d = [q[a] / q[3] - cam[a] for a in range(3)]
                inv = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                ray = ol.Ray(ol.V3(*[float(v) for v in cam32]), ol.V3(*[float(np.float32(d[a] * inv)) for a in range(3)]))
                if lib.orc_scene_intersect(orc.scene, C.byref(ray), C.byref(hit), -1, None):
                    out[j, i, k] = hit.prim
    return out


# ---- sizes: which pixels and workgroups a level treats alike ---------------------------------------------------------------------------------------------

def interior_pixels(W, H, step):
    """The number of pixels whose 25 taps at `step` all lie inside a W x H image."""
    return max(0, W - 4 * step) * max(0, H - 4 * step)


def lds_tile_classes(W, H, step):
    """Of the 16 x 16-pixel workgroups of a W x H image, whose taps at `step` lie in a tile of T x T pixels, T = 16 + 4 step, around them: how many tiles
    lie wholly inside the image, and how many are cut by the left, right, bottom and top border."""
    n = dict(inside=0, left=0, right=0, bottom=0, top=0)
    for by in range((H + 15) // 16):
        for bx in range((W + 15) // 16):
            x0, y0, x1, y1 = bx * 16 - 2 * step, by * 16 - 2 * step, bx * 16 + 16 + 2 * step, by * 16 + 16 + 2 * step
            cut = dict(left=x0 < 0, right=x1 > W, bottom=y0 < 0, top=y1 > H)
            for k, v in cut.items():
                n[k] += int(v)
            n["inside"] += int(not any(cut.values()))
    return n


# ---- values at the edges of binary32 ----------------------------------------------------------------------------------------------------------------------

FLT_MAX = np.finfo(F).max
FLT_MIN = np.finfo(F).tiny        # the smallest normal number


def is_denormal(a):
    a = np.asarray(a, dtype=F)
    return (a != 0) & (np.abs(a) < FLT_MIN)


def extras_with_specials(c, var, seed):
    """80 channels; in valid pixels: a NaN, negative zeros and a denormal in channel 0 (what E = 1 sees), an infinity in channel 1, a channel of negative
    zeros (2), a channel of denormals (4), an infinity in the last"""
    H, W = var.shape
    g = np.random.default_rng(seed)
    e = g.uniform(-2, 6, size=(H, W, 80)).astype(F)
    ok = np.flatnonzero(valid_mask(c, var))
    at = ok[g.permutation(len(ok))]
    flat = e.reshape(-1, 80)
    flat[at[0], 0] = F(np.nan)
    flat[at[1 % len(at)], 1] = F(np.inf)
    flat[at[2 % len(at)], 0] = F(-0.0); flat[at[3 % len(at)], 0] = F(-0.0)
    flat[at[4 % len(at)], 0] = np.uint32(0x00000007).view(F)
    flat[:, 2] = F(-0.0)
    flat[:, 4] = g.integers(1, 0x007FFFFF, size=H * W).astype(np.uint32).view(F) * np.where(g.integers(0, 2, size=H * W) == 1, F(1), F(-1))
    flat[at[5 % len(at)], 79] = F(np.inf)
    assert np.isnan(e).sum() == 1 and np.isinf(e).sum() == 2 and np.signbit(e[e == 0]).all()
    return e


# the patches of synthetic_extreme: name -> (x0, y0, x1, y1, primitive id), x1 and y1 exclusive
EXTREME_PATCHES = {
    "zero_weight": (2, 2, 12, 12, 100),      # var 0, luminance +-1e20 in a checkerboard: xl * xl = +inf, w = +0; inside, den == 1e-6f
    "denormal_weight": (14, 2, 24, 12, 101), # var 0, luminance 0 / 1.2e13 by column: wl = 1 / (1 + 1.44e38) is a denormal
    "albedo_inf": (26, 2, 36, 12, 102),      # albedo.x 0 / 4.5e18 in a checkerboard: da2 = 2e37 is finite, da2 * inv_sa2 = +inf
    "albedo_nan": (38, 2, 48, 12, 103),      # one valid pixel with albedo.y = +inf: its own centre tap is inf - inf
    "colour_max": (2, 16, 22, 36, 104),      # X = FLT_MAX: sum(w X) / sum(w) rounds past FLT_MAX in some pixels, which are invalid from the next level on
    "variance_max": (26, 16, 46, 36, 105),   # var in [FLT_MAX / 2, FLT_MAX]: the 3x3 sum of g overflows, den = +inf; one NaN variance
}
EXTREME_NAN_ALBEDO = (42, 6)                 # (x, y)
EXTREME_LONELY = (54, 6)                     # a primitive id of its own: only the centre tap counts, at every step
EXTREME_NAN_VARIANCE = (30, 20)


def synthetic_extreme(W, H, seed):
    """`synthetic` with patches (EXTREME_PATCHES, each a primitive of its own) whose values sit at the edges of binary32.  Returns (c, var, prim, albedo).

    What cannot be reached, by the definition itself: a tap's w = (k * wl) * wa is at most k <= 9/64, so (w * w) * vq is smaller than vq and never overflows;
    sv / (sw * sw) is a weighted mean of the taps' variances times sum(w^2) / sum(w)^2 <= 1, equal to 1 only for a single tap, and there
    fl(fl(81/4096 v) / (81/4096)) <= FLT_MAX for every finite v (81 (2^24 - 1) rounds down to 24 bits).  A finite variance therefore stays finite, and a pixel
    that is valid on input can turn invalid later only through its colour: the "colour_max" patch, where the rounding of sum(w X) against that of sum(w)
    carries X = FLT_MAX to +inf.  tests/test_pipeline_matrix_cpu.py holds both statements against the restatement."""
    assert W >= 60 and H >= 36
    c, var, prim, albedo = synthetic(W, H, seed)
    g = np.random.default_rng(seed + 1)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = ((xx + yy) & 1).astype(bool)
    for x0, y0, x1, y1, pid in EXTREME_PATCHES.values():
        sl = (slice(y0, y1), slice(x0, x1))
        prim[sl] = pid
        c[sl] = g.uniform(0, 4, size=(y1 - y0, x1 - x0, 4)).astype(F)        # no NaN of `synthetic` inside a patch
        var[sl] = (g.uniform(0.01, 0.5, size=(y1 - y0, x1 - x0)) ** 2).astype(F)
        albedo[sl] = g.uniform(0, 1, size=(y1 - y0, x1 - x0, 4)).astype(F)
    patch = lambda name: (slice(EXTREME_PATCHES[name][1], EXTREME_PATCHES[name][3]), slice(EXTREME_PATCHES[name][0], EXTREME_PATCHES[name][2]))
    sl = patch("zero_weight")
    var[sl] = F(0); albedo[sl] = F(0.5)
    c[sl + (1,)] = np.where(checker[sl], F(1e20), F(-1e20))
    sl = patch("denormal_weight")
    var[sl] = F(0); albedo[sl] = F(0.25)
    c[sl + (1,)] = np.where((xx[sl] & 1) == 1, F(1.2e13), F(0))
    sl = patch("albedo_inf")
    albedo[sl + (0,)] = np.where(checker[sl], F(4.5e18), F(0))
    x, y = EXTREME_NAN_ALBEDO
    albedo[y, x, 1] = F(np.inf)
    sl = patch("colour_max")
    c[sl + (0,)] = FLT_MAX; albedo[sl] = F(0.5)
    sl = patch("variance_max")
    var[sl] = (FLT_MAX * g.uniform(0.5, 1.0, size=var[sl].shape)).astype(F)
    x, y = EXTREME_NAN_VARIANCE
    var[y, x] = F(np.nan)
    x, y = EXTREME_LONELY
    prim[y, x] = 999; c[y, x, :3] = g.uniform(0, 4, size=3).astype(F); var[y, x] = F(0.01)
    return c, var, prim, albedo


def extras_extreme(c, var, seed):
    """`extras_with_specials` with channel 6 = +FLT_MAX in the left half of the image and -FLT_MAX in the right (a tap sum of equal signs: sum(w e) / sum(w)
    rounds past FLT_MAX in some pixels; of both signs at the seam) and channel 7 = +-FLT_MAX in a checkerboard; channel 4 stays the channel of denormals."""
    e = extras_with_specials(c, var, seed)
    H, W = var.shape
    yy, xx = np.mgrid[0:H, 0:W]
    e[..., 6] = np.where(xx < W // 2, FLT_MAX, -FLT_MAX)
    e[..., 7] = np.where(((xx + yy) & 1) == 1, FLT_MAX, -FLT_MAX)
    return e


def level_trace(c, var, prim, albedo, step, sigma_l, sigma_a):
    """What atrous_level computes on the way, for the tests that must show an input reaches a branch: den [H, W], and per tap t = (dy + 2) * 5 + (dx + 2)
    the arrays xl2 = xl * xl, da2s = da2 * inv_sa2, w and counted (the tap takes part), each [25, H, W].  The same expressions in the same order."""
    H, W = var.shape
    valid = valid_mask(c, var)
    sigma_l, sigma_a = F(sigma_l), F(sigma_a)
    inv_sa2 = F(1) / (sigma_a * sigma_a)
    out = dict(xl2=np.zeros((25, H, W), F), da2s=np.zeros((25, H, W), F), w=np.zeros((25, H, W), F), counted=np.zeros((25, H, W), bool))
    with np.errstate(all="ignore"):
        gs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, qy, qx = _tap(H, W, dy, dx)
                m = inside & valid[qy, qx]
                k3 = F((2 if dy == 0 else 1) * (2 if dx == 0 else 1))
                gs = np.where(m, gs + k3 * var[qy, qx], gs)
                ks = np.where(m, ks + k3, ks)
        den = sigma_l * np.sqrt(gs / ks) + F(1e-6)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                t = (dy + 2) * 5 + (dx + 2)
                inside, qy, qx = _tap(H, W, step * dy, step * dx)
                out["counted"][t] = inside & valid[qy, qx] & (prim[qy, qx] == prim) & valid
                x = np.abs(c[qy, qx, 1] - c[..., 1]) / den
                out["xl2"][t] = x * x
                wl = F(1) / (F(1) + x * x)
                d = albedo[qy, qx] - albedo
                da2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
                out["da2s"][t] = da2 * inv_sa2
                out["w"][t] = ((H5[dy + 2] * H5[dx + 2]) * wl) * (F(1) / (F(1) + da2 * inv_sa2))
    out["den"] = den
    out["gs"] = gs
    return out


def synthetic_large(W, H, seed):
    """`synthetic` with one primitive over nearly the whole image (a block of another one and a block of misses in two corners): at the widest step the
    pixels whose 25 taps lie inside the image also count them all, which the blobs of `synthetic` -- smaller than a footprint of 129 pixels -- never do."""
    c, var, prim, albedo = synthetic(W, H, seed)
    prim[:] = 1
    prim[:10, :10] = 2
    prim[-10:, -10:] = MISS
    return c, var, prim, albedo
