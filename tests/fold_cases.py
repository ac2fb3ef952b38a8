"""Level lists for the path fold, independent of any log layout: what tests/test_fold_cpu.py (the oracle alone) and tests/test_fold_gpu.py
(ssx_debug_fold against orc_fold_levels) share.  A sample is one row of ROW 32-bit words -- the oracle's orc_fold_sample, include/ssx.h's
ssx_debug_fold row -- and a case is 64 pixels x 1..5 samples per pixel, rows in [pixel][k] order.  Everything is seeded."""
import ctypes as C

import numpy as np

import oracle_lib as ol

ROW, LEVEL0, LEVEL_WORDS = 160, 10, 15                      # orc_fold_sample / SSX_FOLD_ROW_WORDS
LAMBDA0, CAM_DIR, HIT, N, FLUX = 0, 1, 4, 5, 6
L_FS, L_NDL, L_PDF, L_FLAGS, L_EMISSION, L_NEE = 0, 4, 5, 6, 7, 11
EMISSION, NEE, NEE_VISIBLE = 1, 2, 4
COHORT_KS = 2                                               # SSX_COHORT_KS: samples per pixel in one pass of the fold
FLT_MAX, FLT_MIN, DENORM = np.float32(3.4028235e38), np.float32(1.17549435e-38), np.float32(1e-45)


def f2u(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def u2f(x):
    return np.ascontiguousarray(x, dtype=np.uint32).view(np.float32)


def bind(lib):
    lib.orc_debug_set_level_log.argtypes = [C.c_void_p]
    lib.orc_debug_set_level_log.restype = None
    lib.orc_fold_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    lib.orc_fold_levels.restype = None
    lib.orc_pixel_sums.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_size_t] * 5 + [C.c_int, C.c_void_p]
    lib.orc_pixel_sums.restype = None
    return lib


def oracle_fold(orc, rows, flat_field=True):
    """orc_fold_levels on [n, ROW] rows -> (flux uint32 [n, 4], xyza uint32 [n, 4])"""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    assert rows.ndim == 2 and rows.shape[1] == ROW
    flux, xyza = np.full((len(rows), 4), 0xDEADBEEF, dtype=np.uint32), np.full((len(rows), 4), 0xDEADBEEF, dtype=np.uint32)
    bind(orc.lib).orc_fold_levels(orc.color, orc.scene, rows.ctypes.data, len(rows), 0 if flat_field else 4, flux.ctypes.data, xyza.ctypes.data)
    return flux, xyza


def pixel_sums(xyza_u32, spp, rgb):
    """renderer.cpp:292-295 (:301-303 in RGB mode) restated: per pixel, in ascending k, avg += double(float(x * 0.001f)) -- or the plain add."""
    x = u2f(xyza_u32).reshape(-1, spp, 4)
    acc = np.zeros((x.shape[0], 4), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(spp):
            acc += (x[:, k] if rgb else x[:, k] * np.float32(0.001)).astype(np.float64)
    return acc


# ---- rows -------------------------------------------------------------------------------------------------------------------------------

def level(rows, l):
    return rows[:, LEVEL0 + l * LEVEL_WORDS:LEVEL0 + (l + 1) * LEVEL_WORDS]


def counts(rows):
    """what a set of rows reaches, from the rows themselves (tests/test_fold_cpu.py asserts these per claim)"""
    n = rows[:, N].astype(np.int64)
    c = dict(samples=len(rows), depth9=int((n == 9).sum()), misses=int((rows[:, HIT] == 0).sum()), emission_below_last=0, both_terms=0, occluded=0, inf_pdf=0,
             depth_hist=np.bincount(n, minlength=10).tolist())
    for l in range(10):
        lv = level(rows, l)
        fl = lv[:, L_FLAGS]
        live, below = n >= l, n > l
        c["emission_below_last"] += int((below & ((fl & EMISSION) != 0)).sum())
        c["both_terms"] += int((live & ((fl & (EMISSION | NEE)) == (EMISSION | NEE))).sum())
        c["occluded"] += int((live & ((fl & (NEE | NEE_VISIBLE)) == NEE) & (lv[:, L_NEE:L_NEE + 4] != 0).any(axis=1)).sum())
        c["inf_pdf"] += int((below & np.isinf(u2f(lv[:, L_PDF]))).sum())
    return c


class Case:
    def __init__(self, name, spp, rows, replay=None):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        assert rows.shape == (64 * spp, ROW), (name, rows.shape)
        self.name, self.spp, self.rows, self.replay = name, spp, rows, replay  # replay: (config key, expected flux, expected xyza, pixel means)

    @property
    def partial_cohort(self):
        return self.spp % COHORT_KS != 0


def pack(name, samples, spp, g):
    """`samples` [m, ROW] -> one case of 64 pixels x spp: every sample at least once, the places left over filled by repeats, then shuffled over (pixel, k)"""
    need = 64 * spp
    assert len(samples) <= need, (name, len(samples), need)
    idx = np.concatenate([np.arange(len(samples)), g.integers(0, len(samples), size=need - len(samples))])
    return Case(name, spp, samples[g.permutation(idx)])


def ladder(g, n, last_em, last_nee, level_nee, em_below, lam, vis_p=0.75):
    """one sample of n continued levels with ordinary positive factors"""
    r = np.zeros(ROW, dtype=np.uint32)
    d = g.normal(size=3); d /= np.linalg.norm(d)
    r[LAMBDA0] = f2u([lam])[0]; r[CAM_DIR:CAM_DIR + 3] = f2u(d); r[HIT] = 1; r[N] = n
    for l in range(n + 1):
        v = r[LEVEL0 + l * LEVEL_WORDS:LEVEL0 + (l + 1) * LEVEL_WORDS]
        last = l == n
        fl = 0
        if (last_em if last else em_below):
            fl |= EMISSION; v[L_EMISSION:L_EMISSION + 4] = f2u(g.uniform(0.5, 40, size=4))
        if (last_nee if last else level_nee):
            fl |= NEE | (NEE_VISIBLE if g.uniform() < vis_p else 0); v[L_NEE:L_NEE + 4] = f2u(g.uniform(0.01, 9, size=4))
        v[L_FLAGS] = fl
        if not last:
            v[L_FS:L_FS + 4] = f2u(g.uniform(0.02, 0.32, size=4)); v[L_NDL] = f2u([g.uniform(0.01, 1)])[0]; v[L_PDF] = f2u([g.uniform(0.004, 0.3183)])[0]
    return r


def lambdas(lambda_min, lambda_step, g, n):
    """lambda_0 as unit_cases.flux_inputs chooses it: both ends of the range the observer tables are sampled over, just inside the upper one, the middle, then random"""
    lam = (lambda_min + g.uniform(0, 1, size=n) * lambda_step).astype(np.float32)
    lam[:4] = (lambda_min, lambda_min + lambda_step, np.nextafter(np.float32(lambda_min + lambda_step), np.float32(0)), lambda_min + 0.5 * lambda_step)
    return lam


def synthetic_ladders(lambda_min, lambda_step, seed=25):
    """every n in 0..9 x {last-level emission} x {last-level next-event term} x {per-level next-event term} x {emission below the last level}: 160 samples"""
    g = np.random.default_rng(seed)
    combos = [(n, a, b, c, d) for n in range(10) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]
    lam = lambdas(lambda_min, lambda_step, g, len(combos))
    return np.stack([ladder(g, n, a, b, c, d, lam[i]) for i, (n, a, b, c, d) in enumerate(combos)])


NAN_LANE = "nan-in-one-lane"
EDGE_VALUES = [("+0", np.float32(0.0)), ("-0", np.float32(-0.0)), ("denormal", DENORM), ("-denormal", -np.float32(1e-40)), ("flt_max", FLT_MAX), ("-flt_max", -FLT_MAX),
               ("flt_min", FLT_MIN), ("one", np.float32(1.0)), ("inf", np.float32(np.inf)), (NAN_LANE, np.float32(np.nan))]
EDGE_POSITIONS = ["fs", "n_dot_l", "pdf", "emission", "nee", "last_emission", "last_nee"]


def edge_samples(lambda_min, lambda_step, seed=26):
    """A full ladder (both terms on every level, everything visible) of n = 1, 3 and 9 continued levels with one edge value in one factor position -- all four
    hero lanes, except NaN, which takes one lane only -- at the level in the middle of the path (or the last); then the named specials."""
    g = np.random.default_rng(seed)
    out, names = [], []
    for n in (1, 3, 9):
        for pos in EDGE_POSITIONS:
            for vname, val in EDGE_VALUES:
                r = ladder(g, n, 1, 1, 1, 1, lambda_min + g.uniform() * lambda_step, vis_p=1.0)
                l = n if pos.startswith("last_") else n // 2
                v = r[LEVEL0 + l * LEVEL_WORDS:LEVEL0 + (l + 1) * LEVEL_WORDS]
                at = {"fs": L_FS, "n_dot_l": L_NDL, "pdf": L_PDF, "emission": L_EMISSION, "nee": L_NEE, "last_emission": L_EMISSION, "last_nee": L_NEE}[pos]
                width = 1 if pos in ("n_dot_l", "pdf") else 4
                if vname == NAN_LANE and width == 4:
                    v[at + int(g.integers(0, 4))] = f2u([val])[0]
                else:
                    v[at:at + width] = f2u([val])[0]
                out.append(r); names.append("n%d/%s/%s" % (n, pos, vname))
    lam = lambda_min + 0.25 * lambda_step

    def special(name, r):
        out.append(r); names.append(name)
    # a next-event term of -0 with a -0 indirect term under it, alone on its level (the issue's suspicion): L() starts the level from a literal 0
    for n in (1, 4):
        r = ladder(g, n, 0, 0, 0, 0, lam)
        v = level(r[None], n - 1)[0]
        v[L_FLAGS] = NEE | NEE_VISIBLE; v[L_NEE:L_NEE + 4] = f2u([-0.0] * 4); v[L_FS:L_FS + 4] = f2u([-0.25] * 4)     # (+0 * n_dot_l) * -0.25 = -0
        special("minus-zero/nee-over-indirect/n%d" % n, r)
        r = r.copy(); v = level(r[None], n - 1)[0]
        v[L_FLAGS] = EMISSION; v[L_EMISSION:L_EMISSION + 4] = f2u([-0.0] * 4)
        special("minus-zero/emission-over-indirect/n%d" % n, r)
        r = ladder(g, n, 0, 0, 0, 0, lam)
        v = level(r[None], n)[0]
        v[L_FLAGS] = EMISSION | NEE | NEE_VISIBLE; v[L_EMISSION:L_EMISSION + 4] = f2u([-0.0] * 4); v[L_NEE:L_NEE + 4] = f2u([-0.0] * 4)
        special("minus-zero/last-level-both/n%d" % n, r)
    # products that overflow: FLT_MAX radiance below times factors above 1, and FLT_MAX / smallest normal
    r = ladder(g, 3, 1, 0, 0, 0, lam); level(r[None], 3)[0][L_EMISSION:L_EMISSION + 4] = f2u([FLT_MAX] * 4); level(r[None], 2)[0][L_NDL] = f2u([2.0])[0]
    special("overflow/flt_max-times-two", r)
    r = ladder(g, 2, 1, 0, 0, 0, lam); level(r[None], 2)[0][L_EMISSION:L_EMISSION + 4] = f2u([FLT_MAX] * 4); level(r[None], 1)[0][L_PDF] = f2u([FLT_MIN])[0]
    special("overflow/over-smallest-normal-pdf", r)
    # a mirror chain as the kernel logs it (n_dot_l = pdf = 1) and the raw +inf pdf of a delta BSDF; pdf 1 and the smallest normal on every level
    for name, pdf in (("pdf-one", 1.0), ("pdf-inf", np.inf), ("pdf-smallest-normal", FLT_MIN)):
        r = ladder(g, 9, 1, 1, 1, 0, lam)
        for l in range(9):
            level(r[None], l)[0][L_PDF] = f2u([pdf])[0]; level(r[None], l)[0][L_NDL] = f2u([1.0])[0]
        special("every-level/" + name, r)
    # occluded: a non-zero term on every level and none of them visible
    r = ladder(g, 9, 0, 1, 1, 0, lam, vis_p=0.0); special("occluded/all-nine-levels", r)
    r = ladder(g, 9, 1, 1, 1, 1, lam, vis_p=0.0); special("occluded/with-emission", r)
    return np.stack(out), names


def miss(lam, g):
    r = np.zeros(ROW, dtype=np.uint32)
    d = g.normal(size=3); d /= np.linalg.norm(d)
    r[LAMBDA0] = f2u([lam])[0]; r[CAM_DIR:CAM_DIR + 3] = f2u(d)
    return r


def synthetic_cases(lambda_min, lambda_step):
    """the synthetic cases for a context whose observer tables are sampled over [lambda_min, lambda_min + lambda_step]"""
    g = np.random.default_rng(27)
    lad = synthetic_ladders(lambda_min, lambda_step)
    edge, _ = edge_samples(lambda_min, lambda_step)
    cases = [pack("ladders-spp3", lad, 3, g), pack("ladders-spp2", lad[::2], 2, g), pack("edges-spp5", edge, 5, g), pack("edges-spp4", edge[:256], 4, g)]
    # misses (alpha = 0) between hits in one pixel: k = 0, 2, 4 hit, k = 1, 3 do not; and one sample per pixel, all nine levels
    rows = np.stack([lad[int(g.integers(0, len(lad)))] if k % 2 == 0 else miss(lambda_min + g.uniform() * lambda_step, g) for _ in range(64) for k in range(5)])
    cases.append(Case("misses-between-hits-spp5", 5, rows))
    deep = np.stack([ladder(g, 9, int(g.integers(0, 2)), 1, 1, int(g.integers(0, 2)), lambda_min + g.uniform() * lambda_step) for _ in range(64)])
    cases.append(Case("depth9-spp1", 1, deep))
    # sums whose binary64 additions do not commute: a pixel's samples differ by more than 2^53 in size, so adding them in another order than ascending k
    # (renderer.cpp:292-295) gives other sums -- ordinary samples, 24-bit values of similar size, add exactly in binary64 in any order
    for name, vals in (("sum-order-spp3", (1e30, -1e30, 1.0)), ("sum-order-spp5", (3e20, 1.0, -3e20, 1e-3, 7.0))):
        rows = []
        for _ in range(64):
            lam, scale = lambda_min + g.uniform() * lambda_step, g.uniform(0.5, 1.0, size=4).astype(np.float32)   # the pixel's: its large samples cancel exactly
            for v in vals:
                r = ladder(g, 0, 1, 0, 0, 0, lam)
                level(r[None], 0)[0][L_EMISSION:L_EMISSION + 4] = f2u(np.float32(v) * (scale if abs(v) > 1e10 else g.uniform(0.5, 1.0, size=4).astype(np.float32)))
                rows.append(r)
        cases.append(Case(name, len(vals), np.stack(rows)))
    return cases


# ---- replayed levels: the oracle's own, recorded by orc_debug_set_level_log ------------------------------------------------------------------

TILES = [(0, 0), (8, 8), (16, 0)]   # three 8x8 tiles of a 24 x 16 image
W, H, SEED = 24, 16, 2025


def _mirror_cornell():
    o = ol.Oracle("cornell-srgb", texture="test-img.png")
    for q in (0, 1):   # floor and the next quad reflect: emission is then met below the last level of paths that reach the light by a bounce
        assert o.lib.orc_scene_set_material_kind(o.scene, o.lib.orc_scene_quad_material(o.scene, q), 1) == 0
    return o


REPLAY_CONFIGS = {   # key: (oracle, observer key, spp, render flags of orc_render_sample: 1 indirect-only | 2 without explicit light sampling)
    "cornell-srgb": (lambda: ol.Oracle("cornell-srgb", texture="test-img.png"), 1931, 3, 0),
    "plane-srgb": (lambda: ol.Oracle("plane-srgb", texture="test-img.png"), 1931, 2, 0),
    "cornell-2006": (lambda: ol.Oracle("cornell", observer=2006), 2006, 5, 0),
    "mirror-no-els": (_mirror_cornell, 1931, 4, 2),
    "indirect-only": (lambda: ol.Oracle("cornell-srgb", texture="test-img.png"), 1931, 1, 1),
}
_replayed = {}


def replay_cases(key):
    """-> (oracle, flags, [Case]): per tile of TILES one case; Case.replay = (key, flux, xyza of orc_render_sample, the pixels' means of orc_render, their binary64 sums of orc_pixel_sums)"""
    if key in _replayed:
        return _replayed[key]
    make, _, spp, flags = REPLAY_CONFIGS[key]
    orc = make()
    lib = bind(orc.lib)
    rec = np.zeros(ROW, dtype=np.uint32)
    rng, out = ol.Rng(), (C.c_float * 4)()
    image = np.zeros((H, W, 4), dtype=np.float32)
    assert lib.orc_render(orc.color, orc.scene, SEED, W, H, 0, 0, W, H, spp, flags, 1, image.ctypes.data, None) == 0
    cases = []
    for (i0, j0) in TILES:
        rows, flux, xyza = np.zeros((64 * spp, ROW), dtype=np.uint32), np.zeros((64 * spp, 4), dtype=np.uint32), np.zeros((64 * spp, 4), dtype=np.uint32)
        for p in range(64):
            i, j = i0 + (p & 7), j0 + (p >> 3)
            for k in range(spp):
                lib.orc_seed_sample(SEED, j * W + i, k, C.byref(rng))
                lib.orc_debug_set_level_log(rec.ctypes.data)
                try:
                    lib.orc_render_sample(orc.color, orc.scene, C.byref(rng), i, j, W, H, flags, out, None)
                finally:
                    lib.orc_debug_set_level_log(None)
                rows[p * spp + k] = rec; flux[p * spp + k] = rec[FLUX:FLUX + 4]; xyza[p * spp + k] = f2u(out[:])
        means = image[j0:j0 + 8, i0:i0 + 8].reshape(64, 4).copy()
        sums = np.zeros((64, 4), dtype=np.float64)   # the oracle's own binary64 accumulators (orc_pixel_sums), before orc_render divides and rounds them
        for p in range(64):
            lib.orc_pixel_sums(orc.color, orc.scene, SEED, i0 + (p & 7), j0 + (p >> 3), W, H, spp, flags, sums[p].ctypes.data)
        cases.append(Case("%s/tile-%d-%d" % (key, i0, j0), spp, rows, replay=(key, flux, xyza, means, sums)))
    _replayed[key] = (orc, flags, cases)
    return _replayed[key]
