"""Synthetic sample records for ssx_spectral_bin_kernel and ssx_spectral_moment_kernel (run through ssx_debug_spectral_accumulate) and the reference they are
held to: include/ssx.h "Spectral radiance output" and "Spectral moments" restated sequentially.  Pure numpy, no GPU: tests/test_spectral_accumulate_cpu.py
proves on the restatement alone that a subtly wrong kernel would change a word on these inputs, tests/test_spectral_accumulate_gpu.py holds the kernels to
them bit for bit.  TEST INFRASTRUCTURE; every array is computed once per process and is read-only.

    t = (lambda_0 - lambda_min) / lambda_step;  m = min(M-1, (uint32)(t * (float)M))            binary32
    S[i*M+m] += (double)f[i];   N[m] += 1;   Q[i*M+m] += (double)f[i] * (double)f[i]           binary64, ascending k

Every lambda_0 lies inside [lambda_min, lambda_min + lambda_step]: outside it the conversion to unsigned is not defined and not part of the contract."""
import functools
from typing import NamedTuple

import numpy as np

import spectral_ref
from simple_spectral_amd.renderer import Scene

F = np.float32
DOWN = F(-np.inf)
SIZES = ((1, 1), (9, 1), (1, 9), (17, 9), (13, 11))      # (W, H): one pixel; two tiles in a row / a column, ragged; 3 x 2 and 2 x 2 tiles, ragged both ways
ALL_BINS = tuple(range(4, 68, 4))                        # M = 1..16
WHOLE = (0, 1, 0)                                        # (tile_first, tile_stride, tile_skew): the whole image
FLT_MAX = np.finfo(F).max


class Case(NamedTuple):
    name: str
    flux: np.ndarray            # float32 [H, W, K, 4]
    lam: np.ndarray             # float32 [H, W, K]
    lambda_min: np.float32
    lambda_step: np.float32
    bins: int
    splits: tuple               # the launch lengths the records are given in: tuples that add up to K
    layouts: tuple = (WHOLE,)   # (tile_first, tile_stride, tile_skew)
    expected_index: np.ndarray = None   # int [H, W, K]: the bin index m written down from the construction, where the case has one


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(got, want):
    """bool array: the words that agree -- bit for bit, a NaN against any NaN (sign and payload of a generated NaN differ between x86 and the GPU)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    ok = bits(got) == bits(want)
    if got.dtype.kind == "f":
        ok |= np.isnan(got) & np.isnan(want)
    return ok


def differing(got, want):
    """words of (S, N, Q) triples that differ"""
    return sum(int((~same(g, w)).sum()) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def grid(observer):
    """(lambda_min, lambda_step) of the scenes' colour tables as the host library reports them: CIE 1931 or 2006"""
    scene = Scene("cornell-srgb", observer=observer, texture="test-img.png")     # (kept until the two numbers are copied: the description is the scene's)
    d = scene.desc.contents
    return F(d.lambda_min), F(d.lambda_step)


def top(lambda_min, lambda_step):
    """the upper end of the range, as binary32 adds it"""
    return F(F(lambda_min) + F(lambda_step))


# ---------------------------------------------------------------------------------------------------------------- the definition, and wrong ones ----
def bin_index(lam, lambda_min, lambda_step, bins, wrong=None):
    """m [H, W, K] int64 by the formula; -1: the sample is dropped.  wrong: None (the definition), or one of
         "wrap"        the clamp dropped, an index M wraps to 0          "discard"     the clamp dropped, an index M is not counted
         "round"       t * M rounded to nearest instead of truncated     "reciprocal"  t = (lambda_0 - lambda_min) * (1.0f / lambda_step)"""
    M = bins // 4
    d = np.asarray(lam, dtype=F) - F(lambda_min)
    t = d * (F(1.0) / F(lambda_step)) if wrong == "reciprocal" else d / F(lambda_step)
    x = t * F(M)
    assert x.dtype == F
    m = (np.rint(x) if wrong == "round" else x).astype(np.uint32).astype(np.int64)
    if wrong == "wrap":
        return m % M
    if wrong == "discard":
        return np.where(m >= M, -1, m)
    return np.minimum(m, M - 1)


def accumulate(flux, m, bins, order="ascending", product="binary64"):
    """(S float64 [H, W, B], N uint32 [H, W, M], Q float64 [H, W, B]) of the samples with bin indices m, pixel by pixel in plain Python floats (binary64).
       order: "ascending" (the definition), "reversed" (descending k), "interleaved4" (four partial sums k % 4, added ((p0 + p1) + p2) + p3 at the end)
       product: "binary64" (the definition: the product of the two converted values), "binary32" (rounded to binary32 first)"""
    H, W, K = m.shape
    M = bins // 4
    S, N, Q = np.zeros((H, W, bins)), np.zeros((H, W, M), dtype=np.uint32), np.zeros((H, W, bins))
    f64 = flux.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (flux * flux).astype(np.float64) if product == "binary32" else f64 * f64
        ks = range(K - 1, -1, -1) if order == "reversed" else range(K)
        ways = 4 if order == "interleaved4" else 1
        for j in range(H):
            for i in range(W):
                s, q = np.zeros((ways, bins)), np.zeros((ways, bins))
                for k in ks:
                    mm = m[j, i, k]
                    if mm < 0:
                        continue
                    N[j, i, mm] += 1
                    s[k % ways, mm::M] += f64[j, i, k]      # bins i * M + m of the four hero slots: distinct accumulators
                    q[k % ways, mm::M] += sq[j, i, k]
                S[j, i], Q[j, i] = s[0], q[0]
                for w in range(1, ways):
                    S[j, i] += s[w]; Q[j, i] += q[w]
    return S, N, Q


WRONG_INDEX = ("wrap", "discard", "round", "reciprocal")
WRONG_SUM = (("reversed", "binary64"), ("interleaved4", "binary64"), ("ascending", "binary32"))
WRONG = WRONG_INDEX + tuple("%s-k" % o if o != "ascending" else "%s-product" % p for o, p in WRONG_SUM)


def wrong_restatement(case, which):
    """(S, N, Q) of a deliberately wrong kernel: one of WRONG"""
    if which in WRONG_INDEX:
        return accumulate(case.flux, bin_index(case.lam, case.lambda_min, case.lambda_step, case.bins, which), case.bins)
    order, product = WRONG_SUM[WRONG.index(which) - len(WRONG_INDEX)]
    return accumulate(case.flux, bin_index(case.lam, case.lambda_min, case.lambda_step, case.bins), case.bins, order, product)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _reference(family, name):
    c = case(family, name)
    with np.errstate(over="ignore", invalid="ignore"):
        S, N, _ = spectral_ref.restate_bins(c.flux, c.lam, c.lambda_min, c.lambda_step, c.bins)
        Q = spectral_ref.restate_moments(c.flux, c.lam, c.lambda_min, c.lambda_step, c.bins)
    return _frozen(S, N, Q)


def reference(c):
    """(S, N, Q) of the whole image: the definition restated (tests/spectral_ref.py), once per case"""
    return _reference(*c.name.split("/", 1))


def owned(W, H, layout):
    """bool [H, W]: the pixels of the tiles the layout's tile list holds -- tile t' = ty * tiles_x + (tx + ty * skew) % tiles_x of the shared-out list belongs
    to the device with t' % tile_stride == tile_first (include/ssx.h ssx_render_params)"""
    first, stride, skew = layout
    tiles_x = (W + 7) // 8
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = (jj // 8) * tiles_x + (ii // 8 + (jj // 8) * skew) % tiles_x
    return t % stride == first


def reference_share(c, layout):
    """the whole image's (S, N, Q) with +0.0 / 0 where the layout owns nothing"""
    own = owned(c.lam.shape[1], c.lam.shape[0], layout)[:, :, None]
    return tuple(np.where(own, a, a.dtype.type(0)) for a in reference(c))


# ------------------------------------------------------------------------------------------------------------------------------------ inputs ----
def wide_flux(g, shape):
    """binary32 values of both signs whose magnitudes spread over 2^-30 .. 2^30 with full mantissas: neither their binary64 sums nor the sums of their squares
    (2^-60 .. 2^60) are exact, so both depend on the order"""
    return (g.standard_normal(shape) * np.exp2(g.integers(-30, 31, shape))).astype(F)


def render_like_flux(g, shape):
    """non-negative values of similar magnitude with a share of exact zeros (the samples that hit nothing), as a render's"""
    return np.where(g.random(shape) < 0.2, 0.0, g.random(shape) * 4.0).astype(F)


def uniform_lam(g, shape, lambda_min, lambda_step):
    """lambda_min + u * lambda_step in binary32 as the path kernel draws it, u in [0, 1)"""
    lam = F(lambda_min) + g.random(shape, dtype=F) * F(lambda_step)
    assert lam.dtype == F and (lam >= lambda_min).all() and (lam <= top(lambda_min, lambda_step)).all()
    return lam


def centre_lam(m, M, lambda_min, lambda_step):
    """a wavelength well inside bin m of M"""
    return (np.float64(lambda_min) + np.float64(lambda_step) * (np.asarray(m) + 0.5) / M).astype(F)


K_ORDER = 40
SPLITS = ((K_ORDER,), (1,) * K_ORDER, (3, 4, 5, 1, 2, 7, 3, 4, 5, 1, 2, 3), (4,) * (K_ORDER // 4))


def _order_case():
    """Even k: all in one bin of the pixel's, hero slot 0 the cancelling a, 1, -a, 1, ... (ascending k leaves 1, any other order another value), the other
    slots wide_flux.  Odd k: wide_flux spread over all bins."""
    W, H, K, bins = 17, 9, K_ORDER, 16
    M = bins // 4
    g = np.random.default_rng(7001)
    lmin, lstep = grid(1931)
    flux = wide_flux(g, (H, W, K, 4))
    a = (F(3e37) * (F(1.0) + (np.arange(H * W) % 7).astype(F) / F(8.0))).reshape(H, W)
    for n, k in enumerate(range(0, K, 2)):
        flux[:, :, k, 0] = (a, F(1.0), -a, F(1.0))[n % 4]
    lam = uniform_lam(g, (H, W, K), lmin, lstep)
    own_bin = (np.arange(H * W) % M).reshape(H, W, 1)
    lam[:, :, 0::2] = centre_lam(np.broadcast_to(own_bin, (H, W, K // 2)), M, lmin, lstep)
    assert sum(SPLITS[2]) == K and all(sum(s) == K for s in SPLITS)
    return Case("order/17x9", flux, lam, lmin, lstep, bins, SPLITS)


EDGE_M = (1, 2, 4, 8, 16)


def _edge_case(M):
    """lambda_min = 256, lambda_step = 64 and M a power of two: every lambda_min + lambda_step * m / M is a binary32 value, the difference, the quotient by 64
    and the product with M are exact, so the index of such a point is m by construction, the index of the value below it m - 1, and m = M (the upper end,
    t == 1) is held to M - 1 by the clamp alone.  2 M + 1 points, every pixel walks them from another start."""
    W, H = 9, 1
    lmin, lstep = F(256.0), F(64.0)
    pts, idx = [], []
    for m in range(M + 1):
        x = F(256.0 + 64.0 * m / M)
        assert float(x) == 256.0 + 64.0 * m / M
        pts.append(x); idx.append(min(m, M - 1))
        if m:
            pts.append(np.nextafter(x, DOWN)); idx.append(m - 1)
    pts, idx = np.array(pts, dtype=F), np.array(idx)
    K = len(pts)
    walk = (np.arange(K)[None, None, :] + 5 * np.arange(W)[None, :, None]) % K
    lam, expected = pts[walk], idx[walk]
    g = np.random.default_rng(7100 + M)
    return Case("edges/M%d" % M, render_like_flux(g, (H, W, K, 4)), lam, lmin, lstep, 4 * M, ((K,), (2, K - 2)), expected_index=expected)


def grid_points(observer, M):
    """binary32 values around every boundary of the scenes' grid at M bins: lambda_min + lambda_step * m / M rounded from binary64, its three neighbours on
    either side, and both ends of the range; kept inside [lambda_min, lambda_min + lambda_step]"""
    lmin, lstep = grid(observer)
    hi = top(lmin, lstep)
    pts = [lmin, hi]
    for m in range(M + 1):
        c = F(np.float64(lmin) + np.float64(lstep) * m / M)
        below = above = c
        pts.append(c)
        for _ in range(3):
            below, above = np.nextafter(below, DOWN), np.nextafter(above, F(np.inf))
            pts += [below, above]
    pts = np.unique(np.array(pts, dtype=F))
    return pts[(pts >= lmin) & (pts <= hi)]


def _grid_case(observer, M):
    """the points of grid_points dealt to the pixels of a 17 x 9 image, 16 to each, so that every point is some pixel's"""
    W, H, K = 17, 9, 16
    lmin, lstep = grid(observer)
    pts = grid_points(observer, M)
    assert len(pts) <= W * H * K
    lam = pts[(np.arange(H * W * K) % len(pts)).reshape(H, W, K)]
    g = np.random.default_rng(7200 + 100 * (observer == 2006) + M)
    return Case("grid/%d-M%d" % (observer, M), render_like_flux(g, (H, W, K, 4)), lam, lmin, lstep, 4 * M, ((K,),))


def _every_m_case(M):
    W, H, K = 13, 11, 24
    lmin, lstep = grid(2006 if M % 2 else 1931)
    g = np.random.default_rng(7300 + M)
    flux = np.where(g.random((H, W, K, 4)) < 0.5, render_like_flux(g, (H, W, K, 4)), wide_flux(g, (H, W, K, 4)))
    return Case("every_m/M%d" % M, flux, uniform_lam(g, (H, W, K), lmin, lstep), lmin, lstep, 4 * M, ((K,), (5, 7, 12)))


OWNERSHIP_LAYOUTS = (WHOLE, (1, 3, 1), (2, 3, 5))
STRIDE3_SKEWS = (1, 5)      # ... and with them all three shares of these two tile lists


def _ownership_case(W, H):
    K, bins = 7, 12
    lmin, lstep = grid(1931)
    g = np.random.default_rng(7400 + W)
    layouts = tuple(dict.fromkeys(OWNERSHIP_LAYOUTS + tuple((first, 3, skew) for skew in STRIDE3_SKEWS for first in range(3))))
    return Case("ownership/%dx%d" % (W, H), wide_flux(g, (H, W, K, 4)), uniform_lam(g, (H, W, K), lmin, lstep), lmin, lstep, bins, ((3, 4),), layouts)


# the special values: pixel (i, 0) of a 9 x 1 image, hero slot and bin of the value; every other record is render_like_flux in the bins 1..3 next to it
SPECIAL_BINS, SPECIAL_K = 16, 12
SPECIALS = {
    # name: (pixel i, hero slot, bin m, [(k, value), ...])
    "minus-zero-alone": (0, 1, 0, [(5, -0.0)]),
    "denormals": (1, 2, 0, [(0, 1e-45), (3, -4e-45), (4, 1.1754942e-38), (7, 1.0), (8, -1.0), (9, 1e-45)]),
    "denormals-only": (6, 3, 0, [(2, 1e-45), (5, 1.1754942e-38), (9, -7e-42)]),
    "flt-max": (2, 0, 0, [(1, FLT_MAX), (2, FLT_MAX), (6, -FLT_MAX), (10, FLT_MAX)]),
    "plus-inf": (3, 3, 0, [(2, np.inf), (6, 1.5)]),
    "inf-then-minus-inf": (4, 2, 0, [(1, 2.5), (3, np.inf), (4, 1.0), (8, -np.inf), (9, 3.0)]),
    "nan": (5, 1, 0, [(4, np.nan), (6, 2.0)]),
    "minus-inf-first": (8, 0, 0, [(0, -np.inf), (11, -FLT_MAX)]),
}


def _special_case():
    """Bin 0 of each special pixel holds the listed samples and nothing else (the other hero slots of those samples are render_like_flux); every other sample
    falls into bins 1..3.  The launch split (4, 4, 4) puts the -inf, the denormals and the FLT_MAXs of a pixel into other launches than their predecessors."""
    W, H, K, bins = 9, 1, SPECIAL_K, SPECIAL_BINS
    M = bins // 4
    lmin, lstep = grid(1931)
    g = np.random.default_rng(7500)
    flux = render_like_flux(g, (H, W, K, 4)) + F(0.125)        # no zeros here: a zero in bin 0 comes from the list only
    lam = centre_lam(g.integers(1, M, (H, W, K)), M, lmin, lstep)
    for i, slot, m, samples in SPECIALS.values():
        for k, v in samples:
            flux[0, i, k, slot] = F(v)
            lam[0, i, k] = centre_lam(m, M, lmin, lstep)
    return Case("special/9x1", flux, lam, lmin, lstep, bins, ((K,), (4, 4, 4), (1,) * K))


FAMILIES = {
    "order": {"17x9": _order_case},
    "edges": {"M%d" % M: functools.partial(_edge_case, M) for M in EDGE_M},
    "grid": {"%d-M%d" % (o, M): functools.partial(_grid_case, o, M) for o in (1931, 2006) for M in range(1, 17)},
    "every_m": {"M%d" % M: functools.partial(_every_m_case, M) for M in range(1, 17)},
    "ownership": {"17x9": functools.partial(_ownership_case, 17, 9), "13x11": functools.partial(_ownership_case, 13, 11)},
    "special": {"9x1": _special_case},
}


@functools.lru_cache(maxsize=None)
def case(family, name):
    c = FAMILIES[family][name]()
    H, W, K = c.lam.shape
    assert c.name == "%s/%s" % (family, name) and (W, H) in SIZES and K <= 48 and c.bins in ALL_BINS
    assert c.flux.shape == (H, W, K, 4) and c.flux.dtype == F and c.lam.dtype == F and all(sum(s) == K and min(s) > 0 for s in c.splits)
    assert (c.lam >= c.lambda_min).all() and (c.lam <= top(c.lambda_min, c.lambda_step)).all()
    _frozen(c.flux, c.lam)
    return c


def cases(family):
    return [case(family, name) for name in FAMILIES[family]]


def ids(family):
    return list(FAMILIES[family])
