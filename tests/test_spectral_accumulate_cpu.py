"""ssx_debug_spectral_accumulate without a GPU: the interface is declared and bound, and -- the point of this file -- the inputs of
tests/spectral_accumulate_cases.py discriminate: on them a kernel that adds in another order, drops the clamp, rounds instead of truncating, divides through a
reciprocal or squares in binary32 changes at least one word of S, N or Q, so tests/test_spectral_accumulate_gpu.py would fail on it.  Also the measurement
behind the cases: how many words of a real render's bins a reversed order of addition changes (printed, not asserted: run with -s)."""
import os

import numpy as np
import pytest

import spectral_accumulate_cases as sc
import spectral_ref
from simple_spectral_amd import _capi
from simple_spectral_amd.renderer import spectral_bin_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "spectral_sample_flux.npz")


def test_header_and_binding_declare_the_call():
    text = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "int ssx_debug_spectral_accumulate(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, uint32_t tile_first, uint32_t tile_stride, uint32_t tile_skew," in text
    assert "#define SSX_ABI_VERSION 2\n" in text and _capi.SSX_ABI_VERSION == 2
    assert "ssx_debug_spectral_accumulate" in _capi.HIP_SYMBOLS


def test_the_launch_of_each_kernel_is_written_once():
    """the render and the debug call share one launch, dynamic-LDS size included: each kernel's name stands before exactly one launch"""
    csrc = os.path.join(ROOT, "simple_spectral_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip"))
    for kernel in ("ssx_spectral_bin_kernel", "ssx_spectral_moment_kernel"):
        assert text.count("hipLaunchKernelGGL(%s," % kernel) == 1, kernel


# ---- the restatement used to classify agrees with the reference the GPU is held to, on every case -------------------------------------------------------------

@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_the_two_restatements_agree(family):
    """tests/spectral_ref.py (array statements, what the GPU test compares with) and accumulate (pixel by pixel, what the wrong variants are variants of)"""
    for c in sc.cases(family):
        m = sc.bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins)
        assert np.array_equal(m, spectral_bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins)), c.name
        assert sc.differing(sc.accumulate(c.flux, m, c.bins), sc.reference(c)) == 0, c.name
        S, N, Q = sc.reference(c)
        assert (N.sum(axis=2) == c.lam.shape[2]).all(), c.name               # every sample is counted once


# ---- the inputs discriminate --------------------------------------------------------------------------------------------------------------------------------
# family -> the wrong restatements its cases must tell from the definition (every one of sc.WRONG is some family's)
MUST_DETECT = {
    "order": ("reversed-k", "interleaved4-k", "binary32-product", "round"),
    "edges": ("wrap", "discard", "round", "binary32-product"),
    "grid": ("wrap", "discard", "round", "reciprocal", "binary32-product"),
    "every_m": ("round", "reversed-k", "interleaved4-k", "binary32-product"),
    "ownership": ("round", "reversed-k", "interleaved4-k", "binary32-product"),
    "special": ("round", "binary32-product", "reversed-k", "interleaved4-k"),
}


def test_every_wrong_restatement_is_some_familys():
    assert set(MUST_DETECT) == set(sc.FAMILIES)
    assert set(w for ws in MUST_DETECT.values() for w in ws) == set(sc.WRONG)


@pytest.mark.parametrize("family", list(sc.FAMILIES))
def test_a_wrong_restatement_changes_a_word(family):
    changed = {w: 0 for w in sc.WRONG}
    for c in sc.cases(family):
        for w in sc.WRONG:
            changed[w] += sc.differing(sc.wrong_restatement(c, w), sc.reference(c))
    print("%s: words of S, N, Q changed by each wrong restatement: %s" % (family, changed))
    for w in MUST_DETECT[family]:
        assert changed[w] > 0, (family, w)


def test_the_order_case_depends_on_the_order_in_both_sums():
    """... in S and in Q separately, for the reversed and for the unrolled order, in the stream that falls into one bin and in the one spread over all"""
    c = sc.case("order", "17x9")
    S, N, Q = sc.reference(c)
    for w in ("reversed-k", "interleaved4-k"):
        S2, N2, Q2 = sc.wrong_restatement(c, w)
        assert np.array_equal(N, N2)
        dS, dQ = ~sc.same(S2, S), ~sc.same(Q2, Q)
        assert dS.sum() > 100 and dQ.sum() > 100, (w, dS.sum(), dQ.sum())
    # hero slot 0 of the pixel's own bin: a, 1, -a, 1, ... leaves exactly 1 in ascending order whatever the odd samples added before
    H, W, K = c.lam.shape
    M = c.bins // 4
    own = (np.arange(H * W) % M).reshape(H, W)
    m = sc.bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins)
    assert (m[:, :, 0::2] == own[:, :, None]).all()
    assert len(np.unique(m[:, :, 1::2])) == M                               # the other stream reaches every bin


@pytest.mark.parametrize("M", sc.EDGE_M)
def test_edge_indices_are_what_the_construction_says(M):
    """the formula-free table: expected indices from the construction, against the restated formula and renderer.spectral_bin_index; and the clamp is needed"""
    c = sc.case("edges", "M%d" % M)
    want = c.expected_index
    assert np.array_equal(sc.bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins), want)
    assert np.array_equal(spectral_bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins).astype(np.int64), want)
    assert sorted(np.unique(want)) == list(range(M))
    top = c.lam == sc.top(c.lambda_min, c.lambda_step)
    assert top.any(axis=2).all() and (want[top] == M - 1).all()                                # every pixel holds the upper end: t == 1, index M before the clamp
    assert (sc.bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins, "discard")[top] == -1).all()
    assert (c.lam == c.lambda_min).any(axis=2).all() and (want[c.lam == c.lambda_min] == 0).all()
    # (S, N, Q) by the construction's indices are the reference's: nothing in the expectation comes from the formula
    assert sc.differing(sc.accumulate(c.flux, want, c.bins), sc.reference(c)) == 0
    assert sc.differing(sc.wrong_restatement(c, "discard"), sc.reference(c)) > 0
    if M > 1:
        assert sc.differing(sc.wrong_restatement(c, "wrap"), sc.reference(c)) > 0


@pytest.mark.parametrize("observer", (1931, 2006))
def test_grid_cases_hold_every_boundary_point(observer):
    lmin, lstep = sc.grid(observer)
    for M in range(1, 17):
        c = sc.case("grid", "%d-M%d" % (observer, M))
        pts = sc.grid_points(observer, M)
        assert set(pts.tolist()) == set(np.unique(c.lam).tolist())
        assert lmin in pts and sc.top(lmin, lstep) in pts
        # the neighbours straddle every inner boundary: both indices m - 1 and m occur among the seven points around it
        m = sc.bin_index(pts, lmin, lstep, 4 * M)
        assert sorted(np.unique(m)) == list(range(M))


def test_special_values_stay_where_they_are():
    """what the special case's reference holds: the -0.0 alone sums to +0.0 (sign bit clear), inf then -inf is a NaN, a NaN stays in its bin and slot, FLT_MAX
    squared three times over is finite; every other bin, slot and every count is untouched by them"""
    c = sc.case("special", "9x1")
    S, N, Q = sc.reference(c)
    M = c.bins // 4
    plain_flux = c.flux.copy()
    for i, slot, m, samples in sc.SPECIALS.values():
        for k, _ in samples:
            plain_flux[0, i, k, slot] = 0.0
    S0 = sc.accumulate(plain_flux, sc.bin_index(c.lam, c.lambda_min, c.lambda_step, c.bins), c.bins)[0]
    touched = np.zeros(S.shape, dtype=bool)
    for i, slot, m, _ in sc.SPECIALS.values():
        touched[0, i, slot * M + m] = True
    assert np.array_equal(sc.bits(S)[~touched], sc.bits(S0)[~touched]) and np.isfinite(S[~touched]).all() and np.isfinite(Q[~touched]).all()
    at = lambda name: (0, sc.SPECIALS[name][0], sc.SPECIALS[name][1] * M + sc.SPECIALS[name][2])
    assert sc.bits(S)[at("minus-zero-alone")] == 0 and sc.bits(Q)[at("minus-zero-alone")] == 0 and N[0, 0, 0] == 1
    tiny = float(np.float32(1e-45))
    assert 0.0 < tiny < float(np.finfo(np.float32).tiny) and float(np.float32(1.1754942e-38)) < float(np.finfo(np.float32).tiny)   # denormals of binary32
    assert S[at("denormals")] == tiny and Q[at("denormals")] == 2.0          # ... + 1 swallows the three before it, - 1 leaves +0.0, and the last one stands
    only = [float(np.float32(v)) for _, v in sc.SPECIALS["denormals-only"][3]]
    assert S[at("denormals-only")] == (only[0] + only[1]) + only[2] != 0.0 and Q[at("denormals-only")] == (only[0] ** 2 + only[1] ** 2) + only[2] ** 2 > 0.0
    assert S[at("flt-max")] == 2.0 * float(sc.FLT_MAX) and Q[at("flt-max")] == 4.0 * float(sc.FLT_MAX) ** 2 and np.isfinite(Q[at("flt-max")])
    assert S[at("plus-inf")] == np.inf and Q[at("plus-inf")] == np.inf
    assert np.isnan(S[at("inf-then-minus-inf")]) and Q[at("inf-then-minus-inf")] == np.inf
    assert np.isnan(S[at("nan")]) and np.isnan(Q[at("nan")])
    assert S[at("minus-inf-first")] == -np.inf and Q[at("minus-inf-first")] == np.inf
    assert int(np.isnan(S).sum()) == 2 and int(np.isnan(Q).sum()) == 1
    # inf then -inf becomes a NaN at that k and not before: the launches up to the -inf leave +inf
    k_minus = [k for k, v in sc.SPECIALS["inf-then-minus-inf"][3] if v == -np.inf][0]
    before = sc.accumulate(c.flux[:, :, :k_minus], sc.bin_index(c.lam[:, :, :k_minus], c.lambda_min, c.lambda_step, c.bins), c.bins)[0]
    assert before[at("inf-then-minus-inf")] == np.inf


def test_ownership_layouts_split_the_image():
    for c in sc.cases("ownership"):
        H, W, _ = c.lam.shape
        for skew in sc.STRIDE3_SKEWS:
            shares = [sc.owned(W, H, (first, 3, skew)) for first in range(3)]
            assert (np.sum(shares, axis=0) == 1).all() and all(s.any() for s in shares)
        assert sc.owned(W, H, sc.WHOLE).all()
        assert set(sc.OWNERSHIP_LAYOUTS) <= set(c.layouts)


# ---- the measurement: does a render's data show the order of addition? ---------------------------------------------------------------------------------------

def test_measure_what_a_reversed_order_changes_in_a_render(capsys):
    """The per-sample hero fluxes of one small render (tests/golden/spectral_sample_flux.npz, written by tests/golden/make_spectral_flux_fixture.py: cornell-srgb,
    20 x 12, 32 samples per pixel), binned by the definition and with k reversed.  The outcome is printed, not asserted: it is the number behind the synthetic
    cases -- whether render data alone would notice a kernel that adds in another order."""
    z = np.load(FIXTURE)
    flux, lam, lmin, lstep = z["flux"], z["lambda_0"], np.float32(z["lambda_min"]), np.float32(z["lambda_step"])
    H, W, K = lam.shape
    assert flux.shape == (H, W, K, 4) and flux.dtype == np.float32 and lam.dtype == np.float32
    assert (lam >= lmin).all() and (lam <= sc.top(lmin, lstep)).all()
    lines = []
    for bins in (4, 16, 64):
        S, N, _ = spectral_ref.restate_bins(flux, lam, lmin, lstep, bins)
        Q = spectral_ref.restate_moments(flux, lam, lmin, lstep, bins)
        m = sc.bin_index(lam, lmin, lstep, bins)
        S2, N2, Q2 = sc.accumulate(flux, m, bins, order="reversed")
        assert np.array_equal(N, N2)
        filled = np.tile(N, (1, 1, 4)) >= 2                                  # words that hold at least two samples: only they have an order
        lines.append("bins %2d: reversed k changes %d of %d S words and %d of %d Q words that hold two samples or more"
                     % (bins, int((~sc.same(S2, S) & filled).sum()), int(filled.sum()), int((~sc.same(Q2, Q) & filled).sum()), int(filled.sum())))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
