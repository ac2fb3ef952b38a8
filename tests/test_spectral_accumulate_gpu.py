"""ssx_spectral_bin_kernel and ssx_spectral_moment_kernel on synthetic sample records (ssx_debug_spectral_accumulate: the kernels and launches of a render)
against the definition restated sequentially (tests/spectral_accumulate_cases.py, tests/spectral_ref.py): S and Q as uint64 and N, bit for bit, no tolerance; a
NaN against any NaN.  tests/test_spectral_accumulate_cpu.py shows that these inputs tell a subtly wrong kernel from the definition.  Then: the refusals, that
the call leaves the context's own state alone, and that it reproduces a real render's bins from that render's per-sample fluxes."""
import ctypes as C
import functools

import numpy as np
import pytest

import spectral_accumulate_cases as sc
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import Scene, SsxError

pytestmark = pytest.mark.gpu
TEX = "test-img.png"
W, H, SEED = 20, 12, 5


@functools.lru_cache(maxsize=None)
def pure():
    """one context for every pure call of this module (its scene is never rendered)"""
    return Renderer(Options(scene_name="cornell-srgb", res=(8, 8), seed=SEED, texture=TEX))


def run(c, split, layout=sc.WHOLE, moments=True):
    first, stride, skew = layout
    return pure().debug_spectral_accumulate(c.flux, c.lam, c.bins, c.lambda_min, c.lambda_step, n_k=split, tile_first=first, tile_stride=stride, tile_skew=skew,
                                            moments=moments)


def check(got, want, what):
    for name, g, w in zip("SNQ", got, want):
        bad = ~sc.same(g, w)
        assert not bad.any(), "%s: %d of %d words of %s differ, first at %s: got %r, want %r" % (
            what, bad.sum(), bad.size, name, tuple(np.argwhere(bad)[0]), g[tuple(np.argwhere(bad)[0])], w[tuple(np.argwhere(bad)[0])])


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["order", "edges", "grid", "every_m", "special"])
def test_kernels_equal_the_sequential_restatement(family):
    """every case of the family, in every launch split it lists"""
    for c in sc.cases(family):
        for split in c.splits:
            got = run(c, split)
            check(got, sc.reference(c), "%s as %d launches" % (c.name, len(split)))
            assert (got[1].sum(axis=2) == c.lam.shape[2]).all()                # every sample is counted once


def test_launch_splits_continue_bit_for_bit():
    """one record set as one launch, one launch per sample, unequal launches and launches of four: the same bits, and the restatement's"""
    c = sc.case("order", "17x9")
    assert {len(s) for s in c.splits} == {1, c.lam.shape[2], 12, c.lam.shape[2] // 4} and {1, 2, 3, 4, 5, 7} <= {n for s in c.splits for n in s}
    results = [run(c, split) for split in c.splits]
    for split, got in zip(c.splits, results):
        check(got, results[0], "%s: launches %r against one launch" % (c.name, split))
        check(got, sc.reference(c), "%s: launches %r" % (c.name, split))


def test_edge_indices_are_what_the_construction_says():
    """the formula-free table: the counts and sums by the indices written down from the construction"""
    for c in sc.cases("edges"):
        want = sc.accumulate(c.flux, c.expected_index, c.bins)
        check(run(c, c.splits[0]), want, c.name)


def test_without_moments_the_bins_are_the_same():
    c = sc.case("every_m", "M5")
    S, N, q = run(c, c.splits[1], moments=False)
    assert q is None
    check((S, N), sc.reference(c)[:2], c.name)


@pytest.mark.parametrize("size", sc.ids("ownership"))
def test_ownership(size):
    """foreign pixels +0.0 / 0 exactly, owned pixels the whole image's, the three shares of a stride of 3 add up to it"""
    c = sc.case("ownership", size)
    whole = run(c, c.splits[0])
    check(whole, sc.reference(c), c.name)
    shares = {layout: run(c, c.splits[0], layout) for layout in c.layouts}
    for layout, got in shares.items():
        own = sc.owned(c.lam.shape[1], c.lam.shape[0], layout)
        for a in got:
            assert not sc.bits(a)[~own].any(), "%s %r: a foreign pixel is not +0.0 / 0" % (c.name, layout)
        check(got, sc.reference_share(c, layout), "%s %r" % (c.name, layout))
        check(tuple(a[own] for a in got), tuple(a[own] for a in whole), "%s %r: owned pixels against the whole-image call" % (c.name, layout))
    for skew in sc.STRIDE3_SKEWS:
        with np.errstate(invalid="ignore"):
            added = tuple(sum(shares[(first, 3, skew)][n] for first in range(3)) for n in range(3))
        check(added, whole, "%s: the three shares of skew %d added" % (c.name, skew))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------------------------------

def refused(call, code, *words):
    with pytest.raises(SsxError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals():
    r = pure()
    c = sc.case("every_m", "M3")
    Hc, Wc, K = c.lam.shape
    good = dict(width=Wc, height=Hc, bins=c.bins, tile_first=0, tile_stride=1, tile_skew=0, lambda_min=float(c.lambda_min), lambda_step=float(c.lambda_step),
                n_k=[K], flux=c.flux, lam=c.lam, sums=True, counts=True)
    out_s, out_n, out_q = np.zeros((Hc, Wc, c.bins)), np.zeros((Hc, Wc, c.bins // 4), dtype=np.uint32), np.zeros((Hc, Wc, c.bins))

    def call(**over):
        a = dict(good, **over)
        n_k = None if a["n_k"] is None else np.asarray(a["n_k"], dtype=np.uint32)
        launches = a.get("launches", 0 if n_k is None else len(n_k))
        ptr = lambda x: None if x is None else x.ctypes.data
        r._check(r._lib.ssx_debug_spectral_accumulate(r._ctx, a["width"], a["height"], a["bins"], a["tile_first"], a["tile_stride"], a["tile_skew"], a["lambda_min"],
                                                      a["lambda_step"], launches, ptr(n_k), ptr(a["flux"]), ptr(a["lam"]), out_s.ctypes.data if a["sums"] else None,
                                                      out_n.ctypes.data if a["counts"] else None, out_q.ctypes.data))

    call()                                                                                                 # the arguments the refusals vary are good
    check((out_s, out_n, out_q), sc.reference(c), c.name)
    ARG = _capi.SSX_ERR_ARG
    for bins in (0, 2, 6, 68, 128):
        refused(lambda: call(bins=bins), ARG, "bins")
    refused(lambda: call(width=0), ARG, "width and height")
    refused(lambda: call(height=0), ARG, "width and height")
    refused(lambda: call(width=1 << 15, height=(1 << 13) + 1), ARG, "too large")
    refused(lambda: call(width=1 << 14, height=1 << 14, n_k=[K]), ARG, "too many records")
    refused(lambda: call(tile_stride=0), ARG, "tile_first < tile_stride")
    refused(lambda: call(tile_first=3, tile_stride=3), ARG, "tile_first < tile_stride")
    refused(lambda: call(n_k=[K], launches=0), ARG, "launches")
    refused(lambda: call(n_k=[K - 3, 0, 3]), ARG, "n_k[1] = 0")
    refused(lambda: call(lambda_step=0.0), ARG, "lambda_step")
    refused(lambda: call(lambda_step=float("nan")), ARG, "lambda_step")
    refused(lambda: call(lambda_min=float("inf")), ARG, "lambda_min")
    for null in ("n_k", "flux", "lam"):
        refused(lambda: call(**{null: None, "launches": 1}), ARG, "must not be NULL")
    for null in ("sums", "counts"):
        refused(lambda: call(**{null: False}), ARG, "must not be NULL")
    assert r._lib.ssx_debug_spectral_accumulate(None, *([0] * 6), 0.0, 0.0, 0, *([None] * 6)) == ARG
    # while a render runs: refused as every pure call is
    busy = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=SEED, texture=TEX, spp=1 << 20, spp_per_launch=16))
    busy.render_start()
    try:
        refused(lambda: busy.debug_spectral_accumulate(c.flux, c.lam, c.bins, c.lambda_min, c.lambda_step), _capi.SSX_ERR_STATE, "render in progress")
    finally:
        busy.render_stop(); busy.render_wait()
    busy.debug_spectral_accumulate(c.flux, c.lam, c.bins, c.lambda_min, c.lambda_step)                     # the stopped render's context takes the call


# ---- 3. the context's own state ----------------------------------------------------------------------------------------------------------------------------------

def renderer(scene, bins):
    r = Renderer(Options(scene_name=scene, res=(W, H), seed=SEED, texture=TEX))
    r.set_spectral_bins(bins)
    r.set_spectral_moments(True)
    return r


def start(r, spp):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp))))
    r.render_wait()


def cont(r, spp):
    r._check(r._lib.ssx_render_continue(r._ctx, spp))
    r.render_wait()


def state(r):
    """(sums, counts, q, var) of the context's render"""
    _, _, counts, sums = r.spectral_read(sums=True)
    _, var, q = r.spectral_variance(q=True)
    return sums, counts, q, var


@functools.lru_cache(maxsize=None)
def lambda_range(scene):
    s = Scene(scene, texture=TEX)
    d = s.desc.contents
    return np.float32(d.lambda_min), np.float32(d.lambda_step)


LAUNCHES = (2, 1, 2)


@functools.lru_cache(maxsize=None)
def rendered(scene, bins):
    """the render of part 4: a start and two continues of unequal length, moments on -> (sums, counts, q, var), read-only"""
    r = renderer(scene, bins)
    start(r, LAUNCHES[0])
    for n in LAUNCHES[1:]:
        cont(r, n)
    out = state(r)
    for a in out:
        a.setflags(write=False)
    return out


def test_the_call_only_reads_the_context():
    """a finished spectral render with moments reads the same before and after a call, and continues to the bits of the render that was never interrupted"""
    scene, bins = "cornell-srgb", 12
    r = renderer(scene, bins)
    start(r, LAUNCHES[0])
    before, image = state(r), r.xyza.copy()
    c = sc.case("every_m", "M7")                                            # another size, another bin count, other wavelengths than the context's
    check(r.debug_spectral_accumulate(c.flux, c.lam, c.bins, c.lambda_min, c.lambda_step, n_k=c.splits[1]), sc.reference(c), c.name)
    after = state(r)
    for b, a in zip(before, after):
        assert sc.same(a, b).all()
    assert r.done_spp() == LAUNCHES[0] and r.holds_spectral() and r.holds_moments()
    for n in LAUNCHES[1:]:
        cont(r, n)
    for got, want in zip(state(r), rendered(scene, bins)):
        assert sc.same(got, want).all()
    one = renderer(scene, bins)
    start(one, sum(LAUNCHES))
    for got, want in zip(state(r), state(one)):
        assert sc.same(got, want).all()
    assert np.array_equal(sc.bits(r.xyza), sc.bits(one.xyza)) and not np.array_equal(sc.bits(image), sc.bits(one.xyza))


# ---- 4. the call is the render's path ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", (12, 64))
@pytest.mark.parametrize("scene", ("cornell-srgb", "plane-srgb"))
def test_the_call_reproduces_a_render_from_its_samples(scene, bins):
    """a start and two continues; ssx_debug_sample_flux gives the same samples' flux and lambda_0; fed to the call with the same launch lengths they give
    ssx_spectral_read's sums and counts and ssx_spectral_variance's q, bit for bit"""
    sums, counts, q, _ = rendered(scene, bins)
    r = renderer(scene, bins)
    flux, lam = r.debug_sample_flux(spp=sum(LAUNCHES))
    lmin, lstep = lambda_range(scene)
    assert (lam >= lmin).all() and (lam <= sc.top(lmin, lstep)).all()
    assert counts.sum() == W * H * sum(LAUNCHES) and np.count_nonzero(sums) > W * H
    check(pure().debug_spectral_accumulate(flux, lam, bins, lmin, lstep, n_k=LAUNCHES), (sums, counts, q), "%s, %d bins" % (scene, bins))
    check(pure().debug_spectral_accumulate(flux, lam, bins, lmin, lstep), (sums, counts, q), "%s, %d bins, one launch" % (scene, bins))
