"""Depth of field on the GPU (include/ssx.h "Depth of field after the render"): ssx_defocus_images on the shared case list (tests/defocus_cases.py) against the
numpy restatement (tests/defocus_ref.py), ssx_spectral_develop_lens against its pieces, the state rules and every refusal.  "equals" is np.array_equal on the
uint32 views, bit for bit -- except that where BOTH sides hold a NaN the arithmetic made, any NaN equals any NaN, as in tests/test_optics_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import defocus_cases as dc
import defocus_ref as ref
import develop_ref
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError, _defocus_arg, _optics_arg, develop_weights, thin_lens_defocus

pytestmark = pytest.mark.gpu
W, H, SEED, SPP = 24, 16, 5, 8
TEX = "test-img.png"
F = np.float32
CASES = dc.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def renderer(res=(W, H), **opts):
    return Renderer(Options(scene_name="cornell-srgb", res=res, seed=SEED, texture=TEX, jit_pass1=False, **opts))


def start(r, spp=SPP, **over):
    over.setdefault("spp_per_launch", 4)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    r.render_wait()
    return r.xyza.copy()


@functools.lru_cache(maxsize=None)
def plain_context():
    return renderer()


def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    assert str(e.value).split(": ", 1)[1].strip(), "a refusal says why"
    for w in words:
        assert w in str(e.value), str(e.value)


def an_aperture(bins, R=5, K=12.0):
    """a focus per bin that moves with the bin; the misses (infinitely far) are out of focus in every bin"""
    return {"max_radius": R, "gain": K, "focus": np.linspace(0.4, 0.15, bins).astype(F)}


def a_lens(bins, R=3, seed=0):
    g = np.random.default_rng(100 + seed)
    radius = np.array([(0, R, min(1, R), min(2, R))[b % 4] for b in range(bins)], dtype=np.uint32)
    scale = np.array([(1.0, 0.98, 1.03)[b % 3] for b in range(bins)], dtype=F)
    return {"cx": 10.3, "cy": 9.75, "max_radius": R, "scale": scale, "radius": radius, "taps": g.uniform(0.05, 0.4, size=(bins, 2 * R + 1)).astype(F)}


# ---- 1. the pure function ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_defocus_images_equals_the_restatement(case):
    want = ref.defocus(case["q"], case["depth"], case["R"], case["K"], case["focus"])
    got = plain_context().defocus_images(case["q"], case["depth"], dc.params_of(case))
    assert got.shape == case["q"].shape and got.dtype == np.float32
    wrong = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not wrong.any(), "%d of %d differ, first at %r" % (wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]))
    if case["R"] == 0 or case["K"] == 0:
        assert np.array_equal(bits(got), bits(case["q"]))                                               # a copy: NaN payloads, -0 and denormals as they came


# ---- 2. from the context's state --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rendered(bins):
    """one render per bin count, two batches (the denoised source needs a variance); read-only for the tests that share it"""
    r = renderer()
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    start(r)
    q = develop_ref.raw_q(r.spectral_read(sums=True)[3], SPP)                                           # q rebuilt on the host from the exported sums
    depth = r.guides()["depth"]
    assert (q != 0).any() and (depth > 0).any()
    return r, q, depth


@pytest.mark.parametrize("bins", [16, 64])
@pytest.mark.parametrize("with_optics", [False, True])
def test_state_entry_equals_the_pure_chain(bins, with_optics):
    r, q, depth = rendered(bins)
    pure = plain_context()
    w = np.random.default_rng(bins).uniform(-2, 3, size=(3, bins)).astype(F)
    lens = a_lens(bins) if with_optics else None
    for ap in (an_aperture(bins, 5), an_aperture(bins, 12, 40.0), an_aperture(bins, 1, 3.0)):
        out, behind = r.develop(w, defocus=ap, optics=lens, return_bins=True)
        want = pure.defocus_images(q, depth, ap)
        assert same(want, ref.defocus(q, depth, ap["max_radius"], ap["gain"], ap["focus"]))
        assert not np.array_equal(bits(want), bits(q))
        if lens is not None:
            want = pure.optics_images(want, lens)
        assert np.array_equal(bits(behind), bits(want)), (bins, ap["max_radius"])
        assert np.array_equal(bits(out), bits(pure.develop_images(want, w)))
    # the denoised source goes the same way
    kw = dict(levels=3, sigma_l=4.0, sigma_a=0.037)
    filtered = r.denoise_spectral(**kw)
    ap = an_aperture(bins, 5)
    out, behind = r.develop(w, denoise=kw, defocus=ap, optics=lens, return_bins=True)
    want = pure.defocus_images(filtered, depth, ap)
    if lens is not None:
        want = pure.optics_images(want, lens)
    assert np.array_equal(bits(behind), bits(want)) and np.array_equal(bits(out), bits(pure.develop_images(want, w)))
    assert np.array_equal(bits(r.denoise_spectral(**kw)), bits(filtered))                               # the filter's buffers stayed as ssx_denoise_spectral needs them


def lens_call(r, w, out, dp=None, df=None, op=None, bins_out=None, ch=None, wp=True):
    r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None if dp is None else C.byref(dp), None if df is None else C.byref(df), None if op is None else C.byref(op),
                                              w.ctypes.data if wp else None, w.shape[0] if ch is None else ch, None if out is None else out.ctypes.data,
                                              None if bins_out is None else bins_out.ctypes.data))


@pytest.mark.parametrize("bins", [16, 64])
def test_null_stages_give_the_bits_of_the_entries_without_them(bins):
    r, q, depth = rendered(bins)
    w = np.random.default_rng(bins + 2).uniform(-2, 3, size=(4, bins)).astype(F)
    lens = a_lens(bins)
    op, keep = _optics_arg(lens, W, H)
    out, behind = np.zeros((H, W, 4), F), np.zeros_like(q)
    lens_call(r, w, out, op=op, bins_out=behind)                                                        # defocus NULL: ssx_spectral_develop_optics
    o2, b2 = r.develop(w, optics=lens, return_bins=True)
    assert np.array_equal(bits(out), bits(o2)) and np.array_equal(bits(behind), bits(b2))
    lens_call(r, w, out, bins_out=behind)                                                               # both NULL: ssx_spectral_develop
    assert np.array_equal(bits(out), bits(r.develop(w))) and np.array_equal(bits(behind), bits(q))
    dp = r._denoise_params(2, 1.0, 0.1)
    lens_call(r, w, out, dp=dp)
    assert np.array_equal(bits(out), bits(r.develop(w, denoise=dict(levels=2))))
    for ap in (an_aperture(bins, 0), an_aperture(bins, 5, 0.0)):                                        # R == 0 or K == 0: a copy, nothing launched
        o3, b3 = r.develop(w, defocus=ap, return_bins=True)
        assert np.array_equal(bits(o3), bits(r.develop(w))) and np.array_equal(bits(b3), bits(q))
    lmin_ap = thin_lens_defocus(r.scene, H, bins, 0.0, 3.0)                                             # the host's aperture of zero
    assert np.array_equal(bits(r.develop(w, defocus=lmin_ap)), bits(r.develop(w)))


def test_the_call_reads_only_and_the_render_continues():
    bins = 16
    one = renderer()
    one.set_noise_estimate(True)
    one.set_spectral_bins(bins)
    image = start(one, 12)
    spectral = one.spectral_read(sums=True)
    r = renderer()
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    first = start(r)
    before = r.spectral_read(sums=True)
    w = np.random.default_rng(3).uniform(-2, 3, size=(3, bins)).astype(F)
    r.develop(w, defocus=an_aperture(bins, 5)); r.develop(w, denoise={}, defocus=an_aperture(bins, 12, 40.0), optics=a_lens(bins))
    assert np.array_equal(bits(r.xyza), bits(first))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(r.spectral_read(sums=True)[1:], before[1:]))
    r.render_continue(4); r.render_wait()
    assert r.done_spp() == 12 and np.array_equal(bits(r.xyza), bits(image))
    again = r.spectral_read(sums=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], spectral[1:]))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_returns_its_code_and_names_its_field():
    bins = 8
    r = renderer()
    lib, ctx = r._lib, r._ctx
    g = np.random.default_rng(4)
    q, depth = g.uniform(0, 1, size=(H, W, bins)).astype(F), g.uniform(1, 9, size=(H, W)).astype(F)
    out = np.zeros_like(q)
    ap = an_aperture(bins, 3)

    def params(**over):
        d = dict(ap)
        struct_size = over.pop("struct_size", None)
        null = over.pop("null", False)
        d.update(over)
        p, keep = _defocus_arg(d)
        if struct_size is not None:
            p.struct_size = struct_size
        if null:
            p.focus = None
        return p, keep

    def pure(p=None, qp=q.ctypes.data, dp=depth.ctypes.data, op=out.ctypes.data, width=W, b=bins, defocus=True):
        p = p or params()
        r._check(lib.ssx_defocus_images(ctx, width, H, b, qp, dp, C.byref(p[0]) if defocus else None, op))

    pure()
    bad = lambda **over: (lambda: pure(params(**over)))
    refused(lambda: pure(qp=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: pure(dp=None), _capi.SSX_ERR_ARG, "NULL", "depth")
    refused(lambda: pure(op=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: pure(defocus=False), _capi.SSX_ERR_ARG, "NULL", "defocus")
    refused(bad(null=True), _capi.SSX_ERR_ARG, "NULL", "focus")
    refused(bad(struct_size=C.sizeof(_capi.SsxDefocusParams) - 8), _capi.SSX_ERR_ARG, "struct_size")
    refused(bad(struct_size=0), _capi.SSX_ERR_ARG, "struct_size")
    refused(bad(max_radius=13), _capi.SSX_ERR_ARG, "max_radius")
    for v in (-1.0, np.inf, np.nan):
        refused(bad(gain=v), _capi.SSX_ERR_ARG, "gain")
        f = ap["focus"].copy(); f[5] = v
        refused(bad(focus=f), _capi.SSX_ERR_ARG, "focus[5]")
    for b in (0, 6, 68, 128):
        refused(lambda: pure(b=b), _capi.SSX_ERR_ARG, "multiple of 4")
    refused(lambda: pure(width=0), _capi.SSX_ERR_ARG, "positive")
    refused(lambda: r._check(lib.ssx_defocus_images(ctx, 1 << 20, 1 << 20, bins, q.ctypes.data, depth.ctypes.data, C.byref(params()[0]), out.ctypes.data)), _capi.SSX_ERR_ARG, "too large")

    # the state entry: ssx_spectral_develop_optics's reasons first, then its own
    w = np.random.default_rng(5).uniform(-2, 3, size=(3, bins)).astype(F)
    img = np.zeros((H, W, 3), F)
    refused(lambda: r.develop(w, defocus=ap), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(bins)
    refused(lambda: r.develop(w, defocus=ap), _capi.SSX_ERR_STATE, "no spectral bins", "no render")
    start(r)
    r.develop(w, defocus=ap)
    refused(lambda: r.develop(w, denoise={}, defocus=ap), _capi.SSX_ERR_STATE, "noise estimate is off")
    refused(lambda: r.develop(w, denoise=dict(levels=7), defocus=ap), _capi.SSX_ERR_ARG, "levels")
    refused(lambda: lens_call(r, w, img, df=params()[0], wp=False), _capi.SSX_ERR_ARG, "weights")
    for ch in (0, 17):
        refused(lambda: lens_call(r, w, img, df=params()[0], ch=ch), _capi.SSX_ERR_ARG, "channels")
    refused(lambda: lens_call(r, w, img, df=params(null=True)[0]), _capi.SSX_ERR_ARG, "NULL", "focus")
    refused(lambda: lens_call(r, w, img, df=params(struct_size=4)[0]), _capi.SSX_ERR_ARG, "struct_size")
    refused(lambda: lens_call(r, w, img, df=params(max_radius=13)[0]), _capi.SSX_ERR_ARG, "max_radius")
    refused(lambda: lens_call(r, w, img, df=params(gain=-2.0)[0]), _capi.SSX_ERR_ARG, "gain")
    f = ap["focus"].copy(); f[7] = -0.5
    refused(lambda: lens_call(r, w, img, df=params(focus=f)[0]), _capi.SSX_ERR_ARG, "focus[7]")
    lens = a_lens(bins)
    s = lens["scale"].copy(); s[2] = -1.0
    refused(lambda: r.develop(w, defocus=ap, optics=dict(lens, scale=s)), _capi.SSX_ERR_ARG, "scale[2]")
    info, sums, s2 = r.export_sums()
    r.import_sums(info, sums, s2)
    refused(lambda: r.develop(w, defocus=ap), _capi.SSX_ERR_STATE, "no spectral bins", "ssx_sums_import")
    # while a render runs
    start(r)
    r._check(lib.ssx_render_continue(ctx, 1 << 16))
    try:
        refused(lambda: r.develop(w, defocus=ap), _capi.SSX_ERR_STATE, "render in progress")
        refused(pure, _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop(); r.render_wait()
    r.develop(w, defocus=ap)


def test_a_context_that_owns_every_other_tile_is_refused():
    bins = 8
    r = renderer(tile_first=1, tile_stride=2)
    r.set_spectral_bins(bins)
    start(r)
    w = develop_weights(bins, float(r.scene.desc.contents.lambda_min), float(r.scene.desc.contents.lambda_step))
    r.develop(w)                                                                                        # the plain develop takes such a context
    refused(lambda: r.develop(w, defocus=an_aperture(bins)), _capi.SSX_ERR_STATE, "tile_stride", "neighbours")
    refused(lambda: lens_call(r, w, np.zeros((H, W, w.shape[0]), F)), _capi.SSX_ERR_STATE, "tile_stride")   # whatever is NULL
