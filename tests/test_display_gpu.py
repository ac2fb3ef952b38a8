"""Finishing a development for a display on the GPU (include/ssx.h "Finishing a development for a display"): ssx_meter_images, ssx_local_images and
ssx_tone_images on the shared case list (tests/display_cases.py) against the numpy restatement (tests/display_ref.py) -- METER as integers, LOCAL and TONE to the
bit (or a zero of the other sign; NaN exactly where the restatement has NaN) --, every refusal naming its field, Renderer.finish against the three pure calls chained
by hand, and Renderer.develop(display=None) against a call without the keyword."""
import ctypes as C
import functools

import numpy as np
import pytest

import display_cases as dc
import display_ref as ref
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError, develop_weights, display_luma, display_matrix, meter_derive, tone_curve

pytestmark = pytest.mark.gpu
F = np.float32
METER, LOCAL, TONE = dc.meter_cases(), dc.local_cases(), dc.tone_cases()


@functools.lru_cache(maxsize=None)
def context():
    return Renderer(Options(scene_name="cornell-srgb", res=(32, 32), seed=5, texture="test-img.png", jit_pass1=False))


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN in other places" % what
    wrong = ~((ref.bits(got) == ref.bits(want)) | ((got == 0) & (want == 0)) | np.isnan(want))
    assert not wrong.any(), "%s: %d of %d differ, first at %r" % (what, wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]))


@pytest.mark.parametrize("case", METER, ids=[c["name"] for c in METER])
def test_meter_counts_what_the_restatement_counts(case):
    hist, special = context().meter_images(case["img"], case["luma"], case["mask"])
    want_hist, want_special = ref.meter(case["img"], case["luma"], case["mask"])
    assert hist.dtype == np.uint32 and np.array_equal(special, want_special), (special.tolist(), want_special.tolist())
    assert np.array_equal(hist, want_hist), np.argwhere(hist != want_hist)[:4].tolist()
    assert not hist[:, 4080:].any()


@pytest.mark.parametrize("case", LOCAL, ids=[c["name"] for c in LOCAL])
def test_local_has_the_bits_of_the_restatement(case):
    gain, base = context().local_images(case["img"], case["luma"], return_base=True, **dc.local_params(case))
    want_gain, want_base = ref.local(case["img"], case["luma"], **dc.local_params(case))
    assert_same(base, want_base, "base")
    assert_same(gain, want_gain, "gain")
    assert_same(context().local_images(case["img"], case["luma"], **dc.local_params(case)), want_gain, "gain without base")


@pytest.mark.parametrize("case", TONE, ids=[c["name"] for c in TONE])
def test_tone_has_the_bits_of_the_restatement(case):
    got = context().tone_images(case["img"], case["curve"], **dc.tone_params(case))
    assert_same(got, ref.tone(case["img"], case["curve"], **dc.tone_params(case)), "out")


def refused(call, code, *words):
    with pytest.raises(SsxError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_entries_refuse_what_the_header_says_naming_the_field():
    r = context()
    img = np.full((4, 5, 3), 0.5, dtype=F)
    nan, inf = float("nan"), float("inf")
    # METER
    refused(lambda: r.meter_images(img, (0.2, nan, 0.1)), _capi.SSX_ERR_ARG, "luma[1]")
    refused(lambda: r.meter_images(np.zeros((0, 5, 3), dtype=F), dc.LUMA), _capi.SSX_ERR_ARG, "width and height")
    hist, special = np.zeros((4, 4096), np.uint32), np.zeros((4, 4), np.uint32)
    assert r._lib.ssx_meter_images(r._ctx, 5, 4, None, dc.LUMA.ctypes.data, None, hist.ctypes.data, special.ctypes.data) == _capi.SSX_ERR_ARG
    assert r._lib.ssx_meter_images(r._ctx, 5, 4, img.ctypes.data, None, None, hist.ctypes.data, special.ctypes.data) == _capi.SSX_ERR_ARG
    assert b"luma" in r._lib.ssx_last_error(r._ctx)
    # LOCAL
    ok = dict(radius=2, compress=0.5)
    r.local_images(img, dc.LUMA, **ok)
    for field, kw in (("radius", dict(radius=0)), ("radius", dict(radius=33)), ("exposure", dict(exposure=inf)), ("pivot", dict(pivot=nan)), ("compress", dict(compress=inf)),
                      ("boost", dict(boost=nan)), ("y_lo", dict(y_lo=0.0)), ("y_lo", dict(y_lo=1e-40)), ("y_hi", dict(y_hi=inf)), ("y_lo", dict(y_lo=2.0, y_hi=1.0)),
                      ("eps", dict(eps=0.0)), ("eps", dict(eps=nan))):
        refused(lambda: r.local_images(img, dc.LUMA, **dict(ok, **kw)), _capi.SSX_ERR_ARG, "ssx_local_params." + field)
    refused(lambda: r.local_images(img, (inf, 0, 0), **ok), _capi.SSX_ERR_ARG, "luma[0]")
    p = _capi.SsxLocalParams()
    gain = np.zeros((4, 5), dtype=F)
    assert r._lib.ssx_local_images(r._ctx, 5, 4, img.ctypes.data, dc.LUMA.ctypes.data, C.byref(p), gain.ctypes.data, None) == _capi.SSX_ERR_ARG
    assert b"struct_size" in r._lib.ssx_last_error(r._ctx)
    assert r._lib.ssx_local_images(r._ctx, 5, 4, img.ctypes.data, dc.LUMA.ctypes.data, None, gain.ctypes.data, None) == _capi.SSX_ERR_ARG
    # TONE
    lo, hi, shift = 2.0 ** -4, 4.0, 20
    curve = np.linspace(0, 1, ref.curve_len(lo, hi, shift)).astype(F)
    ok = dict(lo=lo, hi=hi, shift=shift)
    r.tone_images(img, curve, **ok)
    bad = curve.copy(); bad[3] = nan
    for field, call in (("shift", lambda: r.tone_images(img, curve, lo=lo, hi=hi, shift=11)), ("shift", lambda: r.tone_images(img, curve, lo=lo, hi=hi, shift=24)),
                        ("lo", lambda: r.tone_images(img, curve, lo=0.0, hi=hi, shift=shift)), ("hi", lambda: r.tone_images(img, curve, lo=lo, hi=inf, shift=shift)),
                        ("lo", lambda: r.tone_images(img, curve, lo=8.0, hi=hi, shift=shift)), ("curve_len", lambda: r.tone_images(img, curve[:-1], **ok)),
                        ("curve_len", lambda: r.tone_images(img, np.zeros(20000, dtype=F), lo=2.0 ** -20, hi=2.0 ** 20, shift=12)),
                        ("curve[3]", lambda: r.tone_images(img, bad, **ok)), ("gains[2]", lambda: r.tone_images(img, curve, gains=(1, 1, nan), **ok)),
                        ("matrix[1][2]", lambda: r.tone_images(img, curve, matrix=[[1, 0, 0], [0, 1, inf], [0, 0, 1]], **ok))):
        refused(call, _capi.SSX_ERR_ARG, field)
    refused(lambda: r.tone_images(np.zeros((0, 0, 3), dtype=F), curve, **ok), _capi.SSX_ERR_ARG, "width and height")


def test_a_running_render_refuses_the_three_entries():
    r = Renderer(Options(scene_name="cornell-srgb", res=(256, 256), seed=5, texture="test-img.png", jit_pass1=False))
    img = np.full((4, 5, 3), 0.5, dtype=F)
    curve = np.linspace(0, 1, ref.curve_len(0.25, 4.0, 20)).astype(F)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=1 << 16, spp_per_launch=4))))         # 4 G samples: more than a second of rendering; stopped below
    try:
        assert r.is_rendering()
        refused(lambda: r.meter_images(img, dc.LUMA), _capi.SSX_ERR_STATE, "render in progress")
        refused(lambda: r.local_images(img, dc.LUMA, 2, 0.5), _capi.SSX_ERR_STATE, "render in progress")
        refused(lambda: r.tone_images(img, curve, lo=0.25, hi=4.0, shift=20), _capi.SSX_ERR_STATE, "render in progress")
        assert r.is_rendering()                                                                      # ... and was running all the while
    finally:
        r.render_stop()
        r.render_wait()
    r.meter_images(img, dc.LUMA)


@functools.lru_cache(maxsize=None)
def rendered():
    """a 32 x 32, 4-spp, 16-bin Cornell render and its XYZ development"""
    r = Renderer(Options(scene_name="cornell-srgb", res=(32, 32), seed=5, texture="test-img.png", jit_pass1=False))
    r.set_spectral_bins(16)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=4, spp_per_launch=4))))
    r.render_wait()
    return r


def weights_of(r):
    info = r.spectral_read()[0]
    return develop_weights(16, info.lambda_min, info.bin_width * 4)


def test_finish_is_the_three_entries_chained_by_hand():
    r = rendered()
    image = r.develop(weights_of(r))
    for display in (dict(curve="reinhard", local=dict(radius=4, compress=0.5)), dict(curve="filmic", wb="grey"), dict(curve="clip", key=0.36, white_percentile=0.9, wb="white-patch",
                                                                                                                 local=dict(radius=2, compress=0.7, boost=1.5, eps=0.05))):
        got, (hist, special) = r.finish(image, display, return_meter=True)
        luma = display_luma(display_matrix())
        h2, s2 = r.meter_images(image, luma)
        assert np.array_equal(hist, h2) and np.array_equal(special, s2)
        m = meter_derive(h2, s2, key=display.get("key", 0.18), white_percentile=display.get("white_percentile", 0.99))
        wb = {"none": np.ones(3, dtype=F), "grey": m["grey"], "white-patch": m["patch"]}[display.get("wb", "none")]
        loc = display.get("local")
        local = None if loc is None else r.local_images(image, luma, loc["radius"], loc["compress"], boost=loc.get("boost", 1.0), eps=loc.get("eps", 0.25),
                                                        exposure=m["exposure"], pivot=m["pivot"])
        curve = tone_curve(display["curve"], 2.0 ** -12, 16.0, 19, white=float(m["white_exposed"]))
        want = r.tone_images(image, curve, lo=2.0 ** -12, hi=16.0, shift=19, gains=F(m["exposure"]) * wb, matrix=display_matrix(), local=local)
        assert np.array_equal(ref.bits(got), ref.bits(want)), display
        assert got.min() >= 0.0 and got.max() <= 1.0 and got.std() > 0.01                      # display-encoded, and a picture
        # and the device's stages are the restatement's on this image too
        assert_same(want, ref.tone(image, curve, 2.0 ** -12, 16.0, 19, gains=F(m["exposure"]) * wb, matrix=display_matrix(), local=local), "tone of the render")


def test_develop_without_a_display_gives_the_bits_it_gave():
    """against the entry point itself, not against another trip through the wrapper"""
    r = rendered()
    w = weights_of(r)
    raw = np.zeros((32, 32, 3), dtype=F)
    r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, 3, raw.ctypes.data))
    assert raw.any()
    for got in (r.develop(w), r.develop(w, display=None), r._develop(w)):
        assert got.dtype == np.float32 and np.array_equal(ref.bits(got), ref.bits(raw))
    assert np.array_equal(ref.bits(r.develop(w, display={})), ref.bits(r.finish(raw, {})))
