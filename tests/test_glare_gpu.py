"""Glare on the GPU (include/ssx.h "Glare: per-bin convolution by FFT"): ssx_glare_images on the shared case list (tests/glare_cases.py) against the numpy
restatement (tests/glare_ref.py), ssx_spectral_develop_glare against its pieces, the state rules and every refusal.  "equals" is bit for bit on the uint32
views, or both zeros of either sign (an implementation may skip rows that PAD leaves zero, and a sum of zeros has no sign worth pinning); `off` bins are
held to their bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import glare_cases as gc
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError, _glare_arg, glare_aperture, glare_plan, glare_twiddles, lens_optics, thin_lens_defocus

pytestmark = pytest.mark.gpu
W, H, SEED, SPP = 24, 16, 5, 8
TEX = "test-img.png"
F = np.float32
CASES = gc.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def equal(got, want):
    return (bits(got) == bits(want)) | ((got == 0) & (want == 0))


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
    for w in words:
        assert w in str(e.value), str(e.value)


def a_glare(bins, R=5, seed=0, width=W, height=H):
    """a random, positive, asymmetric psf; `on` mixed"""
    g = np.random.default_rng(300 + seed)
    K = 2 * R + 1
    psf = g.uniform(0.1, 1.0, size=(bins, K, K))
    psf = (psf / psf.sum(axis=(1, 2), keepdims=True)).astype(F)
    px, py = glare_plan(width, height, R)
    return {"radius": R, "px": px, "py": py, "on": np.array([b % 4 != 2 for b in range(bins)], np.uint8), "psf": psf,
            "twiddle_x": glare_twiddles(px), "twiddle_y": glare_twiddles(py)}


# ---- 1. the pure function ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_glare_images_equals_the_restatement(k):
    case, want = CASES[k], gc.want(k)
    got = plain_context().glare_images(case["q"], gc.params_of(case))
    assert got.shape == case["q"].shape and got.dtype == np.float32
    wrong = ~equal(got, want)
    assert not wrong.any(), "%d of %d differ, first at %r" % (wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]))
    off = case["on"] == 0
    assert np.array_equal(bits(got[:, :, off]), bits(case["q"][:, :, off]))
    if case["on"].any():
        assert not np.array_equal(bits(got), bits(case["q"]))


def test_a_nan_takes_its_bin_and_no_other():
    k = [c["name"] for c in CASES].index("67x9-r12-b20")
    case, clean = CASES[k], gc.want(k)
    b = int(np.flatnonzero(case["on"])[2])
    q = case["q"].copy()
    q[4, 31, b] = np.nan
    got = plain_context().glare_images(q, gc.params_of(case))
    assert np.isnan(got[:, :, b]).all()
    others = np.arange(q.shape[2]) != b
    assert equal(got[:, :, others], clean[:, :, others]).all()


# ---- 2. from the context's state --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rendered(bins=8):
    """one render, two batches (the denoised source needs a variance); read-only for the tests that share it"""
    r = renderer()
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    image = start(r)
    return r, image


def lens_entry(r, denoise, defocus, optics, w):
    """ssx_spectral_develop_lens, either of defocus and optics absent: (out, bins_out)"""
    from simple_spectral_amd.renderer import _defocus_arg, _optics_arg
    B = w.shape[1]
    p = None if denoise is None else r._denoise_params(denoise.get("levels", 5), denoise.get("sigma_l", 1.0), denoise.get("sigma_a", 0.1))
    df, keep_f = _defocus_arg(defocus) if defocus is not None else (None, None)
    op, keep_o = _optics_arg(optics, W, H) if optics is not None else (None, None)
    out, behind = np.zeros((H, W, w.shape[0]), F), np.zeros((H, W, B), F)
    r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None if p is None else C.byref(p), None if df is None else C.byref(df), None if op is None else C.byref(op),
                                              w.ctypes.data, w.shape[0], out.ctypes.data, behind.ctypes.data))
    return out, behind


@pytest.mark.parametrize("denoise", [None, {"levels": 2}], ids=["raw", "denoised"])
def test_state_entry_equals_the_lens_entry_then_the_pure_entries(denoise):
    bins = 8
    r, _ = rendered(bins)
    pure = plain_context()
    w = np.random.default_rng(bins).uniform(-2, 3, size=(3, bins)).astype(F)
    d = r.scene.desc.contents
    lens = lens_optics(bins, d.lambda_min, d.lambda_step, lateral=0.05, sigma=0.8, max_radius=3)
    aperture = thin_lens_defocus(r.scene, H, bins, aperture=0.08, focus_distance=3.0, max_radius=4)
    glare = a_glare(bins)
    for defocus, optics in ((None, None), (aperture, lens)):
        lens_out, lens_bins = lens_entry(r, denoise, defocus, optics, w)
        out, behind = r.develop(w, denoise=denoise, defocus=defocus, optics=optics, glare=glare, return_bins=True)
        want = pure.glare_images(lens_bins, glare)
        assert np.array_equal(bits(behind), bits(want))
        assert np.array_equal(bits(out), bits(pure.develop_images(want, w)))
        assert not np.array_equal(bits(behind), bits(lens_bins))
        # glare == NULL: the bits of ssx_spectral_develop_lens
        from simple_spectral_amd.renderer import _defocus_arg, _optics_arg
        p = None if denoise is None else r._denoise_params(denoise.get("levels", 5), 1.0, 0.1)
        df = _defocus_arg(defocus)[0] if defocus is not None else None
        opk = _optics_arg(optics, W, H) if optics is not None else None
        o2, b2 = np.zeros_like(lens_out), np.zeros_like(lens_bins)
        r._check(r._lib.ssx_spectral_develop_glare(r._ctx, None if p is None else C.byref(p), None if df is None else C.byref(df), None if opk is None else C.byref(opk[0]),
                                                   None, w.ctypes.data, 3, o2.ctypes.data, b2.ctypes.data))
        assert np.array_equal(bits(o2), bits(lens_out)) and np.array_equal(bits(b2), bits(lens_bins))


def test_it_reads_only():
    """a develop with glare between two halves of a render: the continued render has the bits of a one-shot render"""
    bins = 8
    one = renderer()
    one.set_noise_estimate(True)
    one.set_spectral_bins(bins)
    image = start(one, 12)
    spectral = one.spectral_read(sums=True)
    r = renderer()
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    start(r)
    w = np.random.default_rng(1).uniform(-2, 3, size=(3, bins)).astype(F)
    r.develop(w, glare=a_glare(bins)); r.develop(w, denoise={}, glare=a_glare(bins, R=12, seed=1))
    r.render_continue(4); r.render_wait()
    assert r.done_spp() == 12 and np.array_equal(bits(r.xyza), bits(image))
    again = r.spectral_read(sums=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], spectral[1:]))


def test_develop_with_glare_and_a_sensor_equals_the_pure_entries_chained_by_hand():
    from simple_spectral_amd.renderer import sensor_bayer, sensor_exposure
    bins = 8
    r, _ = rendered(bins)
    g = np.random.default_rng(4)
    sensor = dict(sensor_bayer("RGGB"))
    sensor.update(sensor_exposure(full_well=20000.0, white_level=4.0, bits=12, black=64.0, read_e=2.0))
    sensor.update({"weights": g.uniform(0.0, 1.0, size=(3, bins)).astype(F), "ccm": (np.eye(3) + g.uniform(-0.1, 0.1, size=(3, 3))).astype(F), "noise": 1, "seed": 9})
    glare = a_glare(bins, R=3, seed=2)
    out, raw, dn = r.develop(None, glare=glare, sensor=sensor, return_raw=True)
    w = np.ones((1, bins), F)
    _, lens_bins = lens_entry(r, None, None, None, w)
    pure = plain_context()
    behind = pure.glare_images(lens_bins, glare)
    raw2, dn2 = pure.sensor_images(behind, sensor, return_dn=True)
    assert np.array_equal(bits(raw), bits(raw2)) and np.array_equal(bits(dn), bits(dn2))
    assert np.array_equal(bits(out), bits(pure.demosaic_images(raw2, sensor)))


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_field():
    pure = plain_context()
    bins = 8
    q = np.full((H, W, bins), 0.5, F)
    good = a_glare(bins)
    ARG, STATE = _capi.SSX_ERR_ARG, _capi.SSX_ERR_STATE

    def call(width=W, height=H, b=bins, qp=q, glare=good, out=True, **fields):
        gp, keep = _glare_arg(glare)
        for k, v in fields.items():
            setattr(gp, k, v)
        o = np.zeros_like(q)
        pure._check(pure._lib.ssx_glare_images(pure._ctx, width, height, b, None if qp is None else qp.ctypes.data, C.byref(gp) if glare is not None else None,
                                               o.ctypes.data if out else None))
    call()
    refused(lambda: call(b=6), ARG, "bins")
    refused(lambda: call(b=68), ARG, "bins")
    refused(lambda: call(qp=None), ARG, "q and out")
    refused(lambda: call(out=False), ARG, "q and out")
    refused(lambda: call(width=0), ARG, "width")
    refused(lambda: pure._check(pure._lib.ssx_glare_images(pure._ctx, W, H, bins, q.ctypes.data, None, q.ctypes.data)), ARG, "glare must not be NULL")
    refused(lambda: call(struct_size=8), ARG, "struct_size")
    refused(lambda: call(radius=257), ARG, "radius")
    refused(lambda: call(on=None), ARG, "on, psf")
    refused(lambda: call(psf=None), ARG, "on, psf")
    refused(lambda: call(twiddle_x=None), ARG, "twiddle_x")
    refused(lambda: call(twiddle_y=None), ARG, "twiddle_y")
    refused(lambda: call(px=good["px"] * 2), ARG, "ssx_glare_params.px")
    refused(lambda: call(py=good["py"] // 2), ARG, "ssx_glare_params.py")
    refused(lambda: call(width=4090, height=1, radius=5), ARG, "ssx_glare_params.px", "4096")
    refused(lambda: call(width=5000, height=1), ARG, "too large")
    bad = dict(good, psf=good["psf"].copy())
    bad["psf"][3, 2, 7] = np.inf
    refused(lambda: call(glare=bad), ARG, "psf[3][2][7]")
    bad["psf"][3, 2, 7] = 0.1
    bad["psf"][2, 0, 0] = np.nan                                      # bin 2 is off: its psf is not read
    call(glare=bad)
    bad = dict(good, twiddle_x=good["twiddle_x"].copy())
    bad["twiddle_x"][5, 1] = np.nan
    refused(lambda: call(glare=bad), ARG, "twiddle_x[5][1]")
    bad = dict(good, twiddle_y=good["twiddle_y"].copy())
    bad["twiddle_y"][3, 0] = -np.inf
    refused(lambda: call(glare=bad), ARG, "twiddle_y[3][0]")
    # the state entry: ssx_spectral_develop_lens's reasons and the struct's fields
    r, _ = rendered(8)
    w = np.ones((3, bins), F)
    refused(lambda: r.develop(w, glare=dict(good, px=good["px"] * 2, twiddle_x=glare_twiddles(good["px"] * 2))), ARG, "ssx_glare_params.px")
    refused(lambda: r.develop(w, glare=dict(good, radius=300)), ARG, "radius")
    def state(**fields):
        gp, keep = _glare_arg(good)
        for k, v in fields.items():
            setattr(gp, k, v)
        out = np.zeros((H, W, 3), F)
        r._check(r._lib.ssx_spectral_develop_glare(r._ctx, None, None, None, C.byref(gp), w.ctypes.data, 3, out.ctypes.data, None))
    state()
    refused(lambda: state(struct_size=8), ARG, "struct_size")
    refused(lambda: state(on=None), ARG, "on, psf")
    refused(lambda: state(psf=None), ARG, "on, psf")
    refused(lambda: state(twiddle_x=None), ARG, "twiddle_x")
    refused(lambda: state(twiddle_y=None), ARG, "twiddle_y")
    refused(lambda: state(py=good["py"] * 2), ARG, "ssx_glare_params.py")
    bad = dict(good, psf=good["psf"].copy())
    bad["psf"][0, 1, 1] = np.nan
    refused(lambda: r.develop(w, glare=bad), ARG, "psf[0][1][1]")
    refused(lambda: plain_context().develop(w, glare=good), STATE)
    part = renderer(tile_first=1, tile_stride=2)
    part.set_spectral_bins(bins)
    start(part)
    refused(lambda: part.develop(w, glare=good), STATE, "tile_stride", "ssx_glare_images")
    # while a render runs
    busy = renderer()
    busy.set_spectral_bins(bins)
    start(busy)
    busy._check(busy._lib.ssx_render_continue(busy._ctx, 1 << 16))
    try:
        refused(lambda: busy.develop(w, glare=good), STATE, "render in progress")
        refused(lambda: busy.glare_images(q, good), STATE, "render in progress")
    finally:
        busy.render_stop(); busy.render_wait()
    busy.develop(w, glare=good)
