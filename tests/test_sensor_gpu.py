"""Developing onto a sensor on the GPU (include/ssx.h "Developing onto a sensor"): ssx_sensor_images and ssx_demosaic_images on the shared case list
(tests/sensor_cases.py) against the numpy restatement (tests/sensor_ref.py), the identities of the definition, ssx_spectral_develop_sensor against its pieces,
the state rules and every refusal.  "equals" is np.array_equal on the uint32 views, bit for bit -- except that where BOTH sides hold a NaN the arithmetic
made, any NaN equals any NaN, as in tests/test_optics_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import develop_ref
import sensor_cases as sc
import sensor_ref as ref
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError, _sensor_arg, develop_weights, sensor_bayer, sensor_ccm, sensor_exposure

pytestmark = pytest.mark.gpu
W, H, SEED, SPP = 24, 16, 5, 8
TEX = "test-img.png"
F = np.float32
CASES = sc.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    wrong = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not wrong.any(), "%s: %d of %d differ, first at %r" % (what, wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]))


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


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement on a shared case, computed once: (raw, dn or None, out)"""
    c = next(c for c in CASES if c["name"] == name)
    raw, dn = ref.sensor(q=c["q"], **sc.sensor_of(c))
    return raw, dn, ref.demosaic(raw, c["taps"], c["ccm"])


def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    assert str(e.value).split(": ", 1)[1].strip(), "a refusal says why"
    for w in words:
        assert w in str(e.value), str(e.value)


# ---- 1. the pure functions --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sensor_images_equals_the_restatement(case):
    raw, dn, _ = expected(case["name"])
    r = plain_context()
    if dn is None:
        assert_same(r.sensor_images(case["q"], sc.sensor_of(case)), raw, "raw")
    else:
        got_raw, got_dn = r.sensor_images(case["q"], sc.sensor_of(case), return_dn=True)
        assert_same(got_raw, raw, "raw")
        assert_same(got_dn, dn, "dn")
        assert np.array_equal(got_dn, np.floor(got_dn)) and got_dn.min() >= 0 and got_dn.max() <= case["white"]
        assert_same(r.sensor_images(case["q"], sc.sensor_of(case)), raw, "raw without dn")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_demosaic_images_equals_the_restatement(case):
    raw, _, out = expected(case["name"])
    assert_same(plain_context().demosaic_images(raw, sc.sensor_of(case)), out, "out")


def test_the_identities_hold_on_the_device():
    r = plain_context()
    g = np.random.default_rng(2)
    for c in CASES:
        Hc, Wc, _ = c["q"].shape
        # noise off, no ADC, exposure 1: the develop at the photosite's filter
        s = dict(sc.sensor_of(c), noise=0, white=0.0, exposure=1.0, inv_exposure=1.0)
        img = r.develop_images(c["q"], c["weights"])
        assert same(r.sensor_images(c["q"], s), np.take_along_axis(img, ref.cfa_map(c["cfa"], Hc, Wc)[..., None], axis=2)[..., 0]), c["name"]
        # identity tables: raw in all three channels (finite raw; -0 comes out as +0: the header)
        raw = g.uniform(-3, 3, size=(Hc, Wc)).astype(F)
        raw.reshape(-1)[:2] = np.array([0x00000007, 0x80000001], dtype=np.uint32).view(F)
        out = r.demosaic_images(raw, dict(s, taps=ref.IDENTITY_TAPS, ccm=ref.IDENTITY_CCM))
        assert np.array_equal(bits(out), bits(np.repeat(raw[..., None], 3, axis=2))), c["name"]
    # a constant mosaic stays constant, a ramp stays a ramp inside, with the host's own tables
    for pattern in ref.PATTERNS:
        for method in ("mhc", "bilinear"):
            t = dict(sensor_bayer(pattern, method), ccm=ref.IDENTITY_CCM)
            j, i = np.mgrid[0:23, 0:37]
            ramp = (3 * i + 2 * j + 1).astype(F)
            assert np.array_equal(r.demosaic_images(ramp, t)[2:-2, 2:-2], np.repeat(ramp[2:-2, 2:-2, None], 3, axis=2)), (pattern, method)
            assert np.array_equal(bits(r.demosaic_images(np.full((5, 7), F(0.625)), t)), bits(np.full((5, 7, 3), F(0.625))))


def test_a_seed_or_a_frame_changes_the_noise_and_nothing_else():
    r = plain_context()
    c = max((c for c in CASES if c["noise"] and not c["white"]), key=lambda c: c["q"].shape[0] * c["q"].shape[1])
    s = sc.sensor_of(c)
    a = r.sensor_images(c["q"], s)
    assert np.array_equal(bits(a), bits(r.sensor_images(c["q"], s)))                                   # stateless: the same call, the same bits
    for other in (dict(s, seed=s["seed"] + 1), dict(s, frame=s["frame"] + 1)):
        b = r.sensor_images(c["q"], other)
        assert (a != b).mean() > 0.99
    assert same(r.sensor_images(c["q"], dict(s, seed=s["seed"] + 1)), ref.sensor(q=c["q"], **dict(s, seed=s["seed"] + 1))[0])


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


def a_sensor(r, bins, pattern="GRBG", method="mhc", **over):
    """the host's own policy end to end: three Gaussian curves, their weights, the matrix to linear BT.709, a 12-bit ADC, noise"""
    d = r.scene.desc.contents
    lmin, lstep = float(d.lambda_min), float(d.lambda_step)
    lam = np.arange(380.0, 731.0, 5.0)
    curves = [(np.exp(-0.5 * ((lam - peak) / 35.0) ** 2).astype(F), 380.0, 730.0) for peak in (600.0, 540.0, 460.0)]
    cam = develop_weights(bins, lmin, lstep, responses=curves)
    s = dict(sensor_bayer(pattern, method), weights=cam, ccm=sensor_ccm(cam, develop_weights(bins, lmin, lstep, space="lrgb")), noise=1, seed=9, frame=2)
    s.update(sensor_exposure(full_well=15000.0, white_level=float(over.pop("white_level", 40.0)), bits=12, black=64.0, read_e=3.0))
    s.update(over)
    return s


def an_aperture(bins, R=5, K=12.0):
    return {"max_radius": R, "gain": K, "focus": np.linspace(0.4, 0.15, bins).astype(F)}


def a_lens(bins, R=3, seed=0):
    g = np.random.default_rng(100 + seed)
    radius = np.array([(0, R, min(1, R), min(2, R))[b % 4] for b in range(bins)], dtype=np.uint32)
    scale = np.array([(1.0, 0.98, 1.03)[b % 3] for b in range(bins)], dtype=F)
    return {"cx": 10.3, "cy": 9.75, "max_radius": R, "scale": scale, "radius": radius, "taps": g.uniform(0.05, 0.4, size=(bins, 2 * R + 1)).astype(F)}


@pytest.mark.parametrize("bins", [16, 64])
@pytest.mark.parametrize("stages", ["none", "defocus", "optics", "both"])
def test_state_entry_equals_the_pure_chain(bins, stages):
    r, q, depth = rendered(bins)
    pure = plain_context()
    ap = an_aperture(bins) if stages in ("defocus", "both") else None
    lens = a_lens(bins) if stages in ("optics", "both") else None
    kw = dict(levels=3, sigma_l=4.0, sigma_a=0.037)
    for source, denoise in ((q, None), (r.denoise_spectral(**kw), kw)):
        want = source
        if ap is not None:
            want = pure.defocus_images(want, depth, ap)
        if lens is not None:
            want = pure.optics_images(want, lens)
        white_level = float(np.nanmax(pure.develop_images(want, a_sensor(r, bins)["weights"]))) * 0.8    # the image fills the ADC's range
        for s in (a_sensor(r, bins, white_level=white_level), a_sensor(r, bins, "BGGR", "bilinear", white_level=white_level, noise=0, white=0.0)):
            adc = s["white"] > 0
            out, raw, dn = r.develop(None, denoise=denoise, defocus=ap, optics=lens, sensor=s, return_raw=True)
            if adc:
                want_raw, want_dn = pure.sensor_images(want, s, return_dn=True)
                assert np.array_equal(bits(dn), bits(want_dn)) and dn.min() >= 0 and dn.max() <= s["white"] and len(np.unique(dn)) > 16
            else:
                want_raw = pure.sensor_images(want, s)
                assert dn is None
            assert same(want_raw, ref.sensor(q=want, **s)[0])
            assert np.array_equal(bits(raw), bits(want_raw)), (bins, stages, adc)
            assert np.array_equal(bits(out), bits(pure.demosaic_images(want_raw, s)))
            assert np.array_equal(bits(r.develop(None, denoise=denoise, defocus=ap, optics=lens, sensor=s)), bits(out))   # raw_out and dn_out NULL
    assert np.array_equal(bits(r.denoise_spectral(**kw)), bits(source))                                # the filter's buffers stayed as ssx_denoise_spectral needs them


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
    s = a_sensor(r, bins)
    r.develop(None, sensor=s); r.develop(None, denoise={}, defocus=an_aperture(bins, 12, 40.0), optics=a_lens(bins), sensor=s, return_raw=True)
    assert np.array_equal(bits(r.xyza), bits(first))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(r.spectral_read(sums=True)[1:], before[1:]))
    r.render_continue(4); r.render_wait()
    assert r.done_spp() == 12 and np.array_equal(bits(r.xyza), bits(image))
    again = r.spectral_read(sums=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], spectral[1:]))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------------------

def sensor_call(r, sp, out=None, raw=None, dn=None, dp=None, sensor=True):
    ptr = lambda a: None if a is None else a.ctypes.data
    r._check(r._lib.ssx_spectral_develop_sensor(r._ctx, None if dp is None else C.byref(dp), None, None, C.byref(sp) if sensor else None, ptr(out), ptr(raw), ptr(dn)))


def test_every_refusal_returns_its_code_and_names_its_field():
    bins = 8
    r = renderer()
    lib, ctx = r._lib, r._ctx
    g = np.random.default_rng(4)
    q = g.uniform(0, 1, size=(H, W, bins)).astype(F)
    raw, dn, out = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
    base = dict(sensor_bayer("RGGB"), weights=g.uniform(0, 1, size=(3, bins)).astype(F), ccm=np.eye(3, dtype=F), noise=1, **sensor_exposure(20000.0, 2.0, bits=10, black=16.0, read_e=2.0))

    def params(**over):
        d = dict(base)
        struct_size = over.pop("struct_size", None)
        null = over.pop("null", ())
        d.update(over)
        p, keep = _sensor_arg(d)
        if struct_size is not None:
            p.struct_size = struct_size
        for n in null:
            setattr(p, n, None)
        return p, keep

    def sense(p=None, qp=q.ctypes.data, rp=raw.ctypes.data, dp=dn.ctypes.data, width=W, height=H, b=bins, sensor=True):
        p = p or params()
        r._check(lib.ssx_sensor_images(ctx, width, height, b, qp, C.byref(p[0]) if sensor else None, rp, dp))

    def mosaic(p=None, rp=raw.ctypes.data, op=out.ctypes.data, width=W, height=H, sensor=True):
        p = p or params()
        r._check(lib.ssx_demosaic_images(ctx, width, height, rp, C.byref(p[0]) if sensor else None, op))

    sense(); mosaic()
    sense(params(null=("taps", "ccm"))); mosaic(params(null=("weights",)))                              # each pure entry reads only its own tables
    for call in (sense, mosaic):
        bad = lambda **over: (lambda: call(params(**over)))
        refused(lambda: call(rp=None), _capi.SSX_ERR_ARG, "NULL")
        refused(lambda: call(sensor=False), _capi.SSX_ERR_ARG, "NULL", "sensor")
        refused(bad(struct_size=C.sizeof(_capi.SsxSensorParams) - 8), _capi.SSX_ERR_ARG, "struct_size")
        refused(bad(struct_size=0), _capi.SSX_ERR_ARG, "struct_size")
        refused(bad(cfa=[0, 1, 3, 2]), _capi.SSX_ERR_ARG, "cfa[2]")
        for name in ("exposure", "inv_exposure", "read_var", "dn_per_e", "e_per_dn", "black", "white"):
            for v in (np.inf, np.nan):
                refused(bad(**{name: v}), _capi.SSX_ERR_ARG, "ssx_sensor_params." + name)
        for name in ("exposure", "read_var", "white"):
            refused(bad(**{name: -1.0}), _capi.SSX_ERR_ARG, "ssx_sensor_params." + name, "negative")
        refused(bad(black=2000.0), _capi.SSX_ERR_ARG, "black", "white")
        call(params(black=2000.0, white=0.0), **(dict(dp=None) if call is sense else {}))                # without an ADC the black level is not looked at
        refused(lambda: call(width=2), _capi.SSX_ERR_ARG, "3 x 3")
        refused(lambda: call(height=2), _capi.SSX_ERR_ARG, "3 x 3")
        refused(lambda: call(width=0), _capi.SSX_ERR_ARG, "3 x 3")
        refused(lambda: call(width=1 << 20, height=1 << 20), _capi.SSX_ERR_ARG, "too large")
    refused(lambda: sense(qp=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: mosaic(op=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: sense(params(null=("weights",))), _capi.SSX_ERR_ARG, "NULL", "weights")
    refused(lambda: mosaic(params(null=("taps",))), _capi.SSX_ERR_ARG, "NULL", "taps")
    refused(lambda: mosaic(params(null=("ccm",))), _capi.SSX_ERR_ARG, "NULL", "ccm")
    refused(lambda: sense(params(white=0.0)), _capi.SSX_ERR_ARG, "dn", "ADC")
    sense(params(white=0.0), dp=None)
    for v in (np.inf, -np.inf, np.nan):
        t = base["taps"].copy(); t[2, 1, 7] = v
        refused(lambda: mosaic(params(taps=t)), _capi.SSX_ERR_ARG, "taps[2][1][7]")
        m = base["ccm"].copy(); m[1, 2] = v
        refused(lambda: mosaic(params(ccm=m)), _capi.SSX_ERR_ARG, "ccm[1][2]")
    for b in (0, 6, 68, 128):
        refused(lambda: sense(b=b), _capi.SSX_ERR_ARG, "multiple of 4")

    # the state entry: ssx_spectral_develop_lens's reasons, and its own
    s = dict(base)
    refused(lambda: r.develop(None, sensor=s), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(bins)
    refused(lambda: r.develop(None, sensor=s), _capi.SSX_ERR_STATE, "no spectral bins", "no render")
    start(r)
    r.develop(None, sensor=s)
    refused(lambda: r.develop(None, denoise={}, sensor=s), _capi.SSX_ERR_STATE, "noise estimate is off")
    refused(lambda: r.develop(None, denoise=dict(levels=7), sensor=s), _capi.SSX_ERR_ARG, "levels")
    refused(lambda: sensor_call(r, params()[0], out, sensor=False), _capi.SSX_ERR_ARG, "NULL", "sensor")
    for n in ("weights", "taps", "ccm"):
        refused(lambda: sensor_call(r, params(null=(n,))[0], out), _capi.SSX_ERR_ARG, "NULL", n)
    refused(lambda: sensor_call(r, params(struct_size=4)[0], out), _capi.SSX_ERR_ARG, "struct_size")
    refused(lambda: sensor_call(r, params(cfa=[9, 0, 1, 2])[0], out), _capi.SSX_ERR_ARG, "cfa[0]")
    refused(lambda: sensor_call(r, params(read_var=-1.0)[0], out), _capi.SSX_ERR_ARG, "read_var")
    refused(lambda: sensor_call(r, params(white=0.0)[0], out, dn=dn), _capi.SSX_ERR_ARG, "dn", "ADC")
    refused(lambda: r.develop(None, sensor=s, defocus=dict(an_aperture(bins), gain=-2.0)), _capi.SSX_ERR_ARG, "gain")
    lens = a_lens(bins)
    sc_ = lens["scale"].copy(); sc_[2] = -1.0
    refused(lambda: r.develop(None, sensor=s, optics=dict(lens, scale=sc_)), _capi.SSX_ERR_ARG, "scale[2]")
    sensor_call(r, params()[0])                                                                          # every output NULL: the kernels run, nothing is copied
    info, sums, s2 = r.export_sums()
    r.import_sums(info, sums, s2)
    refused(lambda: r.develop(None, sensor=s), _capi.SSX_ERR_STATE, "no spectral bins", "ssx_sums_import")
    # while a render runs
    start(r)
    r._check(lib.ssx_render_continue(ctx, 1 << 16))
    try:
        refused(lambda: r.develop(None, sensor=s), _capi.SSX_ERR_STATE, "render in progress")
        refused(sense, _capi.SSX_ERR_STATE, "render in progress")
        refused(mosaic, _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop(); r.render_wait()
    r.develop(None, sensor=s)


def test_a_context_that_owns_every_other_tile_is_refused():
    bins = 8
    r = renderer(tile_first=1, tile_stride=2)
    r.set_spectral_bins(bins)
    start(r)
    d = r.scene.desc.contents
    r.develop(develop_weights(bins, float(d.lambda_min), float(d.lambda_step)))                          # the plain develop takes such a context
    refused(lambda: r.develop(None, sensor=a_sensor(r, bins)), _capi.SSX_ERR_STATE, "tile_stride", "neighbours")
