"""The lens on the GPU (include/ssx.h "Developing through a lens"): ssx_optics_images on the shared case list (tests/optics_cases.py) against the numpy
restatement (tests/optics_ref.py), ssx_spectral_develop_optics against its pieces, the state rules and every refusal.  "equals" is np.array_equal on the
uint32 views, bit for bit -- except that where BOTH sides hold a NaN the arithmetic made (inf - inf, 0 * inf, a NaN operand), any NaN equals any NaN: IEEE 754
leaves the sign and payload of such a NaN to the implementation, and the host's and the device's differ; as in tests/test_develop_gpu.py.  A NaN that is only
COPIED (a bin with s_b == 1 and r_b == 0) is held to its bits."""
import ctypes as C
import functools

import numpy as np
import pytest

import develop_ref
import optics_cases as oc
import optics_ref as ref
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError, _optics_arg, develop_weights, lens_optics

pytestmark = pytest.mark.gpu
W, H, SEED, SPP = 24, 16, 5, 8
TEX = "test-img.png"
F = np.float32
CASES = oc.cases()


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


def a_lens(bins, R=3, seed=0):
    """mixed scales and radii, random taps, a centre off the middle"""
    g = np.random.default_rng(100 + seed)
    radius = np.array([(0, R, min(1, R), min(2, R))[b % 4] for b in range(bins)], dtype=np.uint32)
    scale = np.array([oc.SCALES[b % 5] for b in range(bins)], dtype=F)
    return {"cx": 10.3, "cy": 9.75, "max_radius": R, "scale": scale, "radius": radius, "taps": g.uniform(0.05, 0.4, size=(bins, 2 * R + 1)).astype(F)}


def identity_lens(bins, R=2):
    return {"cx": None, "cy": None, "max_radius": R, "scale": np.ones(bins, F), "radius": np.zeros(bins, np.uint32), "taps": np.full((bins, 2 * R + 1), 0.5, F)}


# ---- 1. the pure function ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_optics_images_equals_the_restatement(case):
    want = ref.optics(case["q"], case["cx"], case["cy"], case["R"], case["scale"], case["radius"], case["taps"])
    got = plain_context().optics_images(case["q"], oc.params_of(case))
    assert got.shape == case["q"].shape and got.dtype == np.float32
    wrong = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not wrong.any(), "%d of %d differ, first at %r" % (wrong.sum(), wrong.size, tuple(np.argwhere(wrong)[0]))
    untouched = (case["scale"] == F(1.0)) & (case["radius"] == 0)
    assert np.array_equal(bits(got[:, :, untouched]), bits(case["q"][:, :, untouched]))                 # copied: NaN payloads, -0 and denormals as they came
    if case["specials"]:                                                                                # (where they come out: test_optics_cpu.py; a warp may read past them)
        assert np.isnan(case["q"]).any() and np.isinf(case["q"]).any()


# ---- 2. from the context's state --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rendered(bins):
    """one render per bin count, two batches (the denoised source needs a variance); read-only for the tests that share it"""
    r = renderer()
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    start(r)
    q = develop_ref.raw_q(r.spectral_read(sums=True)[3], SPP)                                           # q rebuilt on the host from the exported sums
    assert (q != 0).any()
    return r, q


@pytest.mark.parametrize("bins", [8, 64])
def test_state_entry_equals_the_pure_entry_on_the_rebuilt_bins(bins):
    r, q = rendered(bins)
    pure = plain_context()
    w = np.random.default_rng(bins).uniform(-2, 3, size=(3, bins)).astype(F)
    for lens in (a_lens(bins, 3), a_lens(bins, 12, seed=1), a_lens(bins, 0, seed=2)):
        out, behind = r.develop(w, optics=lens, return_bins=True)
        want = pure.optics_images(q, lens)
        assert np.array_equal(bits(behind), bits(want)), (bins, lens["max_radius"])
        assert same(want, ref.optics(q, lens["cx"], lens["cy"], lens["max_radius"], lens["scale"], lens["radius"], lens["taps"]))
        assert np.array_equal(bits(out), bits(pure.develop_images(want, w)))
        assert not np.array_equal(bits(behind), bits(q))
    # either output alone, and neither
    op, keep = _optics_arg(lens, W, H)
    only_bins, only_out = np.zeros_like(q), np.zeros((H, W, 3), F)
    r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), None, 0, None, only_bins.ctypes.data))
    r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), w.ctypes.data, 3, only_out.ctypes.data, None))
    r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), w.ctypes.data, 3, None, None))
    assert np.array_equal(bits(only_bins), bits(behind)) and np.array_equal(bits(only_out), bits(out))


def test_state_entry_on_an_image_with_ragged_tiles():
    """21 x 13: the last tile column holds 5 pixels, the last tile row 5: the unpack kernel's lanes outside the image, rows that are no multiple of anything"""
    bins, res = 8, (21, 13)
    r = renderer(res=res)
    r.set_spectral_bins(bins)
    start(r)
    q = develop_ref.raw_q(r.spectral_read(sums=True)[3], SPP)
    assert q.shape == (13, 21, bins) and (q != 0).any()
    w = np.random.default_rng(9).uniform(-2, 3, size=(3, bins)).astype(F)
    for lens in (a_lens(bins, 3), identity_lens(bins)):
        out, behind = r.develop(w, optics=lens, return_bins=True)
        want = r.optics_images(q, lens)
        assert np.array_equal(bits(behind), bits(want))
        cx, cy = (res[0] / 2.0, res[1] / 2.0) if lens["cx"] is None else (lens["cx"], lens["cy"])
        assert same(want, ref.optics(q, cx, cy, lens["max_radius"], lens["scale"], lens["radius"], lens["taps"]))
        assert np.array_equal(bits(out), bits(r.develop_images(want, w)))
    assert np.array_equal(bits(out), bits(r.develop(w)))                                                # (the identity lens, last in the loop)


@pytest.mark.parametrize("bins", [8, 64])
def test_denoised_source_goes_through_the_same_lens(bins):
    r, _ = rendered(bins)
    pure = plain_context()
    w = np.random.default_rng(bins + 1).uniform(-2, 3, size=(5, bins)).astype(F)
    kw = dict(levels=3, sigma_l=4.0, sigma_a=0.037)
    filtered = r.denoise_spectral(**kw)
    lens = a_lens(bins, 3)
    out, behind = r.develop(w, denoise=kw, optics=lens, return_bins=True)
    want = pure.optics_images(filtered, lens)
    assert np.array_equal(bits(behind), bits(want))
    assert np.array_equal(bits(out), bits(pure.develop_images(want, w)))
    assert np.array_equal(bits(r.denoise_spectral(**kw)), bits(filtered))                               # the filter's buffers stayed as ssx_denoise_spectral needs them


@pytest.mark.parametrize("bins", [8, 64])
def test_identity_parameters_give_the_bits_of_the_plain_develop(bins):
    r, q = rendered(bins)
    w = np.random.default_rng(bins + 2).uniform(-2, 3, size=(4, bins)).astype(F)
    out, behind = r.develop(w, optics=identity_lens(bins), return_bins=True)
    assert np.array_equal(bits(out), bits(r.develop(w))) and np.array_equal(bits(behind), bits(q))
    kw = dict(levels=2)
    assert np.array_equal(bits(r.develop(w, denoise=kw, optics=identity_lens(bins))), bits(r.develop(w, denoise=kw)))
    lmin, lstep = float(r.scene.desc.contents.lambda_min), float(r.scene.desc.contents.lambda_step)
    assert np.array_equal(bits(r.develop(w, optics=lens_optics(bins, lmin, lstep))), bits(r.develop(w)))   # the host's lens of zeros


def test_the_lens_reads_only_and_the_render_continues():
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
    w = np.random.default_rng(3).uniform(-2, 3, size=(3, bins)).astype(F)
    r.develop(w, optics=a_lens(bins, 3)); r.develop(w, denoise={}, optics=a_lens(bins, 12, seed=1))
    r.render_continue(4); r.render_wait()
    assert r.done_spp() == 12 and np.array_equal(bits(r.xyza), bits(image))
    again = r.spectral_read(sums=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], spectral[1:]))


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_returns_its_code_and_a_message():
    bins = 8
    r = renderer()
    lib, ctx = r._lib, r._ctx
    q = np.random.default_rng(4).uniform(0, 1, size=(H, W, bins)).astype(F)
    out = np.zeros_like(q)
    lens = a_lens(bins, 3)

    def params(**over):
        d = dict(lens)
        struct_size = over.pop("struct_size", None)
        null = over.pop("null", None)
        d.update(over)
        p, keep = _optics_arg(d, W, H)
        if struct_size is not None:
            p.struct_size = struct_size
        if null:
            setattr(p, null, None)
        return p, keep

    def pure(p=None, qp=q.ctypes.data, op=out.ctypes.data, width=W, b=bins, optics=True):
        p = p or params()
        r._check(lib.ssx_optics_images(ctx, width, H, b, qp, C.byref(p[0]) if optics else None, op))

    pure()
    bad = lambda **over: (lambda: pure(params(**over)))
    refused(lambda: pure(qp=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: pure(op=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: pure(optics=False), _capi.SSX_ERR_ARG, "NULL")
    for field in ("scale", "radius", "taps"):
        refused(bad(null=field), _capi.SSX_ERR_ARG, "NULL")
    refused(bad(struct_size=C.sizeof(_capi.SsxOpticsParams) - 8), _capi.SSX_ERR_ARG, "struct_size")
    refused(bad(struct_size=0), _capi.SSX_ERR_ARG, "struct_size")
    p13 = params()
    p13[0].max_radius = 13
    refused(lambda: pure(p13), _capi.SSX_ERR_ARG, "max_radius")
    too_wide = lens["radius"].copy(); too_wide[5] = 4
    refused(bad(radius=too_wide), _capi.SSX_ERR_ARG, "radius[5]")
    for v in (0.0, -1.0, np.inf, np.nan):
        s = lens["scale"].copy(); s[2] = v
        refused(bad(scale=s), _capi.SSX_ERR_ARG, "scale[2]")
    for v in (np.inf, -np.inf, np.nan):
        refused(bad(cx=v), _capi.SSX_ERR_ARG, "cx")
        refused(bad(cy=v), _capi.SSX_ERR_ARG, "cy")
    for b in (0, 6, 68, 128):
        refused(lambda: pure(b=b), _capi.SSX_ERR_ARG, "multiple of 4")                                  # the bin and image-size refusals of ssx_develop_images
    refused(lambda: pure(width=0), _capi.SSX_ERR_ARG, "positive")
    refused(lambda: r._check(lib.ssx_optics_images(ctx, 1 << 20, 1 << 20, bins, q.ctypes.data, C.byref(params()[0]), out.ctypes.data)), _capi.SSX_ERR_ARG, "too large")

    # the state entry: ssx_spectral_develop's reasons first, then its own
    w = np.random.default_rng(5).uniform(-2, 3, size=(3, bins)).astype(F)
    refused(lambda: r.develop(w, optics=lens), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(bins)
    refused(lambda: r.develop(w, optics=lens), _capi.SSX_ERR_STATE, "no spectral bins", "no render")
    start(r)
    r.develop(w, optics=lens)
    refused(lambda: r.develop(w, denoise={}, optics=lens), _capi.SSX_ERR_STATE, "noise estimate is off")
    refused(lambda: r.develop(w, denoise=dict(levels=7), optics=lens), _capi.SSX_ERR_ARG, "levels")
    state = lambda p=None, wp=w.ctypes.data, ch=3, optics=True: r._check(lib.ssx_spectral_develop_optics(ctx, None, C.byref((p or params())[0]) if optics else None, wp, ch, out.ctypes.data, None))
    refused(lambda: state(optics=False), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: state(wp=None), _capi.SSX_ERR_ARG, "weights")
    for ch in (0, 17):
        refused(lambda: state(ch=ch), _capi.SSX_ERR_ARG, "channels")
    refused(lambda: state(params(null="taps")), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: state(params(struct_size=4)), _capi.SSX_ERR_ARG, "struct_size")
    refused(lambda: state(p13), _capi.SSX_ERR_ARG, "max_radius")
    refused(lambda: state(params(radius=too_wide)), _capi.SSX_ERR_ARG, "radius[5]")
    s = lens["scale"].copy(); s[7] = -0.5
    refused(lambda: state(params(scale=s)), _capi.SSX_ERR_ARG, "scale[7]")
    refused(lambda: state(params(cy=np.nan)), _capi.SSX_ERR_ARG, "cy")
    info, sums, s2 = r.export_sums()
    r.import_sums(info, sums, s2)
    refused(lambda: r.develop(w, optics=lens), _capi.SSX_ERR_STATE, "no spectral bins", "ssx_sums_import")
    # while a render runs
    start(r)
    r._check(lib.ssx_render_continue(ctx, 1 << 16))
    try:
        refused(lambda: r.develop(w, optics=lens), _capi.SSX_ERR_STATE, "render in progress")
        refused(pure, _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop(); r.render_wait()
    r.develop(w, optics=lens)


def test_a_context_that_owns_every_other_tile_is_refused():
    bins = 8
    r = renderer(tile_first=1, tile_stride=2)
    r.set_spectral_bins(bins)
    start(r)
    w = develop_weights(bins, float(r.scene.desc.contents.lambda_min), float(r.scene.desc.contents.lambda_step))
    r.develop(w)                                                                                        # the plain develop takes such a context
    refused(lambda: r.develop(w, optics=a_lens(bins)), _capi.SSX_ERR_STATE, "tile_stride", "neighbours")
    refused(lambda: r.develop(w, optics=identity_lens(bins)), _capi.SSX_ERR_STATE, "tile_stride")
