"""Finishing a development for a display without a GPU (include/ssx.h "Finishing a development for a display"): the symbols and the structs against the
header, the numpy restatement (tests/display_ref.py) against independent statements of what it computes, the host policy of include/ssx_host.h, and a halo check
of the self-guided filter on a step of eight octaves against a binary64 evaluation of the same formulas."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import display_cases as dc
import display_ref as ref
from simple_spectral_amd import _capi
from simple_spectral_amd.renderer import SsxError, display_matrix, meter_derive, tone_curve, tone_curve_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint32


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_libraries_export_the_entries():
    hip = open(os.path.join(ROOT, "include", "ssx.h")).read()
    host = open(os.path.join(ROOT, "include", "ssx_host.h")).read()
    for name in ("ssx_meter_images", "ssx_local_images", "ssx_tone_images"):
        assert "int %s(" % name in hip and name in _capi.HIP_SYMBOLS
    for name in ("ssh_meter_derive", "ssh_tone_curve", "ssh_display_matrix"):
        assert "int %s(" % name in host and name in _capi.HOST_SYMBOLS and hasattr(_capi.host_lib(), name)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "simple_spectral_amd", "libssx_hip.so")]).decode()
    for name in ("ssx_meter_images", "ssx_local_images", "ssx_tone_images"):
        assert " T %s\n" % name in nm


def test_the_parameter_structs_match_the_header():
    L, T = "ssx_local_params", "ssx_tone_params"
    lf = ("radius", "exposure", "y_lo", "y_hi", "eps", "pivot", "compress", "boost")
    tf = ("shift", "curve_len", "lo", "hi", "gains", "matrix", "curve")
    args = ["sizeof(%s)" % L] + ["offsetof(%s,%s)" % (L, f) for f in lf] + ["sizeof(%s)" % T] + ["offsetof(%s,%s)" % (T, f) for f in tf]
    args += ["(size_t)SSX_METER_KEYS", "(size_t)SSX_LOCAL_MAX_RADIUS", "(size_t)SSX_TONE_MAX_CURVE", "(size_t)SSH_METER_OUT", "(size_t)SSH_METER_GREY",
             "(size_t)SSH_METER_PATCH", "(size_t)SSH_METER_COUNT", "(size_t)SSH_TONE_FILMIC"]
    src = '#include "ssx_host.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % "".join('printf("%%zu ",%s);' % a for a in args)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    PL, PT = _capi.SsxLocalParams, _capi.SsxToneParams
    want = [C.sizeof(PL)] + [getattr(PL, f).offset for f in lf] + [C.sizeof(PT)] + [getattr(PT, f).offset for f in tf]
    want += [_capi.SSX_METER_KEYS, _capi.SSX_LOCAL_MAX_RADIUS, _capi.SSX_TONE_MAX_CURVE, _capi.SSH_METER_OUT, _capi.SSH_METER_GREY, _capi.SSH_METER_PATCH,
             _capi.SSH_METER_COUNT, _capi.SSH_TONE_FILMIC]
    assert got == want


# ---- the restatement against independent statements -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.meter_cases(), ids=[c["name"] for c in dc.meter_cases()])
def test_meter_ref_is_a_bincount_of_an_independent_key(case):
    hist, special = ref.meter(case["img"], case["luma"], case["mask"])
    keep = np.ones(case["img"].shape[:2], dtype=bool) if case["mask"] is None else case["mask"] != 0
    with np.errstate(all="ignore"):
        y = np.float32(0) + case["img"][..., 0] * case["luma"][0]
        y = y + case["img"][..., 1] * case["luma"][1]
        y = y + case["img"][..., 2] * case["luma"][2]
    for k, plane in enumerate([case["img"][..., 0], case["img"][..., 1], case["img"][..., 2], y]):
        with np.errstate(all="ignore"):
            x = plane[keep].astype(np.float64)                                            # the key from the value, not from the bits: frexp and the top four fraction bits
        ok = np.isfinite(x) & (x > 0)
        mant, expo = np.frexp(x[ok])                                                      # x = mant * 2^expo, mant in [0.5, 1)
        normal = expo >= -125
        key = np.where(normal, (expo + 126) * 16 + np.floor((mant * 2 - 1) * 16).astype(np.int64), np.floor(x[ok] * 2.0 ** 149 / 2 ** 19).astype(np.int64))
        assert np.array_equal(hist[k], np.bincount(key, minlength=4096).astype(U)), k
        assert special[k].tolist() == [int((x == 0).sum()), int((x < 0).sum()), int((x == np.inf).sum()), int(np.isnan(x).sum())]
        assert int(hist[k].sum()) + int(special[k].sum()) == int(keep.sum())
        assert not hist[k, 4080:].any()


def test_e_undoes_l_up_to_the_low_seven_bits():
    g = np.random.default_rng(7)
    y = np.concatenate([np.exp2(g.uniform(-126, 127.9, size=20000)).astype(F), np.array([2.0 ** -126, 1.0, 4.0, 3.4028234e38, 1.17549435e-38], dtype=F)])
    L = ref.log_l(np.stack([y, y, y], axis=-1)[None], np.array([0, 1, 0], dtype=F), 1.0, 2.0 ** -126, 3.4028234e38)[0]
    assert np.array_equal(ref.bits(ref.exp_e(L)), ref.bits(y) & U(0xFFFFFF80))
    assert L[-4] == 0.0 and L[-3] == 2.0
    bad = ref.exp_e(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], dtype=F))
    assert np.array_equal(ref.bits(bad), np.array([0x00800000, 0x7F7FFF80, 0x00800000, 0x7F7FFF80, 0x00800000], dtype=U))


def test_local_on_a_constant_image_is_exact():
    c = dc.constant_case()
    gain, base = ref.local(c["img"], c["luma"], **dc.local_params(c))
    assert (base == F(2.0)).all()
    want = ref.exp_e(np.array([F((F(2.0) - F(c["pivot"])) * F(c["compress"]) + F(c["pivot"])) - F(2.0)], dtype=F))[0]
    assert (gain == want).all() and want == F(0.21875)


def test_local_with_unit_compress_and_boost_leaves_the_image():
    c = next(c for c in dc.local_cases() if c["name"].endswith("identity"))
    gain, _ = ref.local(c["img"], c["luma"], **dc.local_params(c))
    assert np.abs(np.log2(gain.astype(np.float64))).max() < 2e-5          # Lo - L is a few rounding errors of L, |L| < 32: a few 2^-19, and E floors to 2^-16


def test_tone_on_nodes_returns_the_table():
    for shift, (lo, hi) in ((12, (2.0 ** -4, 8.0)), (19, (2.0 ** -12, 10.0)), (23, (2.0 ** -12, 16.0))):
        n = ref.curve_len(lo, hi, shift)
        assert n == tone_curve_len(lo, hi, shift)
        nd = ref.nodes(lo, hi, shift)
        inside = nd <= F(hi)
        curve = dc.wild_curve(np.random.default_rng(shift), n)
        img = np.zeros((1, n, 3), dtype=F)
        img[0, :, 0] = nd
        out = ref.tone(img, curve, lo, hi, shift, matrix=[[1, 0, 0], [1, 0, 0], [1, 0, 0]])
        assert np.array_equal(ref.bits(out[0, inside, 1]), ref.bits(curve[inside]))
        assert np.count_nonzero(~inside) <= 1


# ---- the host policy ----------------------------------------------------------------------------------------------------------------------------------------------

def srgb(v):
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)


def hable(x):
    A, B, Cc, D, E, Fh = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return (x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * Fh) - E / Fh


def test_the_tone_curves_against_binary64_formulas():
    lo, hi, shift, white = 2.0 ** -12, 16.0, 19, 5.5
    x = ref.nodes(lo, hi, shift).astype(np.float64)
    for kind, t in (("clip", x), ("reinhard", x * (1 + x / white ** 2) / (1 + x)), ("filmic", hable(2 * x) / hable(white))):
        want = srgb(np.clip(t, 0.0, 1.0))
        got = tone_curve(kind, lo, hi, shift, white=white)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(F)).astype(np.float64)).all(), kind     # one binary32 rounding (libm's pow may differ by its last bit)
        assert (np.diff(got) >= 0).all() and got[0] >= 0 and got[-1] == 1.0
    for kw in (dict(kind="reinhard", white=0.0), dict(kind="clip", shift=11), dict(kind="clip", lo=0.0), dict(kind="clip", lo=2.0 ** -20, hi=2.0 ** 20, shift=12)):
        a = dict(kind="clip", lo=lo, hi=hi, shift=shift, white=1.0); a.update(kw)
        with pytest.raises(SsxError) as e:
            tone_curve(a["kind"], a["lo"], a["hi"], a["shift"], white=a["white"])
        assert e.value.code == _capi.SSX_ERR_ARG
    with pytest.raises(ValueError):
        tone_curve("aces", lo, hi, shift)


def test_the_display_matrix_is_the_projects_xyz_to_srgb():
    m = display_matrix().astype(np.float64)
    std = np.array([[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415], [0.0557, -0.2040, 1.0570]])                       # IEC 61966-2-1
    assert np.allclose(m * (std[1, 1] / m[1, 1]), std, atol=0.03)                     # up to the project's radiometric scale of D65 (and its own white point's digits)
    from simple_spectral_amd.renderer import Scene
    s = Scene("cornell-srgb", texture="test-img.png")
    assert np.array_equal(display_matrix(), s.color_values("xyz_to_lrgb").reshape(3, 3).T)


def an_image():
    g = np.random.default_rng(11)
    img = np.exp2(g.normal(-3.0, 2.5, size=(40, 50, 3))).astype(F)
    img[:4, :6] *= F(300.0)                                                               # a light
    return img


def test_a_percentile_is_within_one_key_of_a_sort():
    img = an_image()
    hist, special = ref.meter(img, dc.LUMA)
    ps = (0.0, 0.01, 0.5, 0.9, 0.99, 1.0)
    got = meter_derive(hist, special, percentiles=ps)["percentiles"]
    planes = [img[..., 0], img[..., 1], img[..., 2], ref.luminance(img, dc.LUMA)]
    for k in range(4):
        x = np.sort(planes[k].reshape(-1))
        for p, v in zip(ps, got[k]):
            at = x[min(max(int(np.ceil(p * x.size)), 1), x.size) - 1]
            assert int(ref.bits(v).reshape(-1)[0]) == (int(ref.bits(at).reshape(-1)[0]) >> 19) << 19, (k, p)        # the lower edge of the key the sorted value lies in
            assert v <= at < v * (1 + 1 / 16)                                             # a key is a sixteenth of its octave's start wide
    m = meter_derive(hist, special, white_percentile=0.99)
    assert m["white"] == got[3][4] and m["count"] == 2000
    for bad in (dict(key=0.0), dict(white_percentile=1.5), dict(percentiles=(2.0,))):
        with pytest.raises(SsxError) as e:
            meter_derive(hist, special, **bad)
        assert e.value.code == _capi.SSX_ERR_ARG


def test_the_exposure_of_a_scaled_image_scales_exactly():
    img = an_image()
    base = meter_derive(*ref.meter(img, dc.LUMA))
    truth = 0.18 / np.exp(np.mean(np.log(ref.luminance(img, dc.LUMA).astype(np.float64))))
    assert abs(np.log2(base["exposure"] / truth)) < 0.09                                  # the piecewise-linear log is within 0.0861 of log2, a key's centre within 1/32
    assert base["pivot"] == ref.log_l(np.full((1, 1, 3), 0.18, dtype=F), [0, 1, 0], 1.0, 2.0 ** -126, 1e38)[0, 0]
    for k in (-7, -1, 3, 10):
        scaled = (img * F(2.0 ** k)).astype(F)                                            # exact: powers of two, nothing leaves the normal range
        m = meter_derive(*ref.meter(scaled, dc.LUMA))
        assert m["exposure"] == F(base["exposure"] * F(2.0 ** -k)) and m["log_average"] == F(base["log_average"] * F(2.0 ** k)), k
        assert np.array_equal(m["grey"], base["grey"]) and np.array_equal(m["patch"], base["patch"])
    grey = meter_derive(*ref.meter(img * np.array([2.0, 1.0, 0.5], dtype=F), dc.LUMA))
    assert np.allclose(grey["grey"] / base["grey"], [0.5, 1.0, 2.0], rtol=1e-6) and np.allclose(grey["patch"] / base["patch"], [0.5, 1.0, 2.0], rtol=1e-6)
    empty = meter_derive(np.zeros((4, 4096), U), np.zeros((4, 4), U))
    assert empty["exposure"] == 1.0 and empty["log_average"] == 0.0 and empty["white"] == 0.0 and (empty["grey"] == 1.0).all()


# ---- the halo check ---------------------------------------------------------------------------------------------------------------------------------------------

def box64(P, r):
    H, W = P.shape
    ii, jj = np.arange(W), np.arange(H)
    h = sum(P[:, np.clip(ii + dx, 0, W - 1)] for dx in range(-r, r + 1))
    return sum(h[np.clip(jj + dy, 0, H - 1), :] for dy in range(-r, r + 1))


def base64(L, r, eps):
    """the header's formulas for base in binary64, on the same (exact) L"""
    L = L.astype(np.float64)
    n = float((2 * r + 1) ** 2)
    m = box64(L, r) / n
    v = np.maximum(box64(L * L, r) / n - m * m, 0.0)
    a = v / (v + eps)
    b = m - a * m
    return box64(a, r) / n * L + box64(b, r) / n


# The tolerance.  A bound derived from worst-case roundings is useless here: the cancellation in v = S2/n - m m costs (3 n + 2) u Lmax^2 = 1.2e-3 absolutely,
# against eps = 0.01 that is 0.12 in a, two octaves in base -- every rounding aligned, which never happens.  So, as the issue allows, the figure is MEASURED ON THE
# BINARY64 EVALUATION, never on the binary32 code: the same formulas in binary64 with every operation's result multiplied by (1 + u d), u = 2^-24 (a binary32
# rounding's largest relative error), d uniform in [-1, 1] and independent per operation and pixel -- the standard model of rounding.  HALO_TRIALS seeded runs; the
# largest deviation from the unperturbed evaluation over all pixels and runs is the figure, and the restatement may differ from binary64 by HALO_MARGIN times it:
# the model's d has the spread of a real rounding error but sixteen runs do not reach its tail, and the restatement's roundings are not independent.
HALO_TRIALS, HALO_MARGIN = 16, 8.0


def base64_rounded(L, r, eps, g):
    """base64 with the rounding model on every operation"""
    u = 2.0 ** -24
    rd = lambda x: x * (1.0 + u * g.uniform(-1.0, 1.0, size=np.shape(x)))
    H, W = L.shape
    ii, jj = np.arange(W), np.arange(H)

    def box(P):
        h = np.zeros((H, W))
        for dx in range(-r, r + 1):
            h = rd(h + P[:, np.clip(ii + dx, 0, W - 1)])
        s = np.zeros((H, W))
        for dy in range(-r, r + 1):
            s = rd(s + h[np.clip(jj + dy, 0, H - 1), :])
        return s
    n = float((2 * r + 1) ** 2)
    m = rd(box(L) / n)
    v = np.maximum(rd(rd(box(rd(L * L)) / n) - rd(m * m)), 0.0)
    a = rd(v / rd(v + eps))
    b = rd(m - rd(a * m))
    return rd(rd(rd(box(a) / n) * L) + rd(box(b) / n))


def test_the_base_layer_of_a_step_of_eight_octaves_has_no_halo_of_rounding():
    """Figures (profiles/r32/NOTES.md): max |base32 - base64| = 2.84e-05 octaves; the rounding model on the binary64 evaluation gives 3.62e-05; the tolerance is
    HALO_MARGIN = 8 times the model's figure, 2.9e-04 octaves."""
    r, eps = 4, 0.01
    y = np.full((24, 48), 2.0 ** -4, dtype=F)
    y[:, 24:] = 2.0 ** 4                                                                  # eight octaves
    y *= np.exp2(np.random.default_rng(3).uniform(-0.05, 0.05, size=y.shape)).astype(F)   # a little texture on both sides
    img = np.stack([y, y, y], axis=-1)
    luma = np.array([0, 1, 0], dtype=F)
    p = dict(radius=r, exposure=32.0, y_lo=2.0 ** -20, y_hi=2.0 ** 20, eps=eps, pivot=0.0, compress=0.5, boost=1.0)   # exposure 32: L in 0.9 .. 9.1, all positive
    L = ref.log_l(img, luma, p["exposure"], p["y_lo"], p["y_hi"])
    assert L.min() >= 0 and L.max() <= 9.1
    _, base = ref.local(img, luma, **p)
    want = base64(L, r, eps)
    err = np.abs(base.astype(np.float64) - want).max()
    L64 = L.astype(np.float64)
    model = max(np.abs(base64_rounded(L64, r, eps, np.random.default_rng(100 + k)) - want).max() for k in range(HALO_TRIALS))
    print("halo check: max |base32 - base64| = %.3g octaves; the rounding model on the binary64 evaluation gives %.3g, the tolerance is %g times that: %.3g" % (err, model, HALO_MARGIN, HALO_MARGIN * model))
    assert err <= HALO_MARGIN * model
    assert HALO_MARGIN * model < 1e-3                                                     # the tolerance itself says something: a thousandth of an octave
    # no halo, on the binary32 base under test: two pixels from the step the base follows L, not the window's mean (which is half way, 4 octaves off)
    off = np.abs(base.astype(np.float64) - L.astype(np.float64))
    assert off[:, [21, 26]].max() < 0.5 and off[:, :16].max() < 0.06 and off[:, 32:].max() < 0.06
