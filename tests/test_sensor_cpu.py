"""Developing onto a sensor without a GPU (include/ssx.h "Developing onto a sensor"): the numpy restatement (tests/sensor_ref.py) against what the definition
implies, the host library's Bayer tables, exposure scales and colour matrix (include/ssx_host.h) against the published stencils and their closed forms, the
noise against the statistics of a standard normal, and the parameter struct and the exported symbols against the headers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import develop_ref
import sensor_cases as sc
import sensor_ref as ref
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.renderer import SsxError, sensor_bayer, sensor_ccm, sensor_exposure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TABLES = [(p, m) for p in ref.PATTERNS for m in ("mhc", "bilinear")]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def both_tables(pattern, method):
    """the host library's tables and the restatement's, which must be the same bits"""
    lib = sensor_bayer(pattern, method)
    cfa, taps = ref.bayer(pattern, method)
    assert np.array_equal(lib["cfa"], cfa) and np.array_equal(bits(lib["taps"]), bits(taps)), (pattern, method)
    return lib["cfa"], lib["taps"]


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern,method", TABLES)
def test_the_taps_sum_to_one_and_reproduce_constants_and_ramps(pattern, method):
    cfa, taps = both_tables(pattern, method)
    assert sorted(cfa.tolist()) == [0, 1, 1, 2] and cfa[0] == "RGB".index(pattern[0]) and cfa[3] == "RGB".index(pattern[3])
    assert np.array_equal(taps.astype(np.float64).sum(axis=2), np.ones((4, 3)))                        # dyadic coefficients: the sum is exact
    for (W, H) in sc.SIZES:
        const = np.full((H, W), F(0.625))                                                               # dyadic: every partial sum is exact
        assert np.array_equal(bits(ref.demosaic(const, taps, ref.IDENTITY_CCM)), bits(np.full((H, W, 3), F(0.625)))), (W, H)
    W, H = 37, 23
    j, i = np.mgrid[0:H, 0:W]
    ramp = (3 * i + 2 * j + 1).astype(F)                                                                # small integers times eighths: exact again
    out = ref.demosaic(ramp, taps, ref.IDENTITY_CCM)
    assert np.array_equal(out[2:-2, 2:-2], np.repeat(ramp[2:-2, 2:-2, None], 3, axis=2))               # the corrections are Laplacians: they vanish on a ramp
    assert not np.array_equal(out[:, :2], np.repeat(ramp[:, :2, None], 3, axis=2))                     # ... but a mirrored ramp is not a ramp


def test_the_four_patterns_are_shifts_of_one_another():
    for method in ("mhc", "bilinear"):
        cfa0, taps0 = both_tables("RGGB", method)
        for pattern, flip in (("GRBG", 1), ("GBRG", 2), ("BGGR", 3)):                                  # a shift by one pixel in i, in j, in both
            cfa, taps = both_tables(pattern, method)
            for phase in range(4):
                assert cfa[phase] == cfa0[phase ^ flip] and np.array_equal(bits(taps[phase]), bits(taps0[phase ^ flip])), (pattern, phase)
    # and on an image: the mosaic of a shifted scene under the shifted pattern is the shifted mosaic
    g = np.random.default_rng(5)
    raw = g.uniform(0, 1, size=(12, 14)).astype(F)
    a = ref.demosaic(raw, ref.bayer("RGGB", "mhc")[1], ref.IDENTITY_CCM)
    b = ref.demosaic(raw[1:, 1:], ref.bayer("BGGR", "mhc")[1], ref.IDENTITY_CCM)
    assert np.array_equal(bits(a[3:-2, 3:-2]), bits(b[2:-2, 2:-2]))


@pytest.mark.parametrize("pattern,method", TABLES)
def test_the_stencils_at_green_sites_point_along_the_right_axis(pattern, method):
    """Pins the orientation of the R / B stencils at G sites without the rule that builds them.  A scene whose R and B planes depend on the row alone (any
    function of j: here j * j + 1 and 3 j * j + 2, not ramps) and whose G plane is constant: at a G photosite the colour carried by its LEFT AND RIGHT
    neighbours -- read off the pattern's letters -- must come out exactly, because both neighbours hold that row's value and the G corrections cancel on a
    constant (everything dyadic).  The transposed stencil would average the rows above and below, or reach for the other colour's sites.  Then the same with
    columns: planes that depend on i alone are exact for the colour carried by the neighbours ABOVE AND BELOW."""
    lib = sensor_bayer(pattern, method)
    H, W = 12, 14
    j, i = np.mgrid[0:H, 0:W]
    letter = np.array(list(pattern))[(j & 1) * 2 + (i & 1)]
    beside = np.array(list(pattern))[(j & 1) * 2 + ((i + 1) & 1)]                                      # the letter left and right of each photosite
    above = np.array(list(pattern))[((j + 1) & 1) * 2 + (i & 1)]
    for t, along in ((j, beside), (i, above)):
        planes = {"R": (t * t + 1).astype(F), "G": np.full((H, W), F(5.0)), "B": (3 * t * t + 2).astype(F)}
        raw = np.select([letter == "R", letter == "G"], [planes["R"], planes["G"]], planes["B"]).astype(F)
        out = ref.demosaic(raw, lib["taps"], ref.IDENTITY_CCM)
        inside = np.zeros((H, W), bool)
        inside[2:-2, 2:-2] = True
        for c, name in enumerate("RGB"):
            if name == "G":
                continue
            exact = inside & (letter == "G") & (along == name)
            other = inside & (letter == "G") & (along != name)
            assert exact.sum() >= 8 and np.array_equal(out[..., c][exact], planes[name][exact]), (name, "along" if t is j else "across")
            assert not np.array_equal(out[..., c][other], planes[name][other])                         # the other kind of G site interpolates a parabola: not exact


def test_mhc_beats_bilinear_on_a_smooth_colour_image():
    """not a bound: the reason the second method exists -- on a band-limited colour image the corrected filters interpolate better"""
    j, i = np.mgrid[0:24, 0:32]
    img = np.stack([1.0 + 0.5 * np.sin(0.5 * i + 0.3 * j), 1.0 + 0.5 * np.sin(0.5 * i + 0.3 * j + 0.2), 1.0 + 0.5 * np.sin(0.5 * i + 0.3 * j - 0.2)], axis=2).astype(F)
    err = {}
    for method in ("mhc", "bilinear"):
        cfa, taps = ref.bayer("RGGB", method)
        raw = np.take_along_axis(img, ref.cfa_map(cfa, 24, 32)[..., None], axis=2)[..., 0]
        err[method] = np.abs(ref.demosaic(raw, taps, ref.IDENTITY_CCM) - img)[2:-2, 2:-2].mean()
    assert err["mhc"] < err["bilinear"]


def test_the_host_refuses_other_patterns_and_methods():
    for pattern, method in (("RGBG", "mhc"), ("rggb", "mhc"), ("", "mhc"), ("RGGBX", "bilinear")):
        with pytest.raises(SsxError) as e:
            sensor_bayer(pattern, method)
        assert e.value.code == _capi.SSX_ERR_ARG and "pattern" in str(e.value)
    cfa, taps = np.zeros(4, np.uint32), np.zeros(300, F)
    assert _capi.host_lib().ssh_sensor_bayer(b"RGGB", 2, cfa.ctypes.data, taps.ctypes.data) == _capi.SSX_ERR_ARG
    assert _capi.host_lib().ssh_sensor_bayer(b"RGGB", 1, None, taps.ctypes.data) == _capi.SSX_ERR_ARG


# ---- DEMOSAIC ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_identity_tables_give_raw_in_all_three_channels():
    """bit for bit for finite raw that is not -0: a zero coefficient on an inf is a NaN, and 0.0f + (-0 * 1) is +0, as the arithmetic of the header says"""
    g = np.random.default_rng(6)
    for (W, H) in sc.SIZES:
        raw = g.uniform(-3, 3, size=(H, W)).astype(F)
        raw.reshape(-1)[:3] = np.array([0x00000007, 0x80000001, 0x00000000], dtype=np.uint32).view(F)
        out = ref.demosaic(raw, ref.IDENTITY_TAPS, ref.IDENTITY_CCM)
        assert np.array_equal(bits(out), bits(np.repeat(raw[..., None], 3, axis=2)))
    raw[1, 1] = F(-0.0)
    assert ref.demosaic(raw, ref.IDENTITY_TAPS, ref.IDENTITY_CCM)[1, 1].view(np.uint32).tolist() == [0, 0, 0]


def test_the_border_is_mirrored_and_the_cases_tell_it_from_a_clamp():
    assert ref.mirror(np.array([-2, -1, 0, 4, 5, 6]), 5).tolist() == [2, 1, 0, 4, 3, 2]
    assert ref.mirror(np.array([-2, -1, 3, 4]), 3).tolist() == [2, 1, 1, 0]                             # the smallest image the entries take
    hit = 0
    for c in sc.cases():
        raw, _ = ref.sensor(**sc.sensor_of(c), q=c["q"])
        a, b = ref.demosaic(raw, c["taps"], c["ccm"]), ref.demosaic(raw, c["taps"], c["ccm"], mutant="clamp")
        differ = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
        hit += bool(differ.any())
        assert not differ[2:-2, 2:-2].any()
    assert hit >= len(sc.cases()) - 2


# ---- SENSOR -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_a_plain_sensor_is_the_develop_at_the_photosites_filter():
    for c in sc.cases():
        s = dict(sc.sensor_of(c), noise=0, white=0.0, exposure=1.0, inv_exposure=1.0)
        raw, dn = ref.sensor(q=c["q"], **s)
        H, W, _ = c["q"].shape
        img = develop_ref.develop(c["q"], c["weights"])
        want = np.take_along_axis(img, ref.cfa_map(c["cfa"], H, W)[..., None], axis=2)[..., 0]
        assert dn is None and not ((bits(raw) != bits(want)) & ~(np.isnan(raw) & np.isnan(want))).any(), c["name"]


def test_the_case_list_covers_what_the_issue_names():
    cs = sc.cases()
    shapes = {c["q"].shape for c in cs}
    assert {(H, W, B) for (W, H) in sc.SIZES for B in sc.BINS} <= shapes
    assert {n for c in cs for n in ref.PATTERNS if n in c["name"]} == set(ref.PATTERNS)
    assert any("mhc" in c["name"] for c in cs) and any("bilinear" in c["name"] for c in cs)
    assert any(c["noise"] and c["white"] > 0 for c in cs) and any(c["noise"] and not c["white"] for c in cs) and any(not c["noise"] and c["white"] > 0 for c in cs)
    edges = [c for c in cs if c["name"].startswith("edges")]
    for c in edges:
        q = c["q"]
        assert np.isnan(q).any() and np.isinf(q).any() and (bits(q) == 0x80000000).any() and ((np.abs(q) < np.finfo(F).tiny) & (q != 0)).any()
        raw, dn = ref.sensor(q=q, **sc.sensor_of(c))
        v = develop_ref.develop(q, c["weights"])
        assert (v < 0).any() and np.isnan(v).any() and np.isfinite(raw).any()
        if dn is None:
            assert np.isnan(raw).any() and np.isinf(raw).any()
        else:
            assert (dn == 0).any() and (dn == F(c["white"])).any() and np.isfinite(dn).all()           # both clamps bite; a NaN count is 0


def test_the_adc_counts_in_whole_numbers_and_a_full_well_lands_on_white():
    s = sensor_exposure(full_well=20000.0, white_level=2.0, bits=12, black=64.0, read_e=2.5)
    assert s["white"] == 4095.0 and s["black"] == 64.0 and s["exposure"] == 10000.0 and s["inv_exposure"] == F(1e-4) and s["read_var"] == 6.25
    assert s["dn_per_e"] == F(4031.0 / 20000.0) and s["e_per_dn"] == F(20000.0 / 4031.0)
    W, H, B = 37, 23, 4
    w = np.zeros((3, B), F)
    w[:, 0] = 1.0
    q = np.zeros((H, W, B), F)
    q[..., 0] = np.linspace(-0.25, 2.5, W * H).astype(F).reshape(H, W)
    q[0, 0, 0], q[5, 5, 0], q[H - 1, W - 1, 0] = 0.0, 2.0, 2.0                                           # black, and white_level itself at two phases
    cfa, _ = ref.bayer("RGGB", "mhc")
    for noise in (0, 1):
        raw, dn = ref.sensor(q, w, cfa, noise=noise, seed=3, **s)
        assert np.array_equal(dn, np.floor(dn)) and dn.min() == 0.0 and dn.max() == 4095.0
        if not noise:
            assert dn[0, 0] == 64.0 and dn[5, 5] == 4095.0 and dn[H - 1, W - 1] == 4095.0 and (dn[q[..., 0] > 2.0] == 4095.0).all()
            assert (np.diff(dn.reshape(-1)[np.argsort(q[..., 0].reshape(-1), kind="stable")]) >= 0).all()    # the count never falls as the light grows
            inside = (dn > 0) & (dn < 4095)
            assert np.abs(raw - q[..., 0])[inside].max() <= 0.5 * 2.0 / 4031.0 * 1.001                  # half a step of the ADC, in the develop's units
    none = sensor_exposure(full_well=20000.0, white_level=2.0)
    assert none["white"] == 0.0 and none["read_var"] == 0.0 and ref.sensor(q, w, cfa, **none)[1] is None
    for kw in (dict(full_well=0.0), dict(white_level=-1.0), dict(bits=25), dict(bits=8, black=255.0), dict(black=-1.0), dict(read_e=-0.5), dict(full_well=float("nan")), dict(read_e=1e30)):
        args = dict(full_well=20000.0, white_level=2.0)
        args.update(kw)
        with pytest.raises(SsxError) as e:
            sensor_exposure(**args)
        assert e.value.code == _capi.SSX_ERR_ARG and "ssh_sensor_exposure" in str(e.value), kw


def test_the_noise_is_a_standard_normal_with_the_poisson_variance():
    """A flat field of N = 4096 photosites at 1000 electrons, read noise 2 electrons: e = 1000 + sd z with sd^2 = 1004.  Every bound is five standard errors of
    its statistic for N independent standard normals: the mean's is sigma / sqrt(N); the variance's is sqrt(2 / N) relative (the fourth moment of the sum of
    twelve uniforms is 2.9, below the normal's 3, so the bound is on the safe side); a correlation coefficient's is 1 / sqrt(N)."""
    side = 64
    N = side * side
    B = 4
    q = np.full((side, side, B), F(0.25))
    w = np.ones((3, B), F)                                                                             # v = 1 exactly at every photosite
    cfa, _ = ref.bayer("RGGB", "mhc")
    kw = dict(exposure=1000.0, inv_exposure=1.0, noise=1, read_var=4.0)                                # inv_exposure 1: raw stays in electrons
    e = ref.sensor(q, w, cfa, seed=11, frame=0, **kw)[0].astype(np.float64)
    var = 1000.0 + 4.0
    sigma = np.sqrt(var)
    assert abs(e.mean() - 1000.0) <= 5.0 * sigma / np.sqrt(N)
    assert abs(e.var() / var - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    z = (e - 1000.0) / sigma
    corr = lambda a, b: float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))
    other = (ref.sensor(q, w, cfa, seed=11, frame=1, **kw)[0].astype(np.float64) - 1000.0) / sigma
    for name, r in (("i", corr(z[:, :-1], z[:, 1:])), ("j", corr(z[:-1], z[1:])), ("frame", corr(z, other))):
        assert abs(r) <= 5.0 / np.sqrt(N), (name, r)
    reseeded = ref.sensor(q, w, cfa, seed=12, frame=0, **kw)[0]
    assert (reseeded != e.astype(F)).all()
    assert np.abs(z).max() <= 6.0 and np.abs(z).max() > 3.0                                            # the tails end at +-6 and are there
    zz = ref.normal(np.arange(N), 11, 0)
    assert zz.dtype == F and np.array_equal(zz * F(65536.0), np.round(zz * F(65536.0)))               # integers only: z is a whole number of 2^-16
    assert int(ref.hash32(np.uint32(0))) == 0 and int(ref.hash32(np.uint32(1))) != 1


# ---- the colour matrix -----------------------------------------------------------------------------------------------------------------------------------------

def test_the_colour_matrix_recovers_a_known_map():
    """target = A cam with a dyadic A and small-integer curves is exact in binary32, and so are cam cam^T and target cam^T in the library's binary64.  What is
    left is the 3 x 3 solve by the adjugate: its relative error is a modest multiple of kappa(cam cam^T) 2^-53 -- 64 covers the 2 x 2 minors, the determinant
    and the three-term products of n = 3 -- and the one rounding to binary32 at the end, 2^-24 relative."""
    g = np.random.default_rng(8)
    for B in (4, 16, 64):
        cam = g.integers(0, 16, size=(3, B)).astype(F)
        A = (g.integers(-16, 17, size=(3, 3)) / 8.0).astype(F)
        target = (A.astype(np.float64) @ cam.astype(np.float64)).astype(F)
        assert np.array_equal(target.astype(np.float64), A.astype(np.float64) @ cam.astype(np.float64))
        G = cam.astype(np.float64) @ cam.astype(np.float64).T
        bound = 64.0 * np.linalg.cond(G) * 2.0 ** -53 * np.abs(A).max() + 2.0 ** -24 * np.abs(A)
        got = sensor_ccm(cam, target)
        assert got.dtype == F and (np.abs(got.astype(np.float64) - A) <= bound).all(), B
    cam[2] = cam[0] + cam[1]
    for bad in (cam, np.zeros((3, 8), F)):
        with pytest.raises(SsxError) as e:
            sensor_ccm(bad, bad)
        assert e.value.code == _capi.SSX_ERR_ARG and "singular" in str(e.value)


# ---- the struct and the symbols ----------------------------------------------------------------------------------------------------------------------------

def test_the_parameter_struct_matches_the_header():
    names = [n for n, _ in _capi.SsxSensorParams._fields_]
    src = ('#include "ssx.h"\n#include "ssx_host.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(ssx_sensor_params));\n'
           + "".join('printf(" %%zu", offsetof(ssx_sensor_params, %s));\n' % n for n in names) + 'printf(" %d %d\\n", SSH_DEMOSAIC_BILINEAR, SSH_DEMOSAIC_MHC);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    P = _capi.SsxSensorParams
    assert got == [C.sizeof(P)] + [getattr(P, n).offset for n in names] + [_capi.SSH_DEMOSAIC_BILINEAR, _capi.SSH_DEMOSAIC_MHC]


def test_the_libraries_export_the_new_symbols():
    hip, host = C.CDLL(sbuild.HIP_LIB), _capi.host_lib()
    for s in ("ssx_sensor_images", "ssx_demosaic_images", "ssx_spectral_develop_sensor"):
        assert s in _capi.HIP_SYMBOLS and hasattr(hip, s), s
    for s in ("ssh_sensor_bayer", "ssh_sensor_exposure", "ssh_sensor_ccm", "ssh_sensor_standin_curve"):
        assert s in _capi.HOST_SYMBOLS and hasattr(host, s), s


def test_the_stand_in_curves_are_the_gaussians_the_header_states():
    from simple_spectral_amd.renderer import sensor_standin_curves
    lam = 380.0 + 5.0 * np.arange(71)
    for (s, low, high), peak in zip(sensor_standin_curves(), (600.0, 540.0, 460.0)):
        want = np.exp(-0.5 * ((lam - peak) / 35.0) ** 2).astype(F)
        assert (low, high) == (380.0, 730.0) and s.dtype == F and s.shape == (71,)
        assert (np.abs(s - want) <= np.spacing(want)).all() and s.max() == 1.0 and lam[int(np.argmax(s))] == peak      # exp is libm's on both sides: one ulp
    buf, lo, hi = np.zeros(71, F), C.c_float(), C.c_float()
    assert _capi.host_lib().ssh_sensor_standin_curve(3, buf.ctypes.data, C.byref(lo), C.byref(hi)) == _capi.SSX_ERR_ARG
    assert _capi.host_lib().ssh_sensor_standin_curve(0, None, C.byref(lo), C.byref(hi)) == _capi.SSX_ERR_ARG
