"""The colour difference of two developments without a GPU (include/ssx.h "Colour difference of two developments"): the numpy restatement
(tests/delta_e_ref.py) against closed forms derived here, the host library's white, derived figures and CSV writer against numpy, and the two properties of the
fixed-seed inputs (tests/delta_e_cases.py) that the GPU tests rely on: they tell a wrong reduction from the right one, and few of them lie near a branch point."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import delta_e_cases as cases
import delta_e_ref as ref
from simple_spectral_amd import _capi
from simple_spectral_amd import build as sbuild
from simple_spectral_amd import renderer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
D65 = os.path.join(ROOT, "data", "d65-300+5+780.csv")


def pair(lab1, lab2):
    """(dE*ab, dE00, parts) of two Lab triples"""
    a, b = tuple(np.float64(v) for v in lab1), tuple(np.float64(v) for v in lab2)
    e00, parts = ref.delta_e_00(a, b, parts=True)
    return float(ref.delta_e_ab(a, b)), float(e00), {k: float(v) for k, v in parts.items()}


def polar(L, C, h):
    return (L, C * math.cos(math.radians(h)), C * math.sin(math.radians(h)))


# ---- 1. closed forms --------------------------------------------------------------------------------------------------------------------------------------

def test_identity_and_symmetry():
    a, b, wa, wb = cases.images((42, 23))
    de, _ = ref.maps(a, a, wa, wa)
    fin = np.isfinite(de)
    assert (de[fin] == 0.0).all() and fin.mean() > 0.99                                # dE(x, x) = 0 exactly
    ab, ba = ref.maps(a, b, wa, wb)[0], ref.maps(b, a, wb, wa)[0]
    assert np.array_equal(ab, ba, equal_nan=True)                                      # symmetric in A and B, bit for bit


def test_neutral_greys():
    for L1, L2 in ((50.0, 60.0), (20.0, 25.0), (90.0, 10.0)):
        eab, e00, _ = pair((L1, 0.0, 0.0), (L2, 0.0, 0.0))
        Lm = 0.5 * (L1 + L2)
        SL = 1.0 + 0.015 * (Lm - 50.0) ** 2 / math.sqrt(20.0 + (Lm - 50.0) ** 2)       # C' = 0: dC' = dH' = 0, only the lightness term is left
        assert eab == abs(L1 - L2)
        assert e00 == pytest.approx(abs(L1 - L2) / SL, rel=1e-15)


def test_pure_a_step_at_equal_lightness():
    a1, a2 = 10.0, 14.0
    eab, e00, p = pair((50.0, a1, 0.0), (50.0, a2, 0.0))
    assert eab == a2 - a1
    Cm = 0.5 * (a1 + a2)
    G = 0.5 * (1.0 - math.sqrt(Cm ** 7 / (Cm ** 7 + 25.0 ** 7)))
    c1, c2 = (1.0 + G) * a1, (1.0 + G) * a2                                            # b = 0, a > 0: h' = 0 on both sides, dH' = 0, C' = a'
    SC = 1.0 + 0.045 * 0.5 * (c1 + c2)
    assert p["h1"] == 0.0 and p["h2"] == 0.0 and p["dH"] == 0.0
    assert e00 == pytest.approx((c2 - c1) / SC, rel=1e-13)                             # dL' = 0; the rotation term multiplies dH' = 0


def test_both_sides_of_every_rule():
    # a' = (1 + G) a turns the hues a little: the primed hues by hand, C = 30 on both sides
    G = 0.5 * (1.0 - math.sqrt(30.0 ** 7 / (30.0 ** 7 + 25.0 ** 7)))

    def primed(h):
        return math.degrees(math.atan2(30.0 * math.sin(math.radians(h)), (1.0 + G) * 30.0 * math.cos(math.radians(h)))) % 360.0
    rules = [(10, 100, False, lambda d, s: (d, 0.5 * s)),                        # |dh'| <= 180: the plain difference and mean
             (10, 200, True, lambda d, s: (d - 360.0, 0.5 * (s + 360.0))),       # d > 180, h1 + h2 < 360
             (200, 10, True, lambda d, s: (d + 360.0, 0.5 * (s + 360.0))),       # d < -180
             (300, 100, True, lambda d, s: (d + 360.0, 0.5 * (s - 360.0))),      # |dh'| > 180, h1 + h2 >= 360
             (200, 300, False, lambda d, s: (d, 0.5 * s))]                       # h1 + h2 > 360 but |dh'| <= 180: the plain mean
    for h1, h2, far, rule in rules:
        _, _, p = pair(polar(50, 30, h1), polar(50, 30, h2))
        g1, g2 = primed(h1), primed(h2)
        assert (abs(g1 - g2) > 180.0) == far, (h1, h2)
        dh, hm = rule(g2 - g1, g1 + g2)
        assert p["dh"] == pytest.approx(dh, abs=1e-9) and p["hm"] == pytest.approx(hm, abs=1e-9) and abs(p["dh"]) <= 180.0, (h1, h2)
        assert p["dH"] == pytest.approx(2.0 * math.sqrt(p["Cp1"] * p["Cp2"]) * math.sin(math.radians(0.5 * dh)), abs=1e-9)
    # C'1 C'2 = 0: dh' = 0 and the mean hue is the SUM, i.e. the other colour's hue
    _, e00, p = pair((50.0, 0.0, 0.0), polar(50, 30, 40))
    assert p["dh"] == 0.0 and p["dH"] == 0.0 and p["hm"] == p["h2"] and p["h1"] == 0.0
    assert e00 == pytest.approx(p["Cp2"] / p["SC"], rel=1e-14)
    # f's knee: continuous, and linear below it
    w = np.ones(3)
    k = ref.KNEE
    below, above = ref.lab(np.float32([[k * 0.999] * 3]), w), ref.lab(np.float32([[k * 1.001] * 3]), w)
    slope = 116.0 * 841.0 / 108.0                                                       # dL / dt below the knee, and the cube root's there: no jump, no kink
    assert float(above[0][0]) - float(below[0][0]) == pytest.approx(slope * 0.002 * k, rel=1e-3) and float(above[0][0]) == pytest.approx(8.0 + slope * 0.001 * k, abs=1e-5)
    t = float(np.float32(0.004))
    assert float(ref.lab(np.float32([[0.004] * 3]), w)[0][0]) == pytest.approx(116.0 * (t * 841.0 / 108.0 + 4.0 / 29.0) - 16.0, rel=1e-15)
    assert float(ref.lab(np.float32([[1.0, 1.0, 1.0]]), w)[0][0]) == 100.0


def test_sharma_pairs():
    """three pairs of the published test data of Sharma, Wu and Dalal (2005), table 1, to the four decimals they print"""
    data = [((50.0, 2.6772, -79.7751), (50.0, 0.0, -82.7485), 2.0425), ((50.0, 2.5, 0.0), (50.0, 0.0, -2.5), 4.3065), ((50.0, 2.5, 0.0), (73.0, 25.0, -18.0), 27.1492),
            ((2.0776, 0.0795, -1.1350), (0.9033, -0.0636, -0.5514), 0.9082)]
    for l1, l2, want in data:
        assert pair(l1, l2)[1] == pytest.approx(want, abs=5e-5)


def test_against_colour_science_if_present():
    try:
        import colour
    except ImportError:
        return                                                                         # not required: the closed forms and the published pairs stand alone
    rng = np.random.default_rng(3)
    l1 = np.stack([rng.uniform(0, 100, 500), rng.uniform(-60, 60, 500), rng.uniform(-60, 60, 500)], axis=-1)
    l2 = l1 + rng.uniform(-8, 8, l1.shape)
    ours = ref.delta_e_00(tuple(l1.T), tuple(l2.T))
    assert np.allclose(ours, colour.delta_E(l1, l2, method="CIE 2000"), rtol=1e-9, atol=1e-9)


# ---- 2. the host library ------------------------------------------------------------------------------------------------------------------------------------

def test_develop_white():
    bins, lmin, lstep = 16, 380.0, 100.0
    w = R.develop_weights(bins, lmin, lstep)
    got = R.develop_white(w, lmin, lstep)
    assert np.array_equal(got, ref.develop_white(w, 1.0))                              # equal energy: the rows' sums, ascending
    assert got[0] / got.sum() == pytest.approx(1.0 / 3.0, abs=2e-3) and got[1] / got.sum() == pytest.approx(1.0 / 3.0, abs=2e-3)
    # a tabulated illuminant: piecewise linear, so its mean over a bin is the trapezoid sum over the knots inside -- here a ramp, whose mean is its value at the centre
    ramp = (np.linspace(1.0, 3.0, 81).astype(np.float32), 380.0, 780.0)
    width = lstep / (bins // 4)
    centres = lmin + (np.arange(bins) + 0.5) * width
    means = 1.0 + (centres - 380.0) * (2.0 / 400.0)
    assert np.allclose(R.develop_white(w, lmin, lstep, ramp), ref.develop_white(w, means), rtol=1e-12)
    with pytest.raises(ValueError):
        R.develop_white(w[:2], lmin, lstep)


def region_arrays(shape=(42, 23), regions=3, t=cases.THRESHOLDS):
    de = cases.reference(shape)[0].astype(np.float32)
    return de, ref.regions_walk(de, cases.labels(shape, regions), regions, t)


def test_derive_and_csv(tmp_path):
    _, sums = region_arrays()
    got, want = R.delta_e_derive(*sums), ref.derive(*sums)
    assert sums[4].any() and not sums[3][2].any()                                      # non-finite pixels are in; region 2 is empty
    for k in R.DELTA_E_FIGURES:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.isnan(got["mean"][2]).all() and np.isnan(got["coverage"][2]).all() and (got["max"][2] == 0.0).all()
    path = tmp_path / "de.csv"
    R.save_delta_e_csv(str(path), *sums)
    lines = path.read_text().splitlines()
    assert lines[0] == "region,metric,mean,rms,max,exceed,coverage,finite,nonfinite" and len(lines) == 1 + 3 * 2
    for n, line in enumerate(lines[1:]):
        r, k = divmod(n, 2)
        f = line.split(",")
        assert f[0] == str(r) and f[1] == ("ab", "00")[k] and int(f[7]) == sums[3][r, k] and int(f[8]) == sums[4][r, k]
        for col, name in zip(f[2:7], R.DELTA_E_FIGURES):
            assert (col == "nan" and np.isnan(want[name][r, k])) or float(col) == want[name][r, k], (line, name)
    with pytest.raises(ValueError):
        R.delta_e_derive(*[s[:, :1] for s in sums])


def test_symbols_are_declared():
    for lib, names in ((_capi.HIP_SYMBOLS, ("ssx_delta_e_images", "ssx_spectral_delta_e")), (_capi.HOST_SYMBOLS, ("ssh_develop_white", "ssh_delta_e_derive", "ssh_delta_e_save_csv"))):
        for n in names:
            assert n in lib
    host = _capi.host_lib()
    assert all(hasattr(host, n) for n in ("ssh_develop_white", "ssh_delta_e_derive", "ssh_delta_e_save_csv"))


def run_cli(*args):
    return subprocess.run([CLI, "-s=cornell", "-w=8", "-h=8", "-spp=2", "-o=/dev/null"] + list(args), cwd=ROOT, capture_output=True, text=True)


def test_cli_refusals(tmp_path):
    """what the CLI refuses when it checks its options, before anything renders: no GPU is touched"""
    sbuild.build_host()
    npy, csv = str(tmp_path / "de.npy"), str(tmp_path / "de.csv")
    both = ["--delta-e-output=" + npy, "--delta-e-csv=" + csv]
    for out in (both[:1], both[1:], both):
        p = run_cli(*out)
        assert p.returncode != 0 and "need `--spectral-bins=<n>`" in p.stderr, p.stderr
        for flag in ("--rgb", "--tile-major", "--libm=glibc-2.35"):
            p = run_cli("--spectral-bins=8", flag, *out)
            assert p.returncode != 0 and "cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`" in p.stderr, (flag, p.stderr)
    for side in ("--delta-e-observer=2006", "--delta-e-filter=" + D65, "--delta-e-relight=" + D65, "--delta-e-denoise", "--delta-e-threshold=2,1", "--delta-e-white-y=1"):
        p = run_cli("--spectral-bins=8", side)
        assert p.returncode != 0 and "need `--delta-e-output=<file.npy>` or `--delta-e-csv=<file.csv>`" in p.stderr, (side, p.stderr)
    for bad, word in (("--delta-e-observer=1964", "--delta-e-observer (1931|2006)"), ("--delta-e-threshold=2", "--delta-e-threshold"), ("--delta-e-threshold=-1,1", "--delta-e-threshold"),
                      ("--delta-e-threshold=1,nan", "--delta-e-threshold"), ("--delta-e-white-y=0", "--delta-e-white-y"), ("--delta-e-white-y=inf", "--delta-e-white-y"),
                      ("--delta-e-denoise=3", "does not take a value")):
        p = run_cli("--spectral-bins=8", bad, *both)
        assert p.returncode != 0 and word in p.stderr, (bad, p.stderr)
    assert not os.path.exists(npy) and not os.path.exists(csv)


# ---- 3. the inputs discriminate ---------------------------------------------------------------------------------------------------------------------------------

def differs(x, y):
    return any(not np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(x, y))


def test_the_inputs_discriminate():
    shape, regions = (42, 23), 3
    de = cases.reference(shape)[0].astype(np.float32)
    lab = cases.labels(shape, regions)
    inside = de[..., 0][(lab == 0) & np.isfinite(de[..., 0])]
    t = (float(np.sort(inside)[inside.size // 2]), float(de[..., 1][lab == 1][0]))     # thresholds that pixels of the map hit exactly: > against >=
    right = ref.regions_walk(de, lab, regions, t)
    assert not differs(right, ref.regions_walk(de, lab, regions, t))
    assert differs(right[:2], ref.regions_walk(de, lab, regions, t, order="columns")[:2])          # another order of additions
    assert differs(right[5:], ref.regions_walk(de, lab, regions, t, strict=False)[5:])             # a non-strict comparison
    assert differs(right[1:2], ref.regions_walk(de, lab, regions, t, square="float")[1:2])         # the square rounded to binary32
    assert differs(right[:2], ref.regions_walk(de, lab, regions, t, finite_only=False)[:2])        # a non-finite value let into SUM
    assert right[4].any() and right[3].min() == 0                                                    # non-finite pixels counted; an empty region


# ---- 4. the exclusion cap -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cases.SHAPES[1:])
def test_few_pairs_lie_near_a_branch_point(shape):
    de, _, guard, db, lb = cases.reference(shape)
    assert guard.mean() < 0.02, guard.mean()
    ok = ~guard & np.isfinite(de).all(axis=-1)
    assert np.isfinite(db[ok]).all() and np.isfinite(lb[ok]).all()
    ulp32 = np.spacing(np.abs(de[ok]).astype(np.float32)).astype(np.float64)
    assert np.median(db[ok] / ulp32) < 1.1                                              # the bound is binary32's resolution, not a licence
