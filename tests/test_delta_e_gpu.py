"""The colour difference of two developments on the GPU (include/ssx.h "Colour difference of two developments"), held to its two classes of guarantee.

SAME BITS: the six region arrays equal the numpy ordered walk (tests/delta_e_ref.py regions_walk) over the map the same call returned, as integer views; the state
entry gives the bits of the pure entry on ssx_spectral_develop's two outputs.

WITHIN A BOUND: de and lab against the binary64 restatement.  The bound is derived, not fitted (delta_e_ref.bounds):
  * ROCm ships no table of the ulp errors of its binary64 device functions on this installation, so 4 ulp per call of cbrt, atan2, sin, cos and exp is an
    ASSUMPTION; numpy's own functions add 1 ulp: T = 5 ulp of the result per call.  + - * / and sqrt are correctly rounded on both sides: half an ulp each.
  * Every operation of the formula propagates its operands' bounds by its partial derivatives (|d(xy)| <= |x| dy + |y| dx, |d atan2(y, x)| <= (|x| dy + |y| dx)
    / (x^2 + y^2), |d cbrt(t)| = cbrt(t) / (3 t) dt, |d sin|, |d cos| <= 1, d exp = exp, |d sqrt(a)| <= min(da / sqrt(a), sqrt(da))) and adds its own error, at the
    pixel's own values -- the input box is x, y, z in [0.004, 1.7] times the white, plus the planted pairs.  The first-order total is doubled for the second order.
  * One binary32 ulp of the value is added for the final rounding.
  Over the box this is 1.0 to 1.1 binary32 ulp of the value for most pixels (the binary64 part is some 1e4 * 2^-52 = 2e-12 for Lab): the test asks for binary32's
  resolution.  Pairs within 1 degree of a branch point of CIEDE2000 (delta_e_ref.hue_guard; fewer than 2 % -- tests/test_delta_e_cpu.py) are compared for their
  non-finite pattern only.  The largest |difference| / bound observed is printed; profiles/r23/NOTES.md records it."""
import numpy as np
import pytest

import delta_e_cases as cases
import delta_e_ref as ref
import test_spectral_gpu as base
import test_spectral_stats_gpu as stats
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import develop_weights, delta_e_derive

pytestmark = pytest.mark.gpu
same, refused, start = stats.same, base.refused, base.start
NAMES = ("SUM", "SSQ", "MAX", "NF", "NX", "EX")
SW, SH = 42, 23                                        # the state entry's image


def pure():
    return base.renderer("cornell-srgb")               # a context that has rendered nothing: the pure entry needs no state


def assert_walk(sums, de, labels, R, t, what=""):
    want = ref.regions_walk(de, labels, R, t)
    for name, g, w in zip(NAMES, sums, want):
        assert same(g, w), name + what


def within(got, want, bound, keep):
    """the largest |got - want| / bound over the finite kept values; the non-finite pattern must match exactly everywhere"""
    got64 = got.astype(np.float64)
    assert np.array_equal(np.isnan(got64), np.isnan(want)) and np.array_equal(np.isposinf(got64), np.isposinf(want)) and np.array_equal(np.isneginf(got64), np.isneginf(want))
    ok = keep & np.isfinite(want)
    return float((np.abs(got64[ok] - want[ok]) / bound[ok]).max()) if ok.any() else 0.0


# ---- 1. the pure entry on synthetic XYZ ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regions,how", [(1, "NULL"), (1, "labelled"), (3, "last empty"), (32, "last empty"), (32, "all occupied")])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_pure_entry(shape, regions, how):
    a, b, wa, wb = cases.images(shape)
    de64, lab64, guard, de_bound, lab_bound = cases.reference(shape)
    labels = None if how == "NULL" else cases.labels(shape, regions, full=how == "all occupied")
    r = pure()
    first = r.delta_e_images(a, b, wa, wb, labels, regions, cases.THRESHOLDS, lab=True)[1]
    t = (float(first[0, 0, 0]), cases.THRESHOLDS[1]) if np.isfinite(first[0, 0, 0]) else cases.THRESHOLDS      # a threshold that a pixel hits exactly: > against >=
    sums, de, lab = r.delta_e_images(a, b, wa, wb, labels, regions, t, lab=True)
    assert same(de, first)
    assert_walk(sums, de, labels, regions, t)                                                                  # (a) the same bits
    keep = ~guard
    worst = (within(lab, lab64, lab_bound, np.repeat(keep[..., None], 6, axis=-1)), within(de[..., 0], de64[..., 0], de_bound[..., 0], np.ones_like(keep)),
             within(de[..., 1], de64[..., 1], de_bound[..., 1], keep))
    print("delta_e %dx%d R=%d: largest |difference| / bound: lab %.3f, dE*ab %.3f, dE00 %.3f" % (shape + (regions,) + worst))
    assert max(worst) <= 1.0, worst                                                                            # (b) within the bound
    none = r.delta_e_images(a, b, wa, wb, labels, regions, t, maps=False, lab=False)                           # (c) the maps are optional
    assert none[1] is None and none[2] is None
    for name, g, w in zip(NAMES, none[0], sums):
        assert same(g, w), name + " (no maps)"
    if how == "all occupied" and shape[0] * shape[1] >= 512:
        assert (sums[3] + sums[4]).all()                                                                        # every one of the 32 regions holds pixels
    if how == "labelled" and shape[0] * shape[1] >= 64:
        assert 0 < (sums[3] + sums[4])[0, 0] < shape[0] * shape[1]                                              # R = 1 with labels: the 255s are left out
    if how == "last empty" and shape[0] * shape[1] >= 64:
        assert not sums[3][regions - 1].any() and (sums[2][regions - 1] == 0).all()                          # the region without a pixel
        assert sums[4].sum() > 0                                                                                # non-finite pixels were counted
    fig = delta_e_derive(*sums)
    d = ref.derive(*sums)
    for k in d:
        assert same(fig[k], d[k]), k


def test_equal_sides_give_zero():
    a, _, wa, _ = cases.images((42, 23))
    sums, de, _ = pure().delta_e_images(a, a, wa, wa, None, 1, (0.0, 0.0))
    fin = np.isfinite(de)
    assert (de[fin] == 0.0).all() and not sums[5].any() and not sums[0].any() and sums[4][0, 0] == (~fin[..., 0]).sum()


# ---- 3. the state entry -----------------------------------------------------------------------------------------------------------------------------------------

def state_renderer(scene, bins, **opts):
    r = Renderer(Options(scene_name=scene, res=(SW, SH), seed=base.SEED, texture=base.TEX, **opts))
    r.set_spectral_bins(bins)
    r.set_noise_estimate(True)                         # the filter of the denoised source is guided by its variance
    return r


def two_weights(r, bins):
    c = r.scene.desc.contents
    return develop_weights(bins, c.lambda_min, c.lambda_step, observer=1931), develop_weights(bins, c.lambda_min, c.lambda_step, observer=2006)


def state_labels():
    rng = np.random.default_rng(9)
    return np.array([0, 1, 2, 255], dtype=np.uint8)[rng.integers(0, 4, (SH, SW))]


@pytest.mark.parametrize("bins", [16, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_state_entry_equals_the_pure_entry_on_two_developments(scene, bins):
    r = state_renderer(scene, bins)
    start(r, 37, spp_per_launch=16)
    w31, w06 = two_weights(r, bins)
    labels, t, dn = state_labels(), cases.THRESHOLDS, {}
    raw31, raw06, den06, den31 = r.develop(w31), r.develop(w06), r.develop(w06, denoise=dn), r.develop(w31, denoise=dn)
    Y = raw31[..., 1]
    white = cases.WHITE_A * (float(Y[np.isfinite(Y)].mean()) / 0.18)
    p = pure()
    for what, (wa, wb, flags, xa, xb) in {"raw/raw": (w31, w06, (False, False), raw31, raw06), "raw/denoised": (w31, w06, (False, True), raw31, den06),
                                          "denoised/denoised": (w31, w06, (True, True), den31, den06)}.items():
        got = r.delta_e_raw(wa, wb, white, white, labels, 4, t, denoise=dn if any(flags) else None, denoised=flags, lab=True)
        want = p.delta_e_images(xa, xb, white, white, labels, 4, t, lab=True)
        for name, g, w in zip(NAMES, got[0], want[0]):
            assert same(g, w), name + " " + what
        assert same(got[1], want[1]) and same(got[2], want[2]), what
        assert_walk(got[0], got[1], labels, 4, t, " " + what)
    assert got[0][0][0, 1] > 0.0                                                                               # two observers do differ
    sums, de, _ = r.delta_e_raw(w31, w31, white, white, labels, 4, t)                                          # one development twice: nothing differs
    assert not de.any() and not sums[5].any() and not sums[0].any()


def test_a_delta_e_changes_nothing_a_continue_builds_on():
    scene, bins = "cornell-srgb", 16
    r, never = state_renderer(scene, bins), state_renderer(scene, bins)
    for x in (r, never):
        start(x, 16, spp_per_launch=8)                  # two launches: the filter's variance needs two batches
    w31, w06 = two_weights(r, bins)
    r.delta_e_raw(w31, w06, cases.WHITE_A, cases.WHITE_A, None, 1, denoise={}, denoised=(False, True))
    for x in (r, never):
        x.render_continue(21); x.render_wait()
    assert same(r.xyza, never.xyza)
    for g, w in zip(r.spectral_read(sums=True)[1:], never.spectral_read(sums=True)[1:]):
        assert same(g, w)


@pytest.mark.parametrize("ranks", [2, 3])
def test_owner_mask(ranks):
    scene, bins = "cornell-srgb", 16
    whole = state_renderer(scene, bins)
    start(whole, 37, spp_per_launch=16)
    w31, w06 = two_weights(whole, bins)
    labels = state_labels()
    one = whole.delta_e_raw(w31, w06, cases.WHITE_A, cases.WHITE_A, labels, 4, lab=True)
    de, lab = np.zeros_like(one[1]), np.zeros_like(one[2])
    counted = np.zeros((4, 2), dtype=np.uint64)
    for first in range(ranks):
        r = state_renderer(scene, bins, tile_first=first, tile_stride=ranks, tile_skew=1)
        start(r, 37, spp_per_launch=16)
        mask = tile_owner_mask(SW, SH, first, ranks, 1)
        sums, d, l = r.delta_e_raw(w31, w06, cases.WHITE_A, cases.WHITE_A, labels, 4, lab=True)
        assert not d[~mask].any() and not l[~mask].any() and not np.signbit(d[~mask]).any()                   # foreign pixels read +0
        assert_walk(sums, d, np.where(mask, labels, 255).astype(np.uint8), 4, cases.THRESHOLDS)              # and belong to no region
        de[mask], lab[mask] = d[mask], l[mask]
        counted += sums[3] + sums[4]
    assert same(de, one[1]) and same(lab, one[2]) and np.array_equal(counted, one[0][3] + one[0][4])          # several contexts' owned pixels are one context's
    # the several-device route: each side developed by its owners and merged by ownership, then the pure entry on one device -- the bits of one device
    xa, xb = np.zeros((SH, SW, 3), dtype=np.float32), np.zeros((SH, SW, 3), dtype=np.float32)
    for first in range(ranks):
        r = state_renderer(scene, bins, tile_first=first, tile_stride=ranks, tile_skew=1)
        start(r, 37, spp_per_launch=16)
        mask = tile_owner_mask(SW, SH, first, ranks, 1)
        xa[mask], xb[mask] = r.develop(w31)[mask], r.develop(w06)[mask]
    merged = pure().delta_e_images(xa, xb, cases.WHITE_A, cases.WHITE_A, labels, 4, lab=True)
    for name, g, w in zip(NAMES, merged[0], one[0]):
        assert same(g, w), name + " (merged by ownership)"
    assert same(merged[1], one[1]) and same(merged[2], one[2])


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    a, b, wa, wb = cases.images((42, 23))
    r, lib, ARG, STATE = pure(), _capi.hip_lib(), _capi.SSX_ERR_ARG, _capi.SSX_ERR_STATE
    labels = cases.labels((42, 23), 3)
    refused(lambda: r.delta_e_images(a, b, wa, wb, labels, 0), ARG, "regions")
    refused(lambda: r.delta_e_images(a, b, wa, wb, labels, 33), ARG, "regions")
    refused(lambda: r.delta_e_images(a, b, wa, wb, None, 2), ARG, "regions")
    refused(lambda: r.delta_e_images(a, b, wa, wb, labels, 1), ARG, "labels[")                                 # a label that is neither a region nor 255
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(lambda: r.delta_e_images(a, b, wa * [1, bad, 1] if np.isfinite(bad) else np.array([wa[0], bad, wa[2]]), wb), ARG, "white_a[1]")
        refused(lambda: r.delta_e_images(a, b, wa, np.array([wb[0], wb[1], bad])), ARG, "white_b[2]")
    for bad in (-0.5, np.inf, np.nan):
        refused(lambda: r.delta_e_images(a, b, wa, wb, thresholds=(1.0, bad)), ARG, "t[1]")
    empty = np.zeros((0, 4, 3), dtype=np.float32)
    refused(lambda: r.delta_e_images(empty, empty, wa, wb), ARG)
    out = [np.zeros((1, 2), dtype=d) for d in (np.float64, np.float64, np.float32, np.uint64, np.uint64, np.uint64)]
    t = np.array(cases.THRESHOLDS)
    full = [r._ctx, 42, 23, a.ctypes.data, b.ctypes.data, wa.ctypes.data, wb.ctypes.data, None, 1, t.ctypes.data, None, None] + [o.ctypes.data for o in out]
    for at, word in ((3, "xyz_a"), (4, "xyz_b"), (5, "white_a"), (6, "white_b"), (9, "t must"), (12, "SUM"), (15, "NF"), (17, "EX")):
        args = list(full); args[at] = None
        refused(lambda: r._check(lib.ssx_delta_e_images(*args)), ARG, word)
    huge = list(full); huge[1], huge[2] = 1 << 15, 1 << 14                                                   # 2^29 pixels: too large (nothing is read before the refusal)
    refused(lambda: r._check(lib.ssx_delta_e_images(*huge)), ARG)
    # the state entry: ssx_spectral_develop's reasons, and its own arguments
    w = np.zeros((3, 16), dtype=np.float32)
    refused(lambda: r.delta_e_raw(w, w, wa, wb), STATE, "spectral output is off")
    s = state_renderer("cornell-srgb", 16)
    refused(lambda: s.delta_e_raw(w, w, wa, wb), STATE, "no spectral bins")
    # ("no sample has been accumulated yet", ssx_done_spp == 0 with valid bins, is not tested: no public route brings a context into that state, and the line is
    # develop_state_ready's, shared with ssx_spectral_develop)
    start(s, 4)
    state = [s._ctx, None, 0, 0, w.ctypes.data, w.ctypes.data, wa.ctypes.data, wb.ctypes.data, None, 1, t.ctypes.data, None, None] + [o.ctypes.data for o in out]
    for at, word in ((4, "weights_a"), (5, "weights_b"), (6, "white_a"), (7, "white_b"), (10, "t must"), (13, "SUM"), (18, "EX")):
        args = list(state); args[at] = None
        refused(lambda: s._check(lib.ssx_spectral_delta_e(*args)), ARG, word)
    refused(lambda: s.delta_e_raw(w, w, wa, wb, denoise={}, denoised=(True, True)), STATE, "batch")             # one launch so far: the filter's variance needs two
    quiet = Renderer(Options(scene_name="cornell-srgb", res=(SW, SH), seed=base.SEED, texture=base.TEX))
    quiet.set_spectral_bins(16)
    start(quiet, 8, spp_per_launch=4)
    refused(lambda: quiet.delta_e_raw(w, w, wa, wb, denoise={}, denoised=(False, True)), STATE, "noise estimate is off")
    quiet.delta_e_raw(w, w, wa, wb)                                                                             # (the raw sides need none of it)
    part = state_renderer("cornell-srgb", 16, tile_first=0, tile_stride=2)
    start(part, 8, spp_per_launch=4)
    refused(lambda: part.delta_e_raw(w, w, wa, wb, denoise={}, denoised=(True, False)), STATE)                  # a share of the image cannot be filtered
    refused(lambda: s.delta_e_raw(w, w, wa, wb, denoised=(True, False)), ARG, "denoise must not be NULL")
    refused(lambda: s.delta_e_raw(w, w, wa, wb, denoised=(False, True)), ARG, "denoised_b")
    refused(lambda: s.delta_e_raw(w, w, wa, wb, labels=np.full((SH, SW), 7, dtype=np.uint8), regions=3), ARG, "labels[")
    refused(lambda: s.delta_e_raw(w, w, -wa, wb), ARG, "white_a[0]")
    with pytest.raises(ValueError):
        s.delta_e_raw(np.zeros((3, 8), dtype=np.float32), np.zeros((3, 8), dtype=np.float32), wa, wb)
    s._check(lib.ssx_render_continue(s._ctx, 1 << 16))                                  # while a render runs: both entries
    try:
        refused(lambda: s.delta_e_raw(w, w, wa, wb), STATE, "render in progress")
        refused(lambda: s.delta_e_images(a, b, wa, wb), STATE, "render in progress")
    finally:
        lib.ssx_render_stop(s._ctx)
        s.render_wait()


# ---- 5. the CLI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_one_device_two_devices_and_the_python_mirror(tmp_path):
    """--delta-e-*: one device (ssx_spectral_delta_e) and --gpus=2 on one card (each side through the develop's route, then ssx_delta_e_images on device 0) write the
    same .npy and .csv bytes; the CSV and the map are what Python gets with the hosts' default-white policy restated here."""
    import os
    import subprocess
    from simple_spectral_amd.renderer import develop_white, emitter_spectrum, save_delta_e_csv
    W, H = base.W, base.H
    common = [base.CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "--seed=%d" % base.SEED, "--texture=data/scenes/test-img.png", "-o=" + str(tmp_path / "o.pfm"),
              "--spectral-bins=8", "--probe=2,1,9,7", "--probe=10,0,20,12"]
    sides = {"observers": ["--delta-e-observer=2006"],
             "denoised": ["--delta-e-denoise", "--delta-e-white-y=1.5", "--delta-e-threshold=1.5,0.5"]}
    got = {}
    for name, extra in sides.items():
        for n, (more, env) in enumerate((([], {}), (["--gpus=2"], {"SSX_TEST_ONE_GPU": "1"}))):
            npy, csv = str(tmp_path / ("%s%d.npy" % (name, n))), str(tmp_path / ("%s%d.csv" % (name, n)))
            p = subprocess.run(common + extra + more + ["--delta-e-output=" + npy, "--delta-e-csv=" + csv], cwd=base.ROOT, capture_output=True, text=True, env=dict(os.environ, **env))
            assert p.returncode == 0 and "Colour difference, region 1" in p.stderr, p.stderr
            got[name, n] = (open(npy, "rb").read(), open(csv, "rb").read())
        assert got[name, 0] == got[name, 1], name
    assert got["observers", 0] != got["denoised", 0]
    # the mirror of "observers": 1931 against 2006, both raw; whites from the scene's emitter spectrum, scaled so that side A's mean finite Y is 0.18 of its white's
    r = base.renderer("cornell-srgb")
    r.set_spectral_bins(8)
    start(r, 16)
    d = r.scene.desc.contents
    w31, w06 = (develop_weights(8, d.lambda_min, d.lambda_step, observer=o) for o in (1931, 2006))
    e = d.spectra[emitter_spectrum(r.scene.desc)]
    emitter = (np.array(d.samples[e.offset:e.offset + e.n], dtype=np.float32), e.low, e.high)
    white_a, white_b = develop_white(w31, d.lambda_min, d.lambda_step, emitter), develop_white(w06, d.lambda_min, d.lambda_step, emitter)
    total, n = 0.0, 0
    for y in r.develop(w31)[..., 1].ravel():                                                                    # the host's own loop: ascending, binary64
        if np.isfinite(y):
            total, n = total + float(y), n + 1
    scale = ((total / n) / 0.18) / white_a[1]
    labels = np.full((H, W), 255, dtype=np.uint8)
    labels[1:7, 2:9], labels[0:12, 10:20] = 0, 1
    sums, de, _ = r.delta_e_raw(w31, w06, white_a * scale, white_b * scale, labels, 2)
    mirror = str(tmp_path / "mirror.csv")
    save_delta_e_csv(mirror, *sums)
    assert open(mirror, "rb").read() == got["observers", 0][1]
    assert same(np.load(str(tmp_path / "observers0.npy")), de) and sums[0][0, 1] > 0.0
