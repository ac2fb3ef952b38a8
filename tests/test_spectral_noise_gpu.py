"""The spectral noise figure on the GPU (include/ssx.h "Spectral noise figure"): the tile partials and totals of the device against the sequential numpy restatement
(tests/spectral_noise_ref.py), bit for bit, and the masks, invariances, state rules, kernel variants and stopping rule around them.  The harness is
tests/test_spectral_stats_gpu.py's: 20 x 12 images (ragged tiles in both directions), seed 5, 37 spp in launches of 16 / 16 / 5, the per-sample fluxes from
ssx_debug_sample_flux -- computed once there and shared."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import spectral_noise_ref as ref
import spectral_stats_ref as stats_ref
import test_spectral_gpu as base
import test_spectral_stats_gpu as stats
from simple_spectral_amd import _capi
from simple_spectral_amd.renderer import spectral_noise_derive

pytestmark = pytest.mark.gpu
W, H, SEED, SPP = base.W, base.H, base.SEED, 37
renderer, start, refused, same, moments_renderer = base.renderer, base.start, base.refused, stats.same, stats.moments_renderer
NAMES = ("EV", "EM", "PP", "PU")
OWNERS = [(0, 2, 1), (1, 2, 1)]


@functools.lru_cache(maxsize=None)
def masks():
    """None; a mask that crosses tile boundaries in both directions and reaches the ragged right and top edges (with one stray pixel, any nonzero value counts); a
    single pixel; nothing."""
    crossing = np.zeros((H, W), dtype=np.uint8); crossing[5:12, 6:20] = 1; crossing[2, 1] = 200
    one = np.zeros((H, W), dtype=np.uint8); one[9, 17] = 1
    out = {"none": None, "crossing": crossing, "one": one, "empty": np.zeros((H, W), dtype=np.uint8)}
    for m in out.values():
        if m is not None:
            m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(scene, bins, mask="none", owner=None):
    """(partials, totals) of the 37 samples; computed once, read-only"""
    S, Q, N, _ = stats.restated(scene, bins)
    part = ref.tile_partials(S, Q, N, masks()[mask], owner)
    tot = ref.totals(*part)
    for a in part + tot:
        a.setflags(write=False)
    return part, tot


def check(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), what + name


# ---- 1. partials and totals, bit for bit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [4, 8, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_partials_and_totals_equal_the_sequential_restatement(scene, bins):
    r = moments_renderer(scene, bins)
    start(r, SPP, spp_per_launch=16)                       # launches of 16 / 16 / 5
    part, tot = restated(scene, bins)
    assert (tot[3] > 0).any() == (bins == 64) and (bins != 64 or (tot[3] > 0).all())    # 64 bins: the unestimated path runs in every bin; 4 and 8 bins: it does not
    got_tot, got_part = r.spectral_noise_raw()
    check(got_part, part, "tile ")
    check(got_tot, tot)
    assert got_part[0].shape == (6, bins) and (got_part[2] + got_part[3] == np.array([64, 64, 32, 32, 32, 16], dtype=np.uint32)[:, None]).all()
    noise, coverage, totals = r.spectral_noise()
    want_noise, want_coverage, want_rel = ref.derive(*tot)
    assert noise == want_noise and coverage == want_coverage and math.isfinite(noise) and noise > 0 and (coverage == 1.0) == (bins != 64)
    check(totals, tot)
    assert same(spectral_noise_derive(*got_tot)[2], want_rel)
    S, Q, N, _ = stats.restated(scene, bins)               # the state beside it is what it was
    _, _, counts, sums = r.spectral_read(sums=True)
    assert same(sums, S) and np.array_equal(counts, N) and same(r.spectral_variance(q=True)[2], Q)


# ---- 2. masks ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [8, 64])
def test_masks(bins):
    scene = "cornell-srgb"
    r = moments_renderer(scene, bins)
    start(r, SPP, spp_per_launch=16)
    for name, mask in masks().items():
        part, tot = restated(scene, bins, name)
        got_tot, got_part = r.spectral_noise_raw(mask)
        check(got_part, part, name + ": tile ")
        check(got_tot, tot, name + ": ")
        in_mask = H * W if mask is None else int((mask != 0).sum())
        assert (got_tot[2] + got_tot[3] == in_mask).all()
    noise, coverage, totals = r.spectral_noise(masks()["empty"])
    assert math.isnan(noise) and math.isnan(coverage) and not totals[0].any() and not totals[2].any()
    S, Q, N, _ = stats.restated(scene, bins)
    e, mu, est = ref.per_pixel(S, Q, N)
    _, _, (EV, EM, PP, PU) = r.spectral_noise(masks()["one"])                         # the one-pixel mask: the pixel itself
    assert same(EV, np.where(est[9, 17], e[9, 17], 0.0)) and same(EM, np.where(est[9, 17], mu[9, 17], 0.0) + 0.0) and np.array_equal(PP, est[9, 17].astype(np.uint64))
    with pytest.raises(ValueError):
        r.spectral_noise(np.zeros((W, H), dtype=np.uint8))
    refused(lambda: r._check(r._lib.ssx_spectral_noise(r._ctx, None, None, None, None, None, None, None, None, None)), _capi.SSX_ERR_ARG, "must not be NULL")


# ---- 3. invariances ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [8, 64])
def test_two_contexts_merged_by_ownership_equal_one(bins):
    scene = "cornell-srgb"
    whole_part, whole_tot = restated(scene, bins, "crossing")
    parts = []
    for owner in OWNERS:
        r = moments_renderer(scene, bins, tile_first=owner[0], tile_stride=owner[1], tile_skew=owner[2])
        start(r, SPP, spp_per_launch=16)
        got_tot, got_part = r.spectral_noise_raw(masks()["crossing"])
        part, tot = restated(scene, bins, "crossing", owner)                          # foreign tiles: +0.0 and 0
        check(got_part, part, "%r: tile " % (owner,))
        check(got_tot, tot, "%r: " % (owner,))
        parts.append(got_part)
    merged = ref.merge_owned(parts, W, H, OWNERS)
    check(merged, whole_part, "merged: tile ")
    pure = renderer(scene).spectral_noise_reduce(*merged)                             # a context that has rendered nothing: the pure call needs no state
    check(pure, whole_tot, "ssx_spectral_noise_reduce: ")
    one = moments_renderer(scene, bins)
    start(one, SPP, spp_per_launch=16)
    check(one.spectral_noise_raw(masks()["crossing"])[0], pure, "one context: ")
    r = renderer(scene)
    refused(lambda: r.spectral_noise_reduce(np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6))), _capi.SSX_ERR_ARG, "6 bins")
    refused(lambda: r.spectral_noise_reduce(*(np.zeros((0, 8)),) * 4), _capi.SSX_ERR_ARG, "0 tiles")


def test_start_plus_continue_equals_one_render():
    r = moments_renderer("cornell-srgb", 8)
    start(r, 16)
    r.render_continue(21); r.render_wait()
    part, tot = restated("cornell-srgb", 8)
    got_tot, got_part = r.spectral_noise_raw()
    assert r.done_spp() == SPP
    check(got_part, part, "tile "); check(got_tot, tot)


# ---- 4. the stop ----------------------------------------------------------------------------------------------------------------------------------------------

STEP, MAX_SPP, BINS, CHECK = 4, 36, 8, 3                   # nine checks; the target is the figure at the fourth (index 3)


@functools.lru_cache(maxsize=None)
def restated_checks(mask="none"):
    """[(noise, coverage, totals)] after 4, 8, ..., 36 samples: the samples of a pixel have independent streams, so the first k of the 37 are a render of k"""
    flux, lam, _ = base.per_sample("cornell-srgb", SPP)
    out = []
    for k in range(STEP, MAX_SPP + 1, STEP):
        S, Q, N = stats_ref.restate_sums(flux[:, :, :k], lam[:, :, :k], *base.lambda_range("cornell-srgb"), BINS)
        tot = ref.totals(*ref.tile_partials(S, Q, N, masks()[mask]))
        out.append(ref.derive(*tot)[:2] + (tot,))
    return out


def expected_stop(mask, min_coverage):
    checks = restated_checks(mask)
    target = checks[CHECK][0]
    stop = next(k for k, (noise, coverage, _) in enumerate(checks) if noise <= target and coverage >= min_coverage)
    print("restated checks", [(c[0], c[1]) for c in checks], "target", target, "stop at check", stop)
    assert 0 < stop < len(checks) - 1                      # neither the first check nor the cap: the rule decides, and it decides after more than one step
    return target, stop, checks[stop]


@pytest.mark.parametrize("mask", ["none", "crossing"])
def test_render_until_spectral_stops_at_the_first_converged_check(mask):
    target, stop, (noise, coverage, tot) = expected_stop(mask, 0.99)
    r = renderer("cornell-srgb")
    r.set_spectral_bins(BINS)
    got = r.render_until_spectral(target, STEP, MAX_SPP, mask=masks()[mask])
    assert got == ((stop + 1) * STEP, noise, coverage)
    check(r.spectral_noise_raw(masks()[mask])[0], tot)
    # a coverage that is never reached, and a NaN target, run to the cap
    capped = r.render_until_spectral(target, STEP, 12, mask=masks()[mask], min_coverage=1.1)
    assert capped[0] == 12 and capped[1:] == restated_checks(mask)[2][:2]
    assert r.render_until_spectral(float("nan"), STEP, 8)[0] == 8
    r.set_spectral_bins(0)
    refused(lambda: r.render_until_spectral(target, STEP, MAX_SPP), _capi.SSX_ERR_STATE, "spectral output is off")


@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_stops_there_and_writes_the_figure(tmp_path, gpus):
    rects = [(6, 5, 20, 12), (1, 2, 2, 3)]                 # the "crossing" mask as a union of rectangles
    target, stop, (noise, coverage, tot) = expected_stop("crossing", 0.99)
    csv, png = str(tmp_path / "n.csv"), str(tmp_path / "o.png")
    cmd = [base.CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=1", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + png,
           "--spectral-bins=%d" % BINS, "--spectral-noise-target=%r" % target, "--max-samples=%d" % MAX_SPP, "--noise-step=%d" % STEP,
           "--spectral-noise-output=" + csv] + ["--spectral-noise-region=%d,%d,%d,%d" % q for q in rects]
    env = dict(os.environ)
    if gpus == 2:                                           # the several-device path on one device: tile partials merged by ownership, the pure reduction on device 0
        cmd.append("--gpus=2"); env["SSX_TEST_ONE_GPU"] = "1"
    p = subprocess.run(cmd, cwd=base.ROOT, capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr
    said = re.search(r"Spectral noise (\S+) \(coverage (\S+)\) after (\d+) samples per pixel \(target (\S+)\)\.", p.stderr)
    assert said, p.stderr
    assert int(said.group(3)) == (stop + 1) * STEP and said.group(1) == "%.6g" % noise and said.group(2) == "%.6g" % coverage and said.group(4) == "%.6g" % target
    EV, EM, PP, PU = tot
    _, _, rel = ref.derive(*tot)
    lines = open(csv).read().split("\n")
    assert lines[0] == "bin,wavelength,rel,EV,EM,estimable,unestimated" and len(lines) == 2 + BINS and lines[-1] == ""
    r = renderer("cornell-srgb"); r.set_spectral_bins(BINS); start(r, 1)
    centres = r.spectral_image()[2]
    for b, line in enumerate(lines[1:-1]):
        f = line.split(",")
        assert (int(f[0]), int(f[5]), int(f[6])) == (b, int(PP[b]), int(PU[b])) and np.float32(f[1]) == centres[b]
        assert float(f[2]) == rel[b] and float(f[3]) == EV[b] and float(f[4]) == EM[b]


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------------------------------

def test_state_rules():
    r = renderer("cornell-srgb")
    refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "ssx_spectral_noise: spectral output is off")
    r.set_spectral_bins(8)
    start(r, 8)
    refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "ssx_spectral_noise: spectral moments are off")
    r.set_spectral_moments(True)                            # switched on over existing bins: invalid
    refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "switched on after the render")
    start(r, SPP, spp_per_launch=16)
    check(r.spectral_noise_raw()[0], restated("cornell-srgb", 8)[1])
    # a changed bin count clears the state
    r.set_spectral_bins(16)
    refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "bin count")
    r.set_spectral_bins(8)
    refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "bin count")
    # after ssx_spectral_import the moments are invalid (a checkpoint does not carry Q)
    start(r, 16)
    info, sums, s2 = r.export_sums()
    sinfo, bsums, bcounts = r.export_spectral()
    r2 = moments_renderer("cornell-srgb", 8)
    r2.import_sums(info, sums, s2)
    r2.import_spectral(sinfo, bsums, bcounts)
    refused(r2.spectral_noise_raw, _capi.SSX_ERR_STATE, "ssx_spectral_import", "does not carry")
    # while a render runs
    r._check(r._lib.ssx_render_continue(r._ctx, 1 << 16))
    try:
        refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE, "render in progress")
        refused(lambda: r.spectral_noise_reduce(*restated("cornell-srgb", 8)[0]), _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop(); r.render_wait()
    r.spectral_noise_raw()                                  # the stopped render: the figure at the count it reached


# ---- 6. nothing else changes --------------------------------------------------------------------------------------------------------------------------------

def test_a_render_does_not_depend_on_the_figure_being_read():
    scene = "cornell-srgb"
    read = moments_renderer(scene, 8)
    start(read, 16)
    for more in (16, 5):
        read.spectral_noise_raw(masks()["crossing"]); read.spectral_noise_raw()
        read.render_continue(more); read.render_wait()
    read.spectral_noise_raw()
    S, Q, N, _ = stats.restated(scene, 8)
    _, _, counts, sums = read.spectral_read(sums=True)
    assert same(sums, S) and np.array_equal(counts, N) and same(read.spectral_variance(q=True)[2], Q)
    assert same(read.xyza, base.oracle(scene).render(W, H, SPP, seed=SEED))


# ---- 7. the run-time compiled kernel path -------------------------------------------------------------------------------------------------------------------

def test_run_time_compiled_kernel():
    r = renderer("custom", jit=True)
    assert r._lib.ssx_kernel_variant(r._ctx) == 3
    r.set_spectral_bins(8)
    r.set_spectral_moments(True)
    start(r, SPP, spp_per_launch=16)
    assert r.plan_info()["kernel"].startswith("ssx_render_kernel_jit")
    part, tot = restated("custom", 8)
    got_tot, got_part = r.spectral_noise_raw()
    check(got_part, part, "tile "); check(got_tot, tot)
