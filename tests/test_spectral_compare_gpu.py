"""Comparing two spectral renders on the GPU (include/ssx.h "Comparing two spectral renders"): the six region sums and the two maps against the sequential numpy
restatement (tests/spectral_compare_ref.py), bit for bit ("same" compares the integer views, a NaN equal to any NaN), the same bits by three routes, hand-made
arrays for the edge cases, the state rules and the CLI.  The harness is tests/test_spectral_gpu.py's: 20 x 12 images (ragged tiles in both directions); A is seed
5 at 37 spp in launches of 16 / 16 / 5, B is seed 6 at 21 spp -- rendered once per scene and bin count and shared."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import spectral_compare_ref as ref
import test_spectral_gpu as base
import test_spectral_stats_gpu as stats
from simple_spectral_amd import _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import compare_derive, compare_zmap, load_checkpoint_file_moments

pytestmark = pytest.mark.gpu
W, H, SPP_A, SPP_B, SEED_B = base.W, base.H, 37, 21, 6
renderer, start, refused, same = base.renderer, base.start, base.refused, stats.same
moments_renderer, probe_labels = stats.moments_renderer, stats.probe_labels
NAMES = ("DD", "VV", "X2", "CC", "NC", "EX")


def arrays_of(r):
    """(SsxSpectralInfo, S, Q, N) as the context exports them"""
    info, _, N, S = r.spectral_read(sums=True)
    return info, S, r.spectral_variance(q=True)[2], N


def render_a(scene, bins, **opts):
    r = moments_renderer(scene, bins, **opts)
    start(r, SPP_A, spp_per_launch=16)
    return r


@functools.lru_cache(maxsize=None)
def other(scene, bins):
    """B: (SsxSpectralInfo, S, N, Q) of seed 6 at 21 spp, in the order Renderer.compare_spectral_raw takes it; read-only"""
    r = moments_renderer(scene, bins)
    start(r, SPP_B, seed=SEED_B)
    info, S, Q, N = arrays_of(r)
    for a in (S, Q, N):
        a.setflags(write=False)
    return info, S, N, Q


def assert_same(got, want, what=""):
    (gs, gd, gv), (ws, wd, wv) = got, want
    for name, g, w in zip(NAMES, gs, ws):
        assert same(g, w), name + what
    assert same(gd, wd), "diff" + what
    assert same(gv, wv), "var" + what


def restated(A, Bset, labels, regions, t2):
    return ref.compare(*A, *Bset, labels, regions, t2), *ref.maps(*A, *Bset)


# ---- 1. bit for bit, and the same bits from the pure call ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [4, 8, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_compare_equals_the_restatement(scene, bins):
    r = render_a(scene, bins)
    _, SA, QA, NA = arrays_of(r)
    info, SB, NB, QB = other(scene, bins)
    assert info.done_spp == SPP_B and r.done_spp() == SPP_A
    labels = probe_labels()
    want = restated((SA, QA, NA), (SB, QB, NB), labels, 32, 9.0)
    NC, CC = want[0][4], want[0][3]
    assert NC.any() == (bins == 64) and CC[0].all()                      # 64 bins: cells that are not comparable; 4 bins: none
    assert not CC[2].any() and not NC[2].any() and (CC[1] + NC[1] == 1).all()          # the empty region; the one-pixel region
    got = r.compare_spectral_raw(other(scene, bins), labels, 32)
    assert_same(got, want)
    pure = renderer(scene).compare_arrays(SA, QA, NA, SB, QB, NB, labels, 32)            # a context that has rendered nothing: the pure call needs no state
    assert_same(pure, want, " (ssx_spectral_compare_arrays)")
    # two regions: at 64 bins the narrow instance of the row kernel over more than one chunk of the row (R * B <= 256)
    two = np.where(labels == 0, 0, np.where(labels == 255, 255, 1)).astype(np.uint8)
    assert_same(r.compare_spectral_raw(other(scene, bins), two, 2, threshold=1.5), restated((SA, QA, NA), (SB, QB, NB), two, 2, 2.25), " (two regions)")
    sums, diff, var = r.compare_spectral_raw(other(scene, bins), two, 2, maps=False)     # the maps are optional
    assert diff is None and var is None and same(sums[0], ref.compare(SA, QA, NA, SB, QB, NB, two, 2, 9.0)[0])
    fig = r.compare_spectral(other(scene, bins), labels, 32)
    d = ref.derive(*want[0])
    for k in d:
        assert same(fig[k], d[k]), k
    assert same(fig["zmap"], ref.zmap(want[1], want[2])) and np.array_equal(fig["comparable"], CC) and np.array_equal(fig["not_comparable"], NC)


# ---- 2. the same bits by other routes ----------------------------------------------------------------------------------------------------------------------

def test_two_contexts_merged_by_ownership_equal_one():
    scene, bins, labels = "cornell-srgb", 8, probe_labels()
    info, SB, NB, QB = other(scene, bins)
    one = render_a(scene, bins).compare_spectral_raw(other(scene, bins), labels, 32)
    S, Q, N = np.zeros_like(SB), np.zeros_like(QB), np.zeros_like(NB)
    for first in (0, 1):
        r = render_a(scene, bins, tile_first=first, tile_stride=2, tile_skew=1)
        _, s, q, n = arrays_of(r)
        mask = tile_owner_mask(W, H, first, 2, 1)
        S[mask], Q[mask], N[mask] = s[mask], q[mask], n[mask]
        own = r.compare_spectral_raw(other(scene, bins), np.zeros((H, W), dtype=np.uint8), 1)       # pixels the context does not own: count 0, not comparable
        assert (own[0][4][0] >= (~mask).sum()).all() and (own[2][~mask] == np.inf).all() and not own[1][~mask].any()
    assert_same(renderer(scene).compare_arrays(S, Q, N, SB, QB, NB, labels, 32), one)


def test_start_plus_continue_equals_one_render():
    scene, bins, labels = "cornell-srgb", 8, probe_labels()
    r = moments_renderer(scene, bins)
    start(r, 16)
    r.render_continue(21); r.render_wait()
    assert_same(r.compare_spectral_raw(other(scene, bins), labels, 32), render_a(scene, bins).compare_spectral_raw(other(scene, bins), labels, 32))


# ---- 3. hand-made arrays through the pure call ---------------------------------------------------------------------------------------------------------------

def hand_made(w, h, bins):
    """Two array sets with two samples in every sub-bin, all exact.  Bin b is of kind b % 4:
       0  black on both sides: S = Q = 0                                          v == 0, d == 0: z2 = +0.0, comparable
       1  constant fluxes 2 (A) and 4 (B): S = n c, Q = n c c                     v == 0, d = -2: z2 = +inf
       2  samples 3, 1 (A) and 7, 5 (B): mu = 2 and 6, e = 1 and 1                d = -4, v = 2: z2 = 8 exactly
       3  samples 3, 1 on both sides                                              d = 0, v = 2: z2 = 0"""
    M = bins // 4
    kinds = {0: ((0.0, 0.0), (0.0, 0.0)), 1: ((4.0, 8.0), (8.0, 32.0)), 2: ((4.0, 10.0), (12.0, 74.0)), 3: ((4.0, 10.0), (4.0, 10.0))}
    SA, QA, SB, QB = (np.zeros((h, w, bins)) for _ in range(4))
    for b in range(bins):
        (SA[..., b], QA[..., b]), (SB[..., b], QB[..., b]) = kinds[b % 4]
    NA, NB = np.full((h, w, M), 2, dtype=np.uint32), np.full((h, w, M), 2, dtype=np.uint32)
    return SA, QA, NA, SB, QB, NB


@pytest.mark.parametrize("regions", [1, 32])
@pytest.mark.parametrize("bins", [4, 16])                               # R * B = 4, 16, 128 (the narrow row kernel) and 512 (the wide one)
@pytest.mark.parametrize("w,h", [(1, 1), (9, 1), (1, 9), (17, 9)])
def test_hand_made_arrays(w, h, bins, regions):
    r = renderer("cornell-srgb")
    labels = (np.arange(w * h, dtype=np.uint8).reshape(h, w) % regions).astype(np.uint8)
    if w * h > 4:
        labels[h - 1, w - 1] = 255
    t2 = 8.0
    sets = hand_made(w, h, bins)
    (DD, VV, X2, CC, NC, EX), diff, var = got = r.compare_arrays(*sets, labels, regions, t2=t2)
    assert_same(got, restated(sets[:3], sets[3:], labels, regions, t2))
    px = np.array([(labels == k).sum() for k in range(regions)], dtype=np.uint64)[:, None]
    kind = np.arange(bins) % 4
    assert (CC == px).all() and not NC.any()
    assert not base.bits(X2[:, kind == 0]).any() and not base.bits(DD[:, kind == 0]).any()           # two black cells: z2 == +0.0, and they are comparable
    assert (X2[:, kind == 1][px[:, 0] > 0] == np.inf).all() and (EX[:, kind == 1] == px).all()       # v == 0 with d != 0: +inf, and it counts
    assert (X2[:, kind == 2] == 8.0 * px).all() and not EX[:, kind == 2].any()                       # z2 == t2 exactly: the comparison is strict
    below = r.compare_arrays(*sets, labels, regions, t2=np.nextafter(8.0, 0.0), maps=False)[0]
    assert (below[5][:, kind == 2] == px).all() and not below[5][:, kind == 3].any() and same(below[2], X2)
    assert (diff[..., kind == 2] == -4).all() and (var[..., kind == 2] == 2).all() and (var[..., kind == 1] == 0).all()
    # a NaN in S_A: DD and X2 of that region and bin only, and not in EX
    bad = [a.copy() for a in sets]
    bad[0][0, 0, 1] = np.nan
    (D2, V2, X22, C2, N2, E2), _, _ = r.compare_arrays(*bad, labels, regions, t2=t2)
    hit = np.zeros((regions, bins), dtype=bool); hit[labels[0, 0], 1] = True
    assert np.isnan(D2[hit]).all() and np.isnan(X22[hit]).all() and same(D2[~hit], DD[~hit]) and same(X22[~hit], X2[~hit])
    assert E2[hit][0] == EX[hit][0] - 1 and np.array_equal(E2[~hit], EX[~hit]) and np.array_equal(C2, CC)
    # nA < 2 alone, nB < 2 alone, both: not comparable, diff == 0 and var == +inf, in the first pixel's first sub-bin
    M = bins // 4
    for nA, nB in ((1, 2), (2, 0), (1, 1)):
        thin = [a.copy() for a in sets]
        thin[2][0, 0, 0], thin[5][0, 0, 0] = nA, nB
        got = r.compare_arrays(*thin, labels, regions, t2=t2)
        assert_same(got, restated(thin[:3], thin[3:], labels, regions, t2), " (thin %d, %d)" % (nA, nB))
        (_, _, _, C3, N3, _), d3, v3 = got
        cells = np.arange(bins) % M == 0
        assert (N3[labels[0, 0], cells] == 1).all() and N3.sum() == cells.sum() and (C3 + N3 == px).all()
        assert not base.bits(d3[0, 0, cells]).any() and (v3[0, 0, cells] == np.inf).all() and np.isfinite(v3[0, 0, ~cells]).all()


# ---- 4. state and arguments ------------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    scene, bins, labels = "cornell-srgb", 8, probe_labels()
    B = other(scene, bins)
    info, SB, NB, QB = B
    r = renderer(scene)
    sets = (SB, QB, NB, SB, QB, NB)
    zero = np.zeros((H, W), dtype=np.uint8)
    # the pure call: bins, size, NULL pointers, regions, labels, t2
    lib, ctx, p = r._lib, r._ctx, lambda a: a.ctypes.data
    outs = [np.zeros((1, bins)) for _ in range(3)] + [np.zeros((1, bins), dtype=np.uint64) for _ in range(3)]
    def pure(width=W, height=H, nbins=bins, SA=p(SB), lab=p(zero), R=1, t2=9.0, DD=p(outs[0])):
        r._check(lib.ssx_spectral_compare_arrays(ctx, width, height, nbins, SA, p(QB), p(NB), p(SB), p(QB), p(NB), lab, R, t2, DD, *[p(o) for o in outs[1:]], None, None))
    pure()
    refused(lambda: pure(nbins=6), _capi.SSX_ERR_ARG, "6 bins")
    refused(lambda: pure(nbins=68), _capi.SSX_ERR_ARG, "68 bins")
    refused(lambda: pure(width=0), _capi.SSX_ERR_ARG, "width and height")
    refused(lambda: pure(SA=None), _capi.SSX_ERR_ARG, "SA, QA and NA")
    refused(lambda: pure(lab=None), _capi.SSX_ERR_ARG, "labels and the six outputs")
    refused(lambda: pure(DD=None), _capi.SSX_ERR_ARG, "labels and the six outputs")
    refused(lambda: pure(R=0), _capi.SSX_ERR_ARG, "1..32")
    refused(lambda: pure(R=33), _capi.SSX_ERR_ARG, "1..32")
    refused(lambda: r.compare_arrays(*sets, labels, 8), _capi.SSX_ERR_ARG, "labels[")
    bad = labels.copy(); bad[0, 0] = 200
    refused(lambda: r.compare_arrays(*sets, bad, 32), _capi.SSX_ERR_ARG, "labels[0][0] = 200")
    for t2 in (-1.0, np.inf, np.nan):
        refused(lambda: r.compare_arrays(*sets, zero, 1, t2=t2), _capi.SSX_ERR_ARG, "t2")
    # the context's own state: what ssx_spectral_variance asks, with its reasons
    refused(lambda: r.compare_spectral_raw(B, zero), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(bins)
    start(r, 8)
    refused(lambda: r.compare_spectral_raw(B, zero), _capi.SSX_ERR_STATE, "spectral moments are off")
    r.set_spectral_moments(True)
    refused(lambda: r.compare_spectral_raw(B, zero), _capi.SSX_ERR_STATE, "switched on after the render")
    start(r, 8)
    r.compare_spectral_raw(B, zero)
    # other_info against the context, field by field; done_spp may differ
    def with_info(**kw):
        i = copy.copy(info)
        for k, v in kw.items():
            setattr(i, k, v)
        return lambda: r.compare_spectral_raw((i, SB, NB, QB), zero)
    with_info(done_spp=info.done_spp + 100)()
    # (the wrapper sizes B's arrays by the info, so a changed size or bin count goes to the library directly)
    def direct(i):
        return lambda: r._check(lib.ssx_spectral_compare(ctx, None if i is None else C.byref(i), p(SB), p(QB), p(NB), p(zero), 1, 9.0, *[p(o) for o in outs], None, None))
    def changed(**kw):
        i = copy.copy(info)
        for k, v in kw.items():
            setattr(i, k, v)
        return i
    refused(direct(None), _capi.SSX_ERR_ARG, "other_info")
    refused(direct(changed(struct_size=8)), _capi.SSX_ERR_ARG, "struct_size")
    refused(direct(changed(width=W + 1)), _capi.SSX_ERR_ARG, "size differs")
    refused(direct(changed(height=H - 1)), _capi.SSX_ERR_ARG, "size differs")
    refused(direct(changed(bins=16)), _capi.SSX_ERR_ARG, "bins differs")
    refused(with_info(lambda_min=float(np.nextafter(np.float32(info.lambda_min), np.float32(1e9)))), _capi.SSX_ERR_ARG, "lambda_min differs")
    refused(with_info(bin_width=float(np.nextafter(np.float32(info.bin_width), np.float32(0)))), _capi.SSX_ERR_ARG, "bin_width differs")
    refused(lambda: r.compare_spectral_raw(B, zero, threshold=float("nan")), _capi.SSX_ERR_ARG, "t2")
    # while a render runs
    r._check(lib.ssx_render_continue(ctx, 1 << 16))
    try:
        refused(lambda: r.compare_spectral_raw(B, zero), _capi.SSX_ERR_STATE, "render in progress")
        refused(lambda: r.compare_arrays(*sets, zero, 1), _capi.SSX_ERR_STATE, "render in progress")
    finally:
        lib.ssx_render_stop(ctx)
        r.render_wait()


def test_a_compare_changes_nothing_a_continue_builds_on():
    scene, bins = "cornell-srgb", 8
    whole = render_a(scene, bins)
    r = moments_renderer(scene, bins)
    start(r, 16)
    r.compare_spectral_raw(other(scene, bins), probe_labels(), 32)
    r.render_continue(21); r.render_wait()
    assert r.done_spp() == SPP_A and same(r.xyza, whole.xyza)
    for g, w, name in zip(arrays_of(r)[1:], arrays_of(whole)[1:], "SQN"):
        assert same(g, w), name


# ---- 5. CLI ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_compares_with_a_checkpoint(tmp_path):
    ck, csv, npy, png = (str(tmp_path / n) for n in ("b.ckpt", "c.csv", "z.npy", "o.png"))
    rects = [(6, 5, 20, 12), (3, 3, 4, 4)]
    common = [base.CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "--texture=data/scenes/test-img.png", "-o=" + png, "--spectral-bins=8"]
    p = subprocess.run(common + ["-spp=%d" % SPP_A, "--seed=%d" % base.SEED, "--checkpoint=" + ck, "--spectral-variance-output=" + str(tmp_path / "v.npy")],
                       cwd=base.ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert open(ck, "rb").read(8) == b"SSXCKPT3"
    compare = ["-spp=%d" % SPP_B, "--seed=%d" % SEED_B, "--compare-to=" + ck, "--compare-output=" + csv, "--compare-map-output=" + npy, "--compare-threshold=2"]
    p = subprocess.run(common + compare + ["--probe=%d,%d,%d,%d" % q for q in rects], cwd=base.ROOT, capture_output=True, text=True)
    assert p.returncode == 0 and "same seed" not in p.stderr, p.stderr
    # the same comparison through Python: A is the CLI's render (seed 6), B the checkpoint (seed 5)
    r = moments_renderer("cornell-srgb", 8)
    start(r, SPP_B, seed=SEED_B)
    sums, diff, var = r.compare_spectral_raw(load_checkpoint_file_moments(ck), stats.labels_from_rects((W, H), rects), threshold=2.0)
    fig = compare_derive(*sums)
    lines = open(csv).read().split("\n")
    assert lines[0] == "region,bin,wavelength,mean_diff,stderr,z,chi2,exceed,comparable,not_comparable" and len(lines) == 2 + 2 * 8 and lines[-1] == ""
    centres = r.spectral_image()[2]
    for k, line in enumerate(lines[1:-1]):
        f = line.split(",")
        reg, b = divmod(k, 8)
        assert (int(f[0]), int(f[1]), int(f[8]), int(f[9])) == (reg, b, int(sums[3][reg, b]), int(sums[4][reg, b])) and np.float32(f[2]) == centres[b]
        for col, name in zip(range(3, 8), ("mean_diff", "stderr", "z", "chi2", "exceed")):
            v = fig[name][reg, b]
            assert (f[col] == "nan") if np.isnan(v) else (float(f[col]) == v), (name, reg, b)
    z = np.load(npy)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert z.dtype == np.float32 and z.shape == (H, W, 8) and same(z, np.where(np.isposinf(var), np.float32(0), diff / np.sqrt(var)).astype(np.float32)) and same(z, compare_zmap(diff, var))
    # the refusal that needs the scene, and the warning: a checkpoint whose bins start elsewhere; the same seed
    loaded = load_checkpoint_file_moments(ck)
    info, sums_, s2, name, text, sinfo, S, N, Q = loaded
    sinfo.lambda_min += 1.0
    moved = str(tmp_path / "moved.ckpt")
    host = _capi.host_lib()
    assert host.ssh_checkpoint_save_moments(os.fsencode(moved), C.byref(info), name.encode(), text.encode(), sums_.ctypes.data, None if s2 is None else s2.ctypes.data,
                                            C.byref(sinfo), S.ctypes.data, N.ctypes.data, Q.ctypes.data) == 0
    os.remove(csv)
    p = subprocess.run(common + ["-spp=4", "--seed=%d" % base.SEED, "--compare-to=" + moved, "--compare-output=" + csv], cwd=base.ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "lambda_min or bin_width differs" in p.stderr and not os.path.exists(csv), p.stderr
    assert "same seed: the samples are not independent; z is not calibrated" in p.stderr
