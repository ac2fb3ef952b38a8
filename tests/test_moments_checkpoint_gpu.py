"""The bins' second moments through checkpoint, resume and import on the GPU (include/ssx.h ssx_spectral_moments_import): a render with
the moments on that is exported and imported -- directly, through a checkpoint file, onto another partition of the tiles -- and continued holds the bits of the
one-shot render in Q and in everything computed from it: the variances, the region probes, the spectral noise figure and the stopping rule.  "equals" is
np.array_equal on the integer views (bit for bit; there are no tolerances).  The harness is tests/test_spectral_checkpoint_gpu.py's: 42 x 23 images (six tile
columns and three rows, the last of each ragged), seed 5, 12 samples per pixel as 5 + 7 in launches of 4."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import moments_import_ref as mref
import test_spectral_checkpoint_gpu as ck
from simple_spectral_amd import _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import SsxError, labels_from_rects, load_checkpoint_file_moments, merge_moments, merge_spectral, merge_sums

pytestmark = pytest.mark.gpu
W, H, SEED, SPP, CLI, ROOT = ck.W, ck.H, ck.SEED, ck.SPP, ck.CLI, ck.ROOT
bits, same, start, cont, refused, frozen = ck.bits, ck.same, ck.start, ck.cont, ck.refused, ck.frozen
RECTS = [(6, 5, 20, 12), (38, 19, 42, 23), (0, 0, 9, 2)]       # one crosses tiles, one is the ragged corner, one lies on the bottom edge


def renderer(scene, bins, moments=True, **opts):
    r = ck.renderer(scene, bins, **opts)
    if moments:
        r.set_spectral_moments(True)
    return r


def state(r):
    """Everything the moments feed, and the image and bins beside them: (Q, var, SS, NN, VV, UU, EV, EM, PP, PU, mean, sums, counts, xyza)"""
    _, var, Q = r.spectral_variance(q=True)
    return (Q, var) + tuple(r.probe_raw(labels_from_rects((W, H), RECTS))) + tuple(r.spectral_noise_raw()[0]) + tuple(ck.state(r))


@functools.lru_cache(maxsize=None)
def one_shot(scene, bins):
    """The reference of every test: 12 samples per pixel in one render with the moments on; computed once, read-only."""
    r = renderer(scene, bins)
    start(r, SPP)
    return frozen(*state(r))


@functools.lru_cache(maxsize=None)
def part(scene, bins, spp=5, owner=(0, 1, 0)):
    """A render of `spp` samples by the context that owns `owner` = (tile_first, tile_stride, tile_skew), exported: (sums info, sums, spectral info, S, N, Q)"""
    r = renderer(scene, bins, tile_first=owner[0], tile_stride=owner[1], tile_skew=owner[2])
    start(r, spp)
    info, sums, _ = r.export_sums()
    sinfo, S, N = r.export_spectral()
    qinfo, Q = r.export_moments()
    assert bytes(qinfo) == bytes(sinfo) and r.holds_moments()
    frozen(sums, S, N, Q)
    return info, sums, sinfo, S, N, Q


def take_bins(r, p):
    info, sums, sinfo, S, N, _ = p
    r.import_sums(info, sums)
    r.import_spectral(sinfo, S, N)


def resumed(scene, bins, spp=5, **opts):
    """A fresh context that took `part` up: sums, bins and moments"""
    p = part(scene, bins, spp)
    r = renderer(scene, bins, **opts)
    take_bins(r, p)
    r.import_moments(p[2], p[5])
    return r


# ---- 1. export, import, continue: the one-shot render's bits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,bins", [("cornell-srgb", 4), ("cornell-srgb", 12), ("cornell-srgb", 64), ("plane-srgb", 16)])
def test_resumed_moments_equal_the_one_shot_render(scene, bins):
    ref, p = one_shot(scene, bins), part(scene, bins)
    n = np.tile(p[4], (1, 1, 4))
    assert (bins == 4) or ((n == 0).any() and (n == 1).any() and (n >= 2).any())         # every branch of the import's check is taken
    assert mref.broken_rule(p[3], p[5], p[4]) is None                                    # ... and the restated check accepts what the device produced
    r = resumed(scene, bins)
    assert r.holds_moments()
    info, Q = r.export_moments()                               # straight after the import: the exporter's state
    assert (info.bins, info.done_spp) == (bins, 5) and same((Q,), (p[5],)) and same(r.export_spectral()[1:], p[3:5])
    cont(r, 7)                                                 # launches of 4 + 3
    assert r.done_spp() == SPP and same(state(r), ref)
    assert ref[0].any() and np.isfinite(ref[1]).any() and ref[4].any()
    # set_spectral_moments may also come after the two imports underneath
    late = renderer(scene, bins, moments=False)
    take_bins(late, p)
    late.set_spectral_moments(True)
    late.import_moments(p[2], p[5])
    cont(late, 7)
    assert same(state(late), ref)


def test_import_from_zero_samples_and_scratch_info():
    info, sums, sinfo, S, N, Q = part("cornell-srgb", 16)
    info0, sinfo0 = type(info).from_buffer_copy(info), type(sinfo).from_buffer_copy(sinfo)
    info0.done_spp = sinfo0.done_spp = 0
    r = renderer("cornell-srgb", 16)
    r.import_sums(info0, np.zeros_like(sums))
    r.import_spectral(sinfo0, np.zeros_like(S), np.zeros_like(N))
    before = r.scratch_info()["sample_bytes"]
    r.import_moments(sinfo0, np.zeros_like(Q))
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert r.scratch_info()["sample_bytes"] - before == tiles * 16 * 64 * 8   # Q is reserved for the owned tiles by the import, and counted
    cont(r, SPP)
    assert same(state(r), one_shot("cornell-srgb", 16))


# ---- 2. through the file -------------------------------------------------------------------------------------------------------------------------------------

def test_checkpoint_file_carries_the_moments(tmp_path):
    scene, bins = "cornell-srgb", 12
    ref, p = one_shot(scene, bins), part(scene, bins)
    path = str(tmp_path / "c.ckpt")
    resumed(scene, bins).save_checkpoint(path)
    assert open(path, "rb").read(8) == b"SSXCKPT3"
    *_, sinfo, S, N, Q = load_checkpoint_file_moments(path)
    assert bytes(sinfo) == bytes(p[2]) and same((S, N, Q), p[3:])
    b = renderer(scene, bins)
    assert b.load_checkpoint(path).done_spp == 5 and b.spectral_resumed and b.moments_resumed
    cont(b, 7)
    assert same(state(b), ref)
    again = str(tmp_path / "c12.ckpt")                         # the resumed render's own checkpoint carries them on
    b.save_checkpoint(again)
    assert open(again, "rb").read(8) == b"SSXCKPT3" and same((load_checkpoint_file_moments(again)[-1],), ref[:1])
    # a loader with the moments off takes the bins only; its own checkpoint is the SSXCKPT2 file
    c = renderer(scene, bins, moments=False)
    assert c.load_checkpoint(path).done_spp == 5 and c.spectral_resumed and not c.moments_resumed and not c.holds_moments()
    cont(c, 7)
    assert same(ck.state(c), ref[10:])
    refused(c.spectral_variance, _capi.SSX_ERR_STATE, "moments are off")
    c.save_checkpoint(again)
    assert open(again, "rb").read(8) == b"SSXCKPT2"
    # the moments on, but another bin count: the plain resume
    d = renderer(scene, 8)
    assert d.load_checkpoint(path).done_spp == 5 and not d.spectral_resumed and not d.moments_resumed


# ---- 3. another partition of the tiles ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ranks_merged(bins, world):
    """`world` contexts (tile_stride world, tile_skew 1) render 5 samples; their exports merged by ownership on the host: (info, sums, sinfo, S, N, Q), and the
    ranks' own unmerged Q."""
    sums, S, N, Q = np.zeros((H, W, 4)), np.full((H, W, bins), 7.0), np.full((H, W, bins // 4), 7, dtype=np.uint32), np.full((H, W, bins), 7.0)
    lone = []
    for first in range(world):
        info, p_sums, sinfo, p_S, p_N, p_Q = part("cornell-srgb", bins, 5, (first, world, 1))
        mask = tile_owner_mask(W, H, first, world, 1)
        assert not bits(p_Q)[~mask].any()                      # zeros where the rank owns nothing
        merge_sums(sums, None, p_sums, None, info)
        merge_spectral(S, N, p_S, p_N, info)
        merge_moments(Q, p_Q, info)
        lone.append(p_Q)
    info = type(info).from_buffer_copy(info)
    info.tile_first, info.tile_stride, info.tile_skew = 0, 1, 0    # the merged arrays are the whole image
    frozen(sums, S, N, Q)
    return info, sums, sinfo, S, N, Q, lone


@pytest.mark.parametrize("world,into", [(2, 1), (2, 3), (3, 1), (3, 2)])
def test_repartitioned_moments_equal_the_one_shot_render(world, into):
    bins = 16
    info, sums, sinfo, S, N, Q, _ = ranks_merged(bins, world)
    assert same((sums, S, N, Q), (part("cornell-srgb", bins)[1],) + part("cornell-srgb", bins)[3:])
    ref = one_shot("cornell-srgb", bins)
    if into == 1:
        r = renderer("cornell-srgb", bins)
        take_bins(r, (info, sums, sinfo, S, N, Q))
        r.import_moments(sinfo, Q)
        cont(r, 7)
        assert same(state(r), ref)
        return
    got_q, got_var = np.zeros_like(ref[0]), np.zeros_like(ref[1])
    for first in range(into):
        r = renderer("cornell-srgb", bins, tile_first=first, tile_stride=into, tile_skew=1)
        take_bins(r, (info, sums, sinfo, S, N, Q))
        r.import_moments(sinfo, Q)
        cont(r, 7)
        mask = tile_owner_mask(W, H, first, into, 1)
        _, var, q = r.spectral_variance(q=True)
        assert not bits(q)[~mask].any()
        got_q[mask], got_var[mask] = q[mask], var[mask]
    assert same((got_q, got_var), ref[:2])


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------------------

def raw_import(r, si, q):                                       # (past the binding's own check of the shape)
    q = np.ascontiguousarray(q, dtype=np.float64)
    r._check(r._lib.ssx_spectral_moments_import(r._ctx, None if si is None else C.byref(si), None if q is None else q.ctypes.data))


def test_refusals_by_state_and_by_field():
    scene, bins = "cornell-srgb", 16
    p = part(scene, bins)
    info, sums, sinfo, S, N, Q = p
    ref = one_shot(scene, bins)
    what = "ssx_spectral_moments_import"

    def changed(**kw):
        si = type(sinfo).from_buffer_copy(sinfo)
        for k, v in kw.items():
            setattr(si, k, v)
        return si

    # state: no ssx_spectral_import underneath; its own render; rendered since; the moments off; the bins off; a render running
    r = renderer(scene, bins)
    refused(lambda: raw_import(r, sinfo, Q), _capi.SSX_ERR_STATE, what, "ssx_spectral_import")
    r.import_sums(info, sums)
    refused(lambda: raw_import(r, sinfo, Q), _capi.SSX_ERR_STATE, what, "ssx_spectral_import")
    start(r, 5)
    refused(lambda: raw_import(r, sinfo, Q), _capi.SSX_ERR_STATE, what, "ssx_spectral_import")
    take_bins(r, p)
    cont(r, 1)
    refused(lambda: raw_import(r, changed(done_spp=6), Q), _capi.SSX_ERR_STATE, what, "rendered since")
    off = renderer(scene, bins, moments=False)
    take_bins(off, p)
    refused(lambda: raw_import(off, sinfo, Q), _capi.SSX_ERR_STATE, what, "moments are off")
    none = ck.renderer(scene, 0)
    none.import_sums(info, sums)
    refused(lambda: raw_import(none, sinfo, Q), _capi.SSX_ERR_STATE, what, "spectral output is off")
    take_bins(r, p)
    r._check(r._lib.ssx_render_continue(r._ctx, 1 << 20))
    try:
        refused(lambda: raw_import(r, sinfo, Q), _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop()
        r.render_wait()

    # ssx_spectral_import alone behaves as before: the moments invalid, and the reason points at the new call
    r = renderer(scene, bins)
    take_bins(r, p)
    refused(r.spectral_variance, _capi.SSX_ERR_STATE, "ssx_spectral_import", "does not carry", what)
    # arguments, each named; after every refusal the moments are invalid and a continue renders normally, bins included
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
    for call, words in ((lambda: raw_import(r, changed(width=W + 1), Q), ("size differs",)),
                        (lambda: raw_import(r, changed(height=H - 1), Q), ("size differs",)),
                        (lambda: raw_import(r, changed(bins=8), Q[..., :8]), ("bins differs",)),
                        (lambda: raw_import(r, changed(done_spp=6), Q), ("done_spp differs",)),
                        (lambda: raw_import(r, changed(lambda_min=up(sinfo.lambda_min)), Q), ("lambda_min differs",)),
                        (lambda: raw_import(r, changed(bin_width=up(sinfo.bin_width)), Q), ("bin_width differs",)),
                        (lambda: raw_import(r, changed(struct_size=sinfo.struct_size + 4), Q), ("struct_size",)),
                        (lambda: r._check(r._lib.ssx_spectral_moments_import(r._ctx, C.byref(sinfo), None)), ("NULL",)),
                        (lambda: r._check(r._lib.ssx_spectral_moments_import(r._ctx, None, Q.ctypes.data)), ("NULL",))):
        take_bins(r, p)
        refused(call, _capi.SSX_ERR_ARG, what, *words)
        refused(r.spectral_variance, _capi.SSX_ERR_STATE, what)
        refused(lambda: r.probe_raw(labels_from_rects((W, H), RECTS)), _capi.SSX_ERR_STATE)
        refused(r.spectral_noise_raw, _capi.SSX_ERR_STATE)
        assert same(r.export_spectral()[1:], (S, N)) and np.array_equal(bits(r.export_sums()[1]), bits(sums))     # bins and pixel sums untouched
        cont(r, 7)
        assert same(ck.state(r), ref[10:])
        refused(r.spectral_variance, _capi.SSX_ERR_STATE)
    # still directly on top of the import after a refusal: the right array is taken
    take_bins(r, p)
    refused(lambda: raw_import(r, changed(done_spp=6), Q), _capi.SSX_ERR_ARG, "done_spp differs")
    raw_import(r, sinfo, Q)
    cont(r, 7)
    assert same(state(r), ref)
    with pytest.raises(ValueError):                            # the binding's own check of the shape
        r.import_moments(sinfo, Q[..., :8])


def test_each_rule_of_the_check_refuses_one_edited_element():
    scene, bins = "cornell-srgb", 16
    p = part(scene, bins)
    info, sums, sinfo, S, N, Q = p
    ref = one_shot(scene, bins)
    n = np.tile(N, (1, 1, 4))
    corner = (H - 1, W - 1)                                    # the last in-image pixel of the ragged corner tile
    edits = []
    for rule, where in ((0, n == 0), (1, (n == 1) & (S * S != S)), (2, n >= 2)):
        found = np.argwhere(where)
        assert len(found), rule
        edits.append((rule, tuple(found[len(found) // 2])))
        in_corner = [tuple(a) for a in found if tuple(a[:2]) == corner]
        if in_corner:
            edits.append((rule, in_corner[-1]))
        right = [tuple(a) for a in found if a[1] == W - 1 and a[0] < H - 1]     # the ragged column's last in-image pixel of a row
        if right:
            edits.append((rule, right[0]))
    assert any(at[:2] == corner for _, at in edits)
    r = renderer(scene, bins)
    for rule, at in edits:
        for value in {0: (1.0, -0.0, 5e-324), 1: (float(np.nextafter(Q[at], np.inf)), 0.0, float(S[at])), 2: (-5e-324, -1.0)}[rule]:
            q = Q.copy()
            q[at] = value
            assert mref.broken_rule(S, q, N) == rule           # the restated check names the same rule
            take_bins(r, p)
            refused(lambda: r.import_moments(sinfo, q), _capi.SSX_ERR_ARG, "ssx_spectral_moments_import", "rule " + mref.RULES[rule])
            refused(r.spectral_variance, _capi.SSX_ERR_STATE, "ssx_spectral_moments_import")
        cont(r, 7)
        assert same(ck.state(r), ref[10:])
    # what the rules do not hold: at n >= 2 any non-negative value and a NaN pass (the file's checksum vouches for those)
    at = edits[-1][1]
    q = Q.copy()
    q[at] = np.nan
    take_bins(r, p)
    r.import_moments(sinfo, q)
    assert np.isnan(r.export_moments()[1][at])
    # a pixel outside the tiles the context owns is held to nothing, and nothing of it is taken
    mask = tile_owner_mask(W, H, 1, 3, 1)
    foreign = tuple(np.argwhere(~mask[..., None] & (n == 0))[0])
    q = Q.copy()
    q[foreign] = 1.0
    third = renderer(scene, bins, tile_first=1, tile_stride=3, tile_skew=1)
    take_bins(third, p)
    third.import_moments(sinfo, q)
    got = third.export_moments()[1]
    assert np.array_equal(bits(got)[mask], bits(Q)[mask]) and not bits(got)[~mask].any()


def test_one_ranks_unmerged_moments_are_refused():
    """64 bins and 5 samples: sub-bins with one sample are plentiful, and rank 1's export holds +0.0 for them wherever it owns nothing."""
    scene, bins = "cornell-srgb", 64
    info, sums, sinfo, S, N, Q, lone = ranks_merged(bins, 3)
    foreign = ~tile_owner_mask(W, H, 1, 3, 1)
    n = np.tile(N, (1, 1, 4))
    assert ((n == 1) & (S != 0.0) & foreign[..., None]).any()  # what rule n == 1 catches: Q = +0.0 against S * S != 0
    assert mref.broken_rule(S, lone[1], N) == 1
    r = renderer(scene, bins)
    take_bins(r, (info, sums, sinfo, S, N, Q))
    refused(lambda: r.import_moments(sinfo, lone[1]), _capi.SSX_ERR_ARG, "ssx_spectral_moments_import", "rule n == 1", "merge")
    refused(r.spectral_variance, _capi.SSX_ERR_STATE)
    cont(r, 7)
    assert same(ck.state(r), one_shot(scene, bins)[10:])
    # the context that owns exactly those tiles takes its own export
    own = renderer(scene, bins, tile_first=1, tile_stride=3, tile_skew=1)
    take_bins(own, (info, sums, sinfo, S, N, Q))
    own.import_moments(sinfo, lone[1])
    assert same((own.export_moments()[1],), (lone[1],))
    # S handed in as Q
    take_bins(r, (info, sums, sinfo, S, N, Q))
    refused(lambda: r.import_moments(sinfo, S), _capi.SSX_ERR_ARG, "rule n == 1")


# ---- 5. the stopping rule, resumed ----------------------------------------------------------------------------------------------------------------------------

def triple_bits(t):
    return (t[0], struct.pack("<dd", t[1], t[2]))


def test_render_until_spectral_resumes_to_the_uninterrupted_run(tmp_path):
    scene, bins, step, cap, cover = "cornell-srgb", 8, 4, 40, 0.9
    # a first pass: the figure after every step, from which the targets are chosen
    first = renderer(scene, bins)
    start(first, step)
    figures = []
    while True:
        noise, coverage, _ = first.spectral_noise()
        figures.append((first.done_spp(), noise, coverage))
        if first.done_spp() >= cap:
            break
        cont(first, step)
    stops_at = lambda t: next((k for k, (_, v, c) in enumerate(figures) if v <= t and c >= cover), len(figures) - 1)
    covered = [k for k, f in enumerate(figures) if f[2] >= cover]
    assert covered and covered[0] + 2 < len(figures)
    k1 = covered[0] + 1
    t1 = figures[k1][1]
    t2 = min(f[1] for f in figures[k1 + 1:-1])
    k1, k2 = stops_at(t1), stops_at(t2)
    assert t2 < t1 and k1 < k2 < len(figures) - 1              # the first run stops before the cap, the second later and also by its target
    n1 = figures[k1][0]
    a = renderer(scene, bins)
    got1 = a.render_until_spectral(t1, step, cap, min_coverage=cover)
    assert got1[0] == n1 < cap and triple_bits(got1) == triple_bits(figures[k1])
    path = str(tmp_path / "u.ckpt")
    a.save_checkpoint(path)
    assert open(path, "rb").read(8) == b"SSXCKPT3"
    whole = renderer(scene, bins)
    want2 = whole.render_until_spectral(t2, step, cap, min_coverage=cover)
    assert want2[0] == figures[k2][0] and triple_bits(want2) == triple_bits(figures[k2])
    b = renderer(scene, bins)
    assert b.load_checkpoint(path).done_spp == n1 and b.moments_resumed
    got2 = b.render_until_spectral(t2, step, cap, min_coverage=cover, resume=True)
    assert triple_bits(got2) == triple_bits(want2)
    assert same(state(b), state(whole))
    # resumed with the first target again it renders nothing
    c = renderer(scene, bins)
    c.load_checkpoint(path)
    assert triple_bits(c.render_until_spectral(t1, step, cap, min_coverage=cover, resume=True)) == triple_bits(got1) and c.done_spp() == n1
    # ... and at the cap likewise
    assert c.render_until_spectral(0.0, step, n1, min_coverage=cover, resume=True)[0] == n1
    # without valid moments a resume is refused; nothing was started
    d = renderer(scene, bins, moments=False)
    d.load_checkpoint(path)
    refused(lambda: d.render_until_spectral(t2, step, cap, min_coverage=cover, resume=True), _capi.SSX_ERR_STATE, "moments")
    assert d.done_spp() == n1


# ---- 6. CLI -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_checkpoint_and_resume_with_the_probe(tmp_path):
    common = ["-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "--spectral-bins=16"]
    probes = ["--probe=%d,%d,%d,%d" % q for q in RECTS]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True)
    path, csv5, csv12, one, png, var12, var1 = (str(tmp_path / n) for n in ("c.ckpt", "five.csv", "twelve.csv", "one.csv", "o.png", "v12.npy", "v1.npy"))
    p = run("-spp=5", "-o=" + png, "--checkpoint=" + path, "--probe-output=" + csv5, *probes)
    assert p.returncode == 0, p.stderr
    assert open(path, "rb").read(8) == b"SSXCKPT3"
    *_, sinfo, S, N, Q = load_checkpoint_file_moments(path)
    assert (sinfo.bins, sinfo.done_spp) == (16, 5) and same((S, N, Q), part("cornell-srgb", 16)[3:])
    p = run("-spp=%d" % SPP, "-o=" + png, "--resume=" + path, "--probe-output=" + csv12, "--spectral-variance-output=" + var12, *probes)
    assert p.returncode == 0 and "5 samples per pixel done, 12 wanted" in p.stderr, p.stderr
    p = run("-spp=%d" % SPP, "-o=" + png, "--probe-output=" + one, "--spectral-variance-output=" + var1, *probes)
    assert p.returncode == 0, p.stderr
    assert open(csv12, "rb").read() == open(one, "rb").read() and open(csv12, "rb").read() != open(csv5, "rb").read()
    assert open(var12, "rb").read() == open(var1, "rb").read()
    assert same((np.load(var12),), one_shot("cornell-srgb", 16)[1:2])
