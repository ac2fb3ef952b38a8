"""The wavelength bins through checkpoint, resume and import on the GPU (include/ssx.h ssx_spectral_import): a render that is exported and
imported -- directly, through a checkpoint file, onto another partition of the tiles -- and continued holds the bits of the one-shot render, in the image, in the
bins and in everything developed or filtered from them.  "equals" is np.array_equal on the integer views (bit for bit; there are no tolerances).  Images are
42 x 23: six tile columns and three rows, the last of each ragged.  12 samples per pixel: 5 + 7 (the 7 in launches of 4 + 3) where only sums are compared, which
do not depend on the launches; 4 + 4 + 4 on both sides where the noise estimate takes part, whose batches are the launches."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import SsxError, develop_weights, load_checkpoint_file, load_checkpoint_file_spectral, merge_spectral, merge_sums

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
TEX = "test-img.png"
W, H, SEED, SPP = 42, 23, 5, 12


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same(got, ref):
    return len(got) == len(ref) and all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, ref))


def renderer(scene, bins, noise=False, **opts):
    opts.setdefault("spp_per_launch", 4)
    r = Renderer(Options(scene_name=scene, res=(W, H), seed=SEED, texture=TEX, **opts))
    if noise:
        r.set_noise_estimate(True)
    if bins:
        r.set_spectral_bins(bins)
    return r


def start(r, spp):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp))))
    r.render_wait()


def cont(r, spp):
    r.render_continue(spp)
    r.render_wait()


def state(r):
    """(mean, sums, counts, xyza) of the context"""
    _, mean, counts, sums = r.spectral_read(sums=True)
    return mean, sums, counts, r.xyza.copy()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def one_shot(scene, bins):
    """The reference of every test: 12 samples per pixel in one render (launches of 4, the noise estimate on); computed once, read-only."""
    r = renderer(scene, bins, noise=True)
    start(r, SPP)
    return r, frozen(*state(r))


@functools.lru_cache(maxsize=None)
def part(scene, bins, spp, noise=False):
    """A whole-image render of `spp` samples, exported: (sums info, sums, S2 or None, spectral info, bin sums, counts); computed once, read-only."""
    r = renderer(scene, bins, noise=noise)
    start(r, spp)
    info, sums, s2 = r.export_sums()
    sinfo, S, N = r.export_spectral()
    frozen(sums, S, N, *(() if s2 is None else (s2,)))
    return info, sums, s2, sinfo, S, N


def resumed(scene, bins, spp, noise=False, **opts):
    """A fresh context that took `part` up, sums and bins"""
    info, sums, s2, sinfo, S, N = part(scene, bins, spp, noise)
    r = renderer(scene, bins, noise=noise, **opts)
    r.import_sums(info, sums, s2)
    r.import_spectral(sinfo, S, N)
    return r


def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


# ---- 1. export, import, continue: the one-shot render's bits -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,bins", [("cornell-srgb", 4), ("cornell-srgb", 16), ("cornell-srgb", 64), ("plane-srgb", 16)])
def test_resumed_render_equals_the_one_shot_render(scene, bins, tmp_path):
    _, ref = one_shot(scene, bins)
    assert (ref[2].sum(axis=2) == SPP).all()                   # every sample counted once: what the import checks
    r = resumed(scene, bins, 5)
    info, mean, counts, sums = r.spectral_read(sums=True)      # straight after the import: the exporter's state
    assert (info.bins, info.done_spp) == (bins, 5) and same((sums, counts), part(scene, bins, 5)[4:])
    cont(r, 7)                                                 # launches of 4 + 3
    assert r.done_spp() == SPP and same(state(r), ref)
    # ... and through the file
    ck = str(tmp_path / "c.ckpt")
    a = resumed(scene, bins, 5)
    a.save_checkpoint(ck)
    assert open(ck, "rb").read(8) == b"SSXCKPT2"
    *_, sinfo, S, N = load_checkpoint_file_spectral(ck)
    assert bytes(sinfo) == bytes(part(scene, bins, 5)[3]) and same((S, N), part(scene, bins, 5)[4:])
    b = renderer(scene, bins)
    assert b.load_checkpoint(ck).done_spp == 5 and b.spectral_resumed
    cont(b, 7)
    assert same(state(b), ref)
    # a resume that does not ask for the bins takes the pixel sums of the same file; one with another bin count likewise
    for other in (0, 8 if bins != 8 else 4):
        c = renderer(scene, other)
        assert c.load_checkpoint(ck).done_spp == 5 and not c.spectral_resumed
        cont(c, 7)
        assert np.array_equal(bits(c.xyza), bits(ref[3]))
        if other:
            refused(c.spectral_read, _capi.SSX_ERR_STATE)


def test_checkpoint_without_bins_is_the_file_it_always_was(tmp_path):
    """spectral output off, or on without valid bins: no SSXCKPT2"""
    info, sums, s2 = part("cornell-srgb", 16, 5)[:3]
    off, on = renderer("cornell-srgb", 0), renderer("cornell-srgb", 16)
    paths = [str(tmp_path / n) for n in ("off.ckpt", "on.ckpt")]
    for r, p in zip((off, on), paths):
        r.import_sums(info, sums, s2)
        r.save_checkpoint(p)
    raw = open(paths[0], "rb").read()
    assert raw[:8] == b"SSXCKPT1" and raw == open(paths[1], "rb").read()
    assert np.array_equal(bits(load_checkpoint_file(paths[0])[1]), bits(sums))


def test_import_from_zero_samples():
    info, sums, _, sinfo, S, N = part("cornell-srgb", 16, 5)
    info0, sinfo0 = type(info).from_buffer_copy(info), type(sinfo).from_buffer_copy(sinfo)
    info0.done_spp = sinfo0.done_spp = 0
    r = renderer("cornell-srgb", 16)
    r.import_sums(info0, np.zeros_like(sums))
    r.import_spectral(sinfo0, np.zeros_like(S), np.zeros_like(N))
    assert r.done_spp() == 0
    cont(r, SPP)
    assert same(state(r), one_shot("cornell-srgb", 16)[1])


# ---- 2. another partition of the tiles ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def three_ranks_merged():
    """Three contexts (tile_stride 3, tile_skew 1) render 5 samples; their exports merged by ownership on the host, and rank 1's own, unmerged."""
    sums, S, N = np.zeros((H, W, 4)), np.full((H, W, 16), 7.0), np.full((H, W, 4), 7, dtype=np.uint32)
    for first in range(3):
        r = renderer("cornell-srgb", 16, tile_first=first, tile_stride=3, tile_skew=1)
        start(r, 5)
        info, p_sums, _ = r.export_sums()
        sinfo, p_S, p_N = r.export_spectral()
        mask = tile_owner_mask(W, H, first, 3, 1)
        assert not p_S[~mask].any() and not p_N[~mask].any() and (p_N[mask].sum(axis=1) == 5).all()
        merge_sums(sums, None, p_sums, None, info)
        merge_spectral(S, N, p_S, p_N, info)
        if first == 1:
            lone = frozen(p_S, p_N)
    info.tile_first, info.tile_stride, info.tile_skew = 0, 1, 0       # the merged arrays are the whole image
    frozen(sums, S, N)
    return info, sums, sinfo, S, N, lone


def test_merged_exports_of_three_equal_the_whole_render():
    _, sums, _, S, N, _ = three_ranks_merged()
    assert same((sums, S, N), (part("cornell-srgb", 16, 5)[1],) + part("cornell-srgb", 16, 5)[4:])


@pytest.mark.parametrize("world", [1, 2])
def test_repartitioned_resume_equals_the_one_shot_render(world):
    info, sums, sinfo, S, N, _ = three_ranks_merged()
    ref = one_shot("cornell-srgb", 16)[1]
    got = [np.zeros_like(a) for a in ref]
    for first in range(world):
        r = renderer("cornell-srgb", 16, tile_first=first, tile_stride=world, tile_skew=1 if world > 1 else 0)
        r.import_sums(info, sums)
        r.import_spectral(sinfo, S, N)
        cont(r, 7)
        mask = tile_owner_mask(W, H, first, world, 1 if world > 1 else 0)
        for g, p in zip(got, state(r)):
            g[mask] = p[mask]
    assert same(got, ref)


# ---- 3. what is built on the bins ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def weights(scene, bins):
    d = one_shot(scene, bins)[0].scene.desc.contents
    return develop_weights(bins, float(d.lambda_min), float(d.lambda_step))


def downstream(r, scene, bins):
    w = weights(scene, bins)
    out = list(r.denoise_spectral(return_image=True)) + list(r.denoise_spectral(return_image=True, demodulate=True))
    out += [r.develop(w), r.develop(w, denoise={}), r.develop(w, demodulate=True)]
    return out


@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_filter_and_develop_after_a_resume_equal_those_of_the_one_shot_render(scene):
    """The noise estimate's batches are the launches: 4 + 4 + 4 on both sides (the checkpoint carries S2 and the batch count), so the variance that guides
    the filter has the same bits."""
    bins = 16
    whole, ref = one_shot(scene, bins)
    r = resumed(scene, bins, 4, noise=True)
    cont(r, 8)
    assert same(state(r), ref)
    assert np.array_equal(bits(r.noise()[1]), bits(whole.noise()[1])) and r.noise_summary[3] == 3
    got, want = downstream(r, scene, bins), downstream(whole, scene, bins)
    assert same(got, want)
    assert want[0].any() and want[3].any() and want[6].any()
    assert same(state(r), ref)                                 # they read only


# ---- 4. the transposition, value by value -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins,own", [(4, (0, 1, 0)), (8, (0, 1, 0)), (12, (1, 3, 1)), (16, (0, 1, 0)), (64, (0, 1, 0)), (64, (2, 3, 1))])
def test_export_after_import_returns_the_arrays(bins, own):
    """Any bit pattern in every bin of every pixel (the counts are a render's: the import checks them): what comes back is what went in, for the pixels the
    context owns, and zeros elsewhere.  An odd and an even bins / 4, a whole image and a third of it."""
    first, stride, skew = own
    info, sums, _, sinfo, _, N = part("cornell-srgb", bins, 5)
    g = np.random.default_rng(bins)
    S = g.integers(0, 2 ** 64, size=(H, W, bins), dtype=np.uint64).view(np.float64)      # NaNs with payloads, infinities, denormals, -0.0 among them
    S[0, 0, 0], S[H - 1, W - 1, bins - 1], S[7, 8, 1] = -0.0, np.inf, np.float64(np.nan)
    r = renderer("cornell-srgb", bins, tile_first=first, tile_stride=stride, tile_skew=skew)
    r.import_sums(info, sums)
    r.import_spectral(sinfo, S, N)
    got_info, got_S, got_N = r.export_spectral()
    assert bytes(got_info) == bytes(sinfo)
    mask = tile_owner_mask(W, H, first, stride, skew)
    assert mask.any() and np.array_equal(bits(got_S)[mask], bits(S)[mask]) and np.array_equal(got_N[mask], N[mask])
    assert not bits(got_S)[~mask].any() and not got_N[~mask].any()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    scene, bins = "cornell-srgb", 16
    info, sums, _, sinfo, S, N = part(scene, bins, 5)
    want12 = ol.Oracle(scene, texture=TEX).render(W, H, SPP, seed=SEED)

    def raw_import(r, si, s=S, n=N):                           # (past the binding's own check of the shapes)
        s, n = np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(n, dtype=np.uint32)
        r._check(r._lib.ssx_spectral_import(r._ctx, C.byref(si), s.ctypes.data, n.ctypes.data))

    def changed(**kw):
        si = type(sinfo).from_buffer_copy(sinfo)
        for k, v in kw.items():
            setattr(si, k, v)
        return si

    # state: spectral output off; nothing imported; rendered since the import; a render running
    off = renderer(scene, 0)
    off.import_sums(info, sums)
    refused(lambda: raw_import(off, sinfo), _capi.SSX_ERR_STATE, "spectral output is off")
    r = renderer(scene, bins)
    refused(lambda: raw_import(r, sinfo), _capi.SSX_ERR_STATE, "ssx_sums_import")
    start(r, 5)
    refused(lambda: raw_import(r, sinfo), _capi.SSX_ERR_STATE, "ssx_sums_import")      # its own render's sums: no import underneath
    r.import_sums(info, sums)
    cont(r, 1)
    refused(lambda: raw_import(r, changed(done_spp=6)), _capi.SSX_ERR_STATE, "rendered since")
    r.import_sums(info, sums)
    r._check(r._lib.ssx_render_continue(r._ctx, 1 << 20))
    try:
        refused(lambda: raw_import(r, sinfo), _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop()
        r.render_wait()

    # arguments, each named; ssx_sums_import alone leaves the bins invalid, and so does every refusal
    r = renderer(scene, bins)
    r.import_sums(info, sums)
    refused(r.spectral_read, _capi.SSX_ERR_STATE, "ssx_sums_import")
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
    lone = three_ranks_merged()[5]
    one_off = N.copy()
    one_off[H - 1, W - 1, 2] += 1                              # the last pixel of the ragged corner tile
    one_less = N.copy()
    one_less[0, 0, 0] -= 1 if one_less[0, 0, 0] else -1
    moved = N.copy()                                           # the sum kept, across two pixels: each of them is off
    moved[3, 4, 0] += 1; moved[3, 5, 0] -= 1 if moved[3, 5, 0] else -1
    for what, call, words in (
            ("width", lambda: raw_import(r, changed(width=W + 1)), ("size differs",)),
            ("height", lambda: raw_import(r, changed(height=H - 1)), ("size differs",)),
            ("bins", lambda: raw_import(r, changed(bins=8), S[..., :8], N[..., :2]), ("bins differs",)),
            ("done_spp", lambda: raw_import(r, changed(done_spp=6)), ("done_spp differs",)),
            ("lambda_min", lambda: raw_import(r, changed(lambda_min=up(sinfo.lambda_min))), ("lambda_min differs",)),
            ("bin_width", lambda: raw_import(r, changed(bin_width=up(sinfo.bin_width))), ("bin_width differs",)),
            ("struct_size", lambda: raw_import(r, changed(struct_size=sinfo.struct_size + 4)), ("struct_size",)),
            ("a count one too many", lambda: raw_import(r, sinfo, S, one_off), ("counts",)),
            ("a count one too few", lambda: raw_import(r, sinfo, S, one_less), ("counts",)),
            ("a count moved to the next pixel", lambda: raw_import(r, sinfo, S, moved), ("counts",)),
            ("one rank's unmerged export", lambda: raw_import(r, sinfo, *lone), ("counts", "merge"))):
        refused(call, _capi.SSX_ERR_ARG, "ssx_spectral_import", *words)
        refused(r.spectral_read, _capi.SSX_ERR_STATE, "ssx_sums_import")
        refused(lambda: r.denoise_spectral(), _capi.SSX_ERR_STATE)
    assert r.done_spp() == 5 and np.array_equal(bits(r.export_sums()[1]), bits(sums))          # the pixel sums are what ssx_sums_import set up
    # still directly on top of the import: the right arrays are taken
    raw_import(r, sinfo)
    assert same(r.export_spectral()[1:], (S, N))
    # ... and after a refusal a continue renders normally: the oracle's image, no bins
    r = renderer(scene, bins)
    r.import_sums(info, sums)
    refused(lambda: raw_import(r, sinfo, S, one_off), _capi.SSX_ERR_ARG, "counts")
    cont(r, 7)
    assert np.array_equal(bits(r.xyza), bits(want12))
    refused(r.spectral_read, _capi.SSX_ERR_STATE)
    # the binding's own check of the shapes
    with pytest.raises(ValueError):
        r.import_spectral(sinfo, S[..., :8], N)


# ---- 6. CLI -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_checkpoint_of_three_devices_is_resumed_by_two_with_the_bins(tmp_path):
    """SSX_TEST_ONE_GPU=1: all contexts on device 0 (tests/test_cli.py).  Three devices write the checkpoint, two resume it; the resumed render's bin count is
    the checkpoint's."""
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    common = ["-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "--seed=%d" % SEED, "--texture=data/scenes/test-img.png"]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True, env=env)
    ck, ck12, plain, npy5, npy12, png = (str(tmp_path / n) for n in ("c.ckpt", "c12.ckpt", "plain.ckpt", "five.npy", "twelve.npy", "o.png"))
    p = run("-spp=5", "-o=" + png, "--gpus=3", "--checkpoint=" + ck, "--spectral-output=" + npy5)
    assert p.returncode == 0, p.stderr
    *_, sinfo, S, N = load_checkpoint_file_spectral(ck)
    assert (sinfo.bins, sinfo.done_spp) == (16, 5) and same((S, N), part("cornell-srgb", 16, 5)[4:])
    p = run("-spp=%d" % SPP, "-o=" + png, "--gpus=2", "--resume=" + ck, "--spectral-output=" + npy12, "--checkpoint=" + ck12)
    assert p.returncode == 0 and "5 samples per pixel done, 12 wanted" in p.stderr, p.stderr
    ref = one_shot("cornell-srgb", 16)[1]
    got = np.load(npy12)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(ref[0]))
    *_, sinfo, S, N = load_checkpoint_file_spectral(ck12)                                       # the resumed render's own checkpoint carries them on
    assert (sinfo.bins, sinfo.done_spp) == (16, SPP) and same((S, N), ref[1:3])
    # without spectral options the same file resumes to the one-shot image, and writes the checkpoint it always wrote
    one, res = str(tmp_path / "one.png"), str(tmp_path / "res.png")
    p = run("-spp=%d" % SPP, "-o=" + res, "--resume=" + ck, "--checkpoint=" + plain)
    assert p.returncode == 0 and open(plain, "rb").read(8) == b"SSXCKPT1", p.stderr
    p = run("-spp=%d" % SPP, "-o=" + one)
    assert p.returncode == 0 and open(res, "rb").read() == open(one, "rb").read(), p.stderr
    # a checkpoint without bins, or with another count than asked for: refused before anything renders
    p = run("-spp=%d" % SPP, "-o=" + res, "--resume=" + plain, "--spectral-output=" + npy5)
    assert p.returncode == 255 and "cannot be combined with `--resume` of a checkpoint without wavelength bins" in p.stderr, p.stderr
    p = run("-spp=%d" % SPP, "-o=" + res, "--resume=" + ck, "--spectral-output=" + npy5, "--spectral-bins=8")
    assert p.returncode == 255 and "cannot be combined with `--resume` of a checkpoint with another bin count" in p.stderr, p.stderr
