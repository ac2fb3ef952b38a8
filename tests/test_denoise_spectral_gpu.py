"""Denoising the spectral bins on the GPU (include/ssx.h "Denoising the spectral bins"): ssx_denoise_channels against the numpy restatement
(tests/denoise_spectral_ref.py), ssx_denoise_spectral against its pieces and the restatement, and the state rules, refusals, quality condition and CLI
around them.  "equals" is np.array_equal on the integer views (bit for bit).  Image sizes as in test_denoise_gpu.py: 72 x 40 (ragged workgroups in both
directions, a level-6 step wider than the image), 20 x 12, 16 x 8, 5 x 3 (smaller than the kernel's footprint)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_spectral_ref as sr
from simple_spectral_amd import Renderer, _capi
from test_denoise_gpu import CLI, OTHER, ROOT, SEED, SIZES, refused, render, renderer, same

pytestmark = pytest.mark.gpu
bits = sr.bits
F = np.float32
SIGMAS = (dict(sigma_l=dr.DEFAULTS["sigma_l"], sigma_a=dr.DEFAULTS["sigma_a"]), OTHER)
CHANNELS = (1, 3, 5, 80)


@functools.lru_cache(maxsize=None)
def filter_context():
    return renderer("cornell-srgb", SIZES[3])


# ---- 1. the extra channels as a pure function ------------------------------------------------------------------------------------------------------------

extras_with_specials = dr.extras_with_specials          # (shared with tests/test_pipeline_matrix_gpu.py)


@pytest.mark.parametrize("res", SIZES)
def test_the_channels_equal_the_restatement(res):
    W, H = res
    c, var, prim, albedo = dr.synthetic(W, H, seed=W * 100 + H)
    e = extras_with_specials(c, var, W + H)
    r = filter_context()
    for sig in SIGMAS:
        ref = (np.ascontiguousarray(c), var, e)                       # the channels are independent: E < 80 is the first E of the 80
        for levels in range(1, 7):
            ref = sr.channels_level(ref[0], ref[1], prim, albedo, ref[2], 1 << (levels - 1), **sig)
            image = r.denoise_images(c, var, prim, albedo, levels=levels, return_variance=True, **sig)
            assert same(image, ref[:2]), (res, levels, sig)
            for E in CHANNELS:
                got = r.denoise_channels(c, var, prim, albedo, e[..., :E], levels=levels, return_image=True, **sig)
                assert got[0].shape == (H, W, E)
                diff = int((bits(got[0]) != bits(ref[2][..., :E])).sum())
                assert diff == 0, (res, levels, sig, E, diff)
                assert same(got[1:], image), (res, levels, sig, E)    # xyza_out and var_out are ssx_denoise_images'
            xyz = r.denoise_channels(c, var, prim, albedo, c[..., :3], levels=levels, **sig)
            assert np.array_equal(bits(xyz), bits(image[0][..., :3])), (res, levels, sig)   # the two kernels' weights, held against each other
    default = r.denoise_channels(c, var, prim, albedo, e[..., :5])                           # the defaults, xyza_out and var_out NULL
    assert np.array_equal(bits(default), bits(sr.atrous_channels(c, var, prim, albedo, e[..., :5], **dr.DEFAULTS)[2]))


# ---- 2. the spectral bins from the context's own state -----------------------------------------------------------------------------------------------------

def spectral_render(scene, res, bins, spp=16, per_launch=4, r=None):
    r = r or renderer(scene, res)
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    image = render(r, spp, spp_per_launch=per_launch)
    return r, image


@pytest.mark.parametrize("res", SIZES[:2])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb", "custom"])
def test_denoise_spectral_equals_the_pieces_and_the_restatement(scene, res):
    r = None
    for B in (4, 16, 64):
        r, image = spectral_render(scene, res, B, r=r)
        info, mean, counts, sums = r.spectral_read(sums=True)
        assert info.done_spp == 16 and (counts.sum(axis=2) == 16).all()
        _, v = r.noise()
        var = dr.variance_in_image_units(v)
        g = r.guides()
        e0 = sr.spectral_channels(sums, counts, 16)
        assert e0.shape[2] == B + B // 4
        for kw in (dict(dr.DEFAULTS), dict(levels=3, **OTHER)):
            own = r.denoise_spectral(return_image=True, **kw)
            eL = r.denoise_channels(image, var, g["prim"], g["albedo"], e0, **kw)
            pieces = sr.spectral_ratio(eL, B)
            ref = sr.denoise_spectral(sums, counts, 16, image, var, g["prim"], g["albedo"], **kw)
            assert np.array_equal(bits(own[0]), bits(pieces)), (scene, res, B, kw)
            assert same(own, ref), (scene, res, B, kw)
            assert same(own[1:], r.denoise(return_variance=True, **kw))                     # its image is Renderer.denoise's
            assert np.array_equal(bits(r.denoise_spectral(**kw)), bits(own[0]))             # xyza_out and var_out NULL
        assert not np.array_equal(bits(own[0]), bits(mean)) and np.isfinite(own[0]).all()


# ---- 3. state ------------------------------------------------------------------------------------------------------------------------------------------

def test_it_reads_only():
    res = SIZES[1]
    r, _ = spectral_render("cornell-srgb", res, 8)
    before, before_bins = r.export_sums(), r.spectral_read(sums=True)
    a = r.denoise_spectral(return_image=True)
    b = r.denoise_spectral(return_image=True)
    assert same(a, b)
    after, after_bins = r.export_sums(), r.spectral_read(sums=True)
    assert np.array_equal(bits(before[1]), bits(after[1])) and np.array_equal(bits(before[2]), bits(after[2])) and bytes(before[0]) == bytes(after[0])
    assert same(before_bins[1:], after_bins[1:])
    r.read_framebuffer()
    r.render_continue(16); r.render_wait()
    one_shot = renderer("cornell-srgb", res)
    one_shot.set_spectral_bins(8)
    assert np.array_equal(bits(r.xyza), bits(render(one_shot, 32)))                        # continue after it: the bits of a one-shot render ...
    assert same(r.spectral_read(sums=True)[1:], one_shot.spectral_read(sums=True)[1:])     # ... in the image and in ssx_spectral_read


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    res = SIZES[1]
    W, H = res
    r = renderer("cornell-srgb", res)
    r.set_noise_estimate(True)
    render(r, 8, spp_per_launch=4)
    refused(r.denoise_spectral, _capi.SSX_ERR_STATE, "spectral output is off")
    plain = renderer("cornell-srgb", res)
    plain.set_spectral_bins(8)
    render(plain, 8, spp_per_launch=4)
    refused(plain.denoise_spectral, _capi.SSX_ERR_STATE, "noise estimate is off")
    r.set_spectral_bins(8)
    refused(r.denoise_spectral, _capi.SSX_ERR_STATE, "bin count")                          # switched on after the render: no bins yet
    render(r, 8, spp_per_launch=8)
    refused(r.denoise_spectral, _capi.SSX_ERR_STATE, "1 batch")
    half = renderer("cornell-srgb", res, tile_stride=2)
    half.set_noise_estimate(True); half.set_spectral_bins(8)
    render(half, 8, spp_per_launch=4)
    refused(half.denoise_spectral, _capi.SSX_ERR_STATE, "tile_stride")
    render(r, 8, spp_per_launch=4)
    assert r.denoise_spectral().shape == (H, W, 8)
    for levels in (0, 7):
        refused(lambda: r.denoise_spectral(levels=levels), _capi.SSX_ERR_ARG, "levels")
    info, sums, s2 = r.export_sums()
    r.import_sums(info, sums, s2)                                                           # the noise estimate is carried on, the bins are not
    assert r.denoise().shape == (H, W, 4)
    refused(r.denoise_spectral, _capi.SSX_ERR_STATE, "ssx_sums_import")
    # the pure function
    c, var, prim, albedo = dr.synthetic(W, H, 1)
    for E in (0, 81):
        refused(lambda: r.denoise_channels(c, var, prim, albedo, np.zeros((H, W, E), dtype=F)), _capi.SSX_ERR_ARG, "channels")
    out, e = np.zeros((H, W, 4), dtype=F), np.zeros((H, W, 3), dtype=F)
    p = Renderer._denoise_params(5, 1.0, 0.1)
    args = [r._ctx, C.byref(p), W, H, c.ctypes.data, var.ctypes.data, prim.ctypes.data, albedo.ctypes.data, 3]
    assert r._lib.ssx_denoise_channels(*args, None, out.ctypes.data, None, e.ctypes.data) == _capi.SSX_ERR_ARG and b"extra" in r._lib.ssx_last_error(r._ctx)
    assert r._lib.ssx_denoise_channels(*args, e.ctypes.data, out.ctypes.data, None, None) == _capi.SSX_ERR_ARG and b"extra_out" in r._lib.ssx_last_error(r._ctx)
    # no scene uploaded: a bare context serves the pure function and refuses the other
    lib, ctx = _capi.hip_lib(), C.c_void_p()
    assert lib.ssx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.ssx_denoise_spectral(ctx, None, None, None, None) == _capi.SSX_ERR_STATE and b"no scene" in lib.ssx_last_error(ctx)
        args[0] = ctx
        x = np.ascontiguousarray(c[..., :3])
        assert lib.ssx_denoise_channels(*args, x.ctypes.data, None, None, e.ctypes.data) == 0
        assert np.array_equal(bits(e), bits(dr.atrous(c, var, prim, albedo, **dr.DEFAULTS)[0][..., :3]))
    finally:
        lib.ssx_destroy(ctx)


# ---- 5. quality ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_the_filtered_bins_are_closer_to_a_1024_spp_render(scene, B):
    """72 x 40, 16 spp in 4 batches, default parameters, against the unfiltered mean at 1024 spp of the same seed: the RMSE over all pixels and bins of the
    filtered spectrum must be below that of the unfiltered 16-spp mean -- a condition, not a tolerance.  The four pairs are recorded in DESIGN.md section 13."""
    r, _ = spectral_render(scene, SIZES[0], B)
    mean16 = r.spectral_read()[1]
    filtered = r.denoise_spectral()
    ref = renderer(scene, SIZES[0])
    ref.set_spectral_bins(B)
    render(ref, 1024)
    mean1024 = ref.spectral_read()[1].astype(np.float64)
    rmse = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - mean1024) ** 2)))
    before, after = rmse(mean16), rmse(filtered)
    print("QUALITY %s B=%d: RMSE unfiltered %.6g, filtered %.6g" % (scene, B, before, after))
    assert after < before


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_filtered_bins(tmp_path):
    W, H = SIZES[1]
    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png"]
    r, _ = spectral_render("cornell-srgb", (W, H), 8, per_launch=2)                        # ceil(16 / 8), --denoise's launch rule
    want, want_image, _ = r.denoise_spectral(levels=4, sigma_l=2.0, sigma_a=0.2, return_image=True)
    assert not np.array_equal(bits(want), bits(r.spectral_read()[1]))
    r.save(str(tmp_path / "plain.pfm"))                                                    # the unfiltered image
    r.framebuffer = r.scene.xyza_to_srgba(want_image)
    r.save(str(tmp_path / "filtered.pfm"))
    outs = []
    for n, env in ((0, {}), (1, {"SSX_TEST_ONE_GPU": "1"})):
        pfm, npy = str(tmp_path / ("o%d.pfm" % n)), str(tmp_path / ("s%d.npy" % n))
        extra = ["--gpus=2"] if n else []
        p = subprocess.run(common + extra + ["-o=" + pfm, "--spectral-output=" + npy, "--spectral-bins=8", "--spectral-denoise", "--denoise-levels=4", "--denoise-sigma=2,0.2"],
                           cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr
        a = np.load(npy)
        assert a.dtype == np.float32 and a.shape == (H, W, 8)
        outs.append(a)
        assert open(pfm, "rb").read() == open(str(tmp_path / "plain.pfm"), "rb").read()    # without --denoise the image is the plain one
    assert np.array_equal(bits(outs[0]), bits(want))                                       # the array Python returns
    assert np.array_equal(bits(outs[1]), bits(want))                                       # the multi-device host path: the same bits
    pfm, npy = str(tmp_path / "both.pfm"), str(tmp_path / "both.npy")
    p = subprocess.run(common + ["-o=" + pfm, "--spectral-output=" + npy, "--spectral-bins=8", "--spectral-denoise", "--denoise", "--denoise-levels=4", "--denoise-sigma=2,0.2"],
                       cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(bits(np.load(npy)), bits(want)) and open(pfm, "rb").read() == open(str(tmp_path / "filtered.pfm"), "rb").read()
