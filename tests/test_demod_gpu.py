"""Demodulated denoising on the GPU (include/ssx.h "Demodulated denoising"): ssx_albedo_bins against the oracle's restatement (tests/demod_ref.py),
ssx_denoise_spectral_demod against the composition the definition states -- numpy divide, the existing pure ssx_denoise_channels with a zero albedo guide,
numpy multiply --, ssx_spectral_develop_demod against ssx_develop_images, the state rules and refusals, and the quality conditions.  "equals" is
np.array_equal on the integer views (bit for bit).  Images are 42 x 23 as in test_develop_gpu.py: six tile columns and three rows, the last of each ragged."""
import functools
import os
import subprocess

import numpy as np
import pytest

import crafted
import demod_ref as mr
import denoise_ref as dr
import denoise_spectral_ref as sr
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import develop_weights
from test_develop_gpu import CLI, H, ROOT, SEED, SPP, TEX, W, lambda_range, random_weights, refused, save_developed, start
from test_denoise_gpu import render, renderer as sized_renderer

pytestmark = pytest.mark.gpu
bits = sr.bits
F = np.float32
SCENES = ("cornell-srgb", "plane-srgb", "crafted")


@functools.lru_cache(maxsize=None)
def crafted_scene():
    """The Cornell box with textures of many sizes on its quads, seen from further back through a wide lens: textured quads in the middle, the box's outside
    and the void around it.  ONE object for the module: `desc()` points into the scene's own arrays."""
    c = crafted.many_textures_scene()
    c.set_camera((150.0, 400.0, -900.0), (300.0, 250.0, 300.0), up=(0, 1, 0), vfov_deg=38.0, aspect=W / H)
    return c


@functools.lru_cache(maxsize=None)
def oracle(scene):
    return crafted_scene().oracle() if scene == "crafted" else ol.Oracle(scene, texture=TEX)


def renderer(scene, **opts):
    r = Renderer(Options(scene_name="cornell-srgb" if scene == "crafted" else scene, res=(W, H), seed=SEED, texture=TEX, jit_pass1=False, **opts))
    if scene == "crafted":
        r.upload_scene_desc(crafted_scene().desc(oracle(scene)))
    return r


@functools.lru_cache(maxsize=None)
def context(scene):
    return renderer(scene)


@functools.lru_cache(maxsize=None)
def reference_bins(scene, B, K):
    rho = mr.albedo_bins(oracle(scene), W, H, B, K)
    rho.setflags(write=False)
    return rho


def own_weights(r, B):
    lmin, lstep = lambda_range(r)
    return develop_weights(B, lmin, lstep)


def rendered(scene, B, spp=SPP, per_launch=10):
    r = renderer(scene)
    r.set_noise_estimate(True)
    r.set_spectral_bins(B)
    image = start(r, spp, spp_per_launch=per_launch)                      # 37 samples in four batches: 10 / 10 / 10 / 7
    return r, image


# ---- 1. the albedo bins ------------------------------------------------------------------------------------------------------------------------------------

def test_the_crafted_scene_has_a_miss_and_textured_quads():
    g = dr.guides_ref(oracle("crafted"), W, H)
    assert (g["prim"] == dr.MISS).any() and (g["prim"] != dr.MISS).any()
    rho = reference_bins("crafted", 4, 1)
    hit = rho[g["prim"] != dr.MISS]
    assert len(np.unique(bits(hit[:, 0]))) > 20                            # a texture, not a handful of constant albedos
    assert not bits(rho[g["prim"] == dr.MISS]).any()                       # a miss is +0 in every bin


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("B", [4, 16, 64])
@pytest.mark.parametrize("scene", SCENES)
def test_albedo_bins_equal_the_restatement(scene, B, K):
    r = context(scene)
    got = r.albedo_bins(B, supersample=K)
    want = reference_bins(scene, B, K)
    assert got.shape == (H, W, B) and got.dtype == np.float32
    diff = int((bits(got) != bits(want)).sum())
    assert diff == 0, (scene, B, K, diff)
    assert np.array_equal(bits(r.albedo_bins(B, supersample=K)), bits(got))                  # the cached call
    if B == 4 and K == 1:
        assert np.array_equal(bits(got), bits(r.guides()["albedo"]))                         # lambda_0 is lambda_g
    if K > 1:
        assert not np.array_equal(bits(got), bits(r.albedo_bins(B, supersample=1)))          # the sub-pixel rays do see other texels


def test_an_odd_number_of_sub_bins_takes_the_other_instance():
    """B = 12: M = 3, the one-sub-bin instance of the kernel (an even M runs the two-sub-bin one)."""
    got = context("plane-srgb").albedo_bins(12, supersample=2)
    assert np.array_equal(bits(got), bits(mr.albedo_bins(oracle("plane-srgb"), W, H, 12, 2)))


# ---- 2. the demodulated spectral filter ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [4, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_denoise_spectral_demod_equals_the_composition(scene, B):
    r, image = rendered(scene, B)
    info, _, counts, sums = r.spectral_read(sums=True)
    assert info.done_spp == SPP
    var = dr.variance_in_image_units(r.noise()[1])
    prim = r.guides()["prim"]
    e0 = sr.spectral_channels(sums, counts, SPP)
    wc = own_weights(r, B)
    pure = lambda c, v, p, a, e, levels, sigma_l: r.denoise_channels(c, v, p, a, e, levels=levels, sigma_l=sigma_l, sigma_a=0.5, return_image=True)
    for K, floor, sigma_l in ((2, mr.DEFAULT_FLOOR, mr.DEFAULT_SIGMA_L), (1, 0.25, 4.0)):
        rho = r.albedo_bins(B, supersample=K)
        for L in (1, 2, 5):                                                                   # both kernel shapes of the channels: LDS-staged levels and gathers
            got = r.denoise_spectral(levels=L, sigma_l=sigma_l, return_image=True, demodulate=dict(supersample=K, albedo_floor=floor))
            want = mr.denoise_spectral_demod(e0, image, var, prim, rho, wc, floor=floor, levels=L, sigma_l=sigma_l, channels=pure)
            for name, g, w in zip(("mean_out", "xyza_out", "var_out"), got, want):
                assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (scene, B, K, L, name, int((bits(g) != bits(w)).sum()))
        if B == 4:                                                                            # ... and once against numpy alone (the filter's restatement)
            want = mr.denoise_spectral_demod(e0, image, var, prim, rho, wc, floor=floor, levels=2, sigma_l=sigma_l)
            got = r.denoise_spectral(levels=2, sigma_l=sigma_l, return_image=True, demodulate=dict(supersample=K, albedo_floor=floor))
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
    default = r.denoise_spectral(demodulate=True)                                             # the defaults; xyza_out and var_out NULL
    want = mr.denoise_spectral_demod(e0, image, var, prim, r.albedo_bins(B), wc, channels=pure)
    assert np.array_equal(bits(default), bits(want[0]))
    assert np.array_equal(bits(r.denoise_spectral(demodulate=True, sigma_a=123.0)), bits(default))   # sigma_a is ignored
    assert not np.array_equal(bits(default), bits(r.denoise_spectral()))                     # and the plain mode is another filter


# ---- 3. develop --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [8, 64])
def test_develop_demod_equals_develop_images_of_the_filtered_bins(B):
    r, _ = rendered("plane-srgb", B)
    for kw, dm in (({}, True), (dict(levels=3, sigma_l=4.0), dict(supersample=4, albedo_floor=0.125))):
        filtered = r.denoise_spectral(demodulate=dm, **kw)
        for channels in (3, 16):
            w = random_weights(channels, B, channels + 1)
            got = r.develop(w, denoise=kw, demodulate=dm)
            assert np.array_equal(bits(got), bits(r.develop_images(filtered, w))), (B, kw, channels)
        assert np.array_equal(bits(r.denoise_spectral(demodulate=dm, **kw)), bits(filtered))
    assert not np.array_equal(bits(r.develop(w, denoise=kw)), bits(got))                     # the plain denoised source differs


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------------------------------

def test_it_reads_only_and_a_continue_gives_the_bits_of_one_render():
    r, _ = rendered("cornell-srgb", 8, spp=16, per_launch=8)
    before, before_bins = r.export_sums(), r.spectral_read(sums=True)
    r.read_framebuffer()
    before_image = r.xyza.copy()
    a = r.denoise_spectral(return_image=True, demodulate=True)
    r.develop(random_weights(3, 8, 1), demodulate=True)
    b = r.denoise_spectral(return_image=True, demodulate=True)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))
    after, after_bins = r.export_sums(), r.spectral_read(sums=True)
    assert np.array_equal(bits(before[1]), bits(after[1])) and np.array_equal(bits(before[2]), bits(after[2])) and bytes(before[0]) == bytes(after[0])
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before_bins[1:], after_bins[1:]))
    r.read_framebuffer()
    assert np.array_equal(bits(r.xyza), bits(before_image))
    r.render_continue(21); r.render_wait()
    one = renderer("cornell-srgb")
    one.set_spectral_bins(8)
    assert np.array_equal(bits(r.xyza), bits(start(one)))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(r.spectral_read(sums=True)[1:], one.spectral_read(sums=True)[1:]))


def test_a_new_scene_drops_the_cached_bins():
    r = renderer("cornell-srgb")
    first = r.albedo_bins(8)
    r.upload_scene_desc(crafted_scene().desc(oracle("crafted")))
    assert np.array_equal(bits(r.albedo_bins(8)), bits(reference_bins("crafted", 8, 2))) and not np.array_equal(bits(first), bits(reference_bins("crafted", 8, 2)))


def test_refusals():
    rgb = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=SEED, texture=TEX, jit_pass1=False, render_mode="rgb"))
    refused(lambda: rgb.albedo_bins(4), _capi.SSX_ERR_STATE, "SSX_MODE_RGB")
    r = renderer("cornell-srgb")
    r.set_noise_estimate(True)
    start(r, 8, spp_per_launch=4)
    refused(lambda: r.denoise_spectral(demodulate=True), _capi.SSX_ERR_STATE, "spectral output is off")
    refused(lambda: r.develop(random_weights(3, 4, 1), demodulate=True), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(8)
    start(r, 8, spp_per_launch=4)
    assert r.denoise_spectral(demodulate=True).shape == (H, W, 8)
    for K in (0, 3, 8):
        refused(lambda: r.albedo_bins(8, supersample=K), _capi.SSX_ERR_ARG, "supersample")
        refused(lambda: r.denoise_spectral(demodulate=dict(supersample=K)), _capi.SSX_ERR_ARG, "supersample")
    for bins in (0, 6, 68):
        refused(lambda: r.albedo_bins(bins), _capi.SSX_ERR_ARG, "multiple of 4")
    for floor in (0.0, -1.0, float("inf"), float("nan")):
        refused(lambda: r.denoise_spectral(demodulate=dict(albedo_floor=floor)), _capi.SSX_ERR_ARG, "albedo_floor")
    w = own_weights(r, 8)
    zero_row = w.copy(); zero_row[1] = 0
    refused(lambda: r.denoise_spectral(demodulate=dict(weights_xyz=zero_row)), _capi.SSX_ERR_ARG, "denominator")
    refused(lambda: r.denoise_spectral(demodulate=dict(weights_xyz=-w)), _capi.SSX_ERR_ARG, "denominator")
    refused(lambda: r.develop(random_weights(3, 8, 1), demodulate=dict(weights_xyz=zero_row)), _capi.SSX_ERR_ARG, "denominator")
    refused(lambda: r.denoise_spectral(levels=7, demodulate=True), _capi.SSX_ERR_ARG, "levels")
    refused(lambda: r._check(r._lib.ssx_denoise_spectral_demod(r._ctx, None, None, None, None, None, None)), _capi.SSX_ERR_ARG, "weights_xyz")
    assert r._lib.ssx_denoise_spectral_demod(r._ctx, None, None, w.ctypes.data, None, None, None) == 0      # NULL parameters: the defaults
    one_batch = renderer("cornell-srgb")
    one_batch.set_noise_estimate(True); one_batch.set_spectral_bins(8)
    start(one_batch, 8, spp_per_launch=8)
    refused(lambda: one_batch.denoise_spectral(demodulate=True), _capi.SSX_ERR_STATE, "1 batch")                # ssx_denoise_spectral's rules


def test_the_kept_channel_albedo_follows_its_inputs():
    """r~_c and the zero guide are kept in the context from call to call: every input they were made from -- weights, floor, K, the scene -- must replace them."""
    r, image = rendered("plane-srgb", 8)
    _, _, counts, sums = r.spectral_read(sums=True)
    var, prim, e0 = dr.variance_in_image_units(r.noise()[1]), r.guides()["prim"], sr.spectral_channels(sums, counts, SPP)
    w1 = own_weights(r, 8)
    w2 = (w1 * np.linspace(0.5, 2.0, 8, dtype=F)[None, :]).astype(F)
    for K, floor, w in ((2, 0.0625, w1), (2, 0.0625, w1), (2, 0.0625, w2), (2, 0.5, w2), (1, 0.5, w2), (2, 0.0625, w1)):
        got = r.denoise_spectral(levels=2, return_image=True, demodulate=dict(supersample=K, albedo_floor=floor, weights_xyz=w))
        want = mr.denoise_spectral_demod(e0, image, var, prim, r.albedo_bins(8, supersample=K), w, floor=floor, levels=2)
        assert all(np.array_equal(bits(g), bits(x)) for g, x in zip(got, want)), (K, floor)
        r.albedo_bins(8, supersample=4)                                                        # another request in between: the bins are computed again


# ---- 5. the several-device route, through the command line -------------------------------------------------------------------------------------------------

def test_cli_two_devices_give_the_bits_of_one(tmp_path):
    B, K = 8, 4
    common = [CLI, "-s=plane-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "--spectral-bins=%d" % B,
              "--spectral-denoise", "--denoise-levels=3", "--denoise-sigma=2,0.2", "--demodulate=%d" % K]
    r, _ = rendered("plane-srgb", B, spp=16, per_launch=2)                                     # ceil(16 / 8): --spectral-denoise's launch rule
    dm = dict(supersample=K)
    want, want_image, _ = r.denoise_spectral(levels=3, sigma_l=2.0, return_image=True, demodulate=dm)
    assert not np.array_equal(bits(want), bits(r.denoise_spectral(levels=3, sigma_l=2.0, sigma_a=0.2)))
    r.framebuffer = r.scene.xyza_to_srgba(want_image)
    r.save(str(tmp_path / "filtered.pfm"))
    save_developed(r, r.develop(own_weights(r, B), denoise=dict(levels=3, sigma_l=2.0), demodulate=dm), str(tmp_path / "developed.pfm"))
    filtered, developed = (open(str(tmp_path / n), "rb").read() for n in ("filtered.pfm", "developed.pfm"))
    rho = r.albedo_bins(B, supersample=K)
    for n, (extra, env) in enumerate((([], {}), (["--gpus=2"], {"SSX_TEST_ONE_GPU": "1"}))):
        pfm, npy, dev, alb = (str(tmp_path / ("%s%d.%s" % (k, n, e))) for k, e in (("o", "pfm"), ("s", "npy"), ("d", "pfm"), ("a", "npy")))
        p = subprocess.run(common + extra + ["-o=" + pfm, "--denoise", "--spectral-output=" + npy, "--develop-output=" + dev, "--albedo-output=" + alb],
                           cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr
        got = np.load(npy)
        assert got.dtype == np.float32 and got.shape == (H, W, B) and np.array_equal(bits(got), bits(want)), extra
        assert open(pfm, "rb").read() == filtered and open(dev, "rb").read() == developed, extra
        assert np.array_equal(bits(np.load(alb)), bits(rho)), extra
    p = subprocess.run(common[:-5] + ["-o=/dev/null", "--demodulate"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--spectral-denoise" in p.stderr                              # a mode of that filter
    p = subprocess.run(common[:-1] + ["-o=/dev/null", "--spectral-output=/dev/null", "--demodulate=3"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--demodulate" in p.stderr


def test_cli_four_devices_with_unequal_shares_give_the_bits_of_one(tmp_path):
    """20 x 12: 3 x 2 tiles, the last column and the upper row ragged; four devices own 2, 2, 1 and 1 of them (tile_skew = 1).  Every gather of the several-device
    routes -- image, variance, sums and counts, the checkpoint's bins -- against the same command line on one device: the files byte for byte."""
    from simple_spectral_amd.renderer import load_checkpoint_file_spectral
    B = 8
    common = [CLI, "-s=plane-srgb", "-w=20", "-h=12", "-spp=16", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "--spectral-bins=%d" % B, "--denoise",
              "--spectral-denoise", "--denoise-levels=3", "--denoise-sigma=2,0.2", "--demodulate=2"]
    names = ("o.pfm", "s.npy", "d.pfm", "a.npy", "c.ckpt")
    files = []
    for n, (extra, env) in enumerate((([], {}), (["--gpus=4"], {"SSX_TEST_ONE_GPU": "1"}))):
        pfm, npy, dev, alb, ck = (str(tmp_path / ("%d%s" % (n, name))) for name in names)
        p = subprocess.run(common + extra + ["-o=" + pfm, "--spectral-output=" + npy, "--develop-output=" + dev, "--albedo-output=" + alb, "--checkpoint=" + ck],
                           cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr
        *_, sinfo, S, N = load_checkpoint_file_spectral(ck)
        files.append([open(f, "rb").read() for f in (pfm, npy, dev, alb)] + [(sinfo.bins, sinfo.done_spp), S, N])
    one, four = files
    for name, a, b in zip(names, one[:4], four[:4]):
        assert len(a) > 0 and a == b, name
    assert np.load(str(tmp_path / "1s.npy")).shape == (12, 20, B)
    assert one[4] == four[4] == (B, 16)
    assert S.shape == (12, 20, B) and N.shape == (12, 20, B // 4) and N.any()
    assert np.array_equal(bits(one[5]), bits(four[5])) and np.array_equal(one[6], four[6])


# ---- 6. quality ----------------------------------------------------------------------------------------------------------------------------------------------

QRES, QSEED, QREF_SEED = (72, 40), 3, 1234          # tests/test_denoise_cpu.py's renders: the Y figures here are that test's


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_quality_against_a_1024_spp_render(scene, B):
    """72 x 40, 16 spp in 4 batches, the defaults of either mode, against 1024 spp: RMSE of Y over the pixels and of the bins over pixels and bins.  plane-srgb:
    the demodulated filter must beat the plain one in both; cornell-srgb (a constant albedo per primitive: demodulation is a scale per primitive there): it must
    not be worse than no filter; its figures against the plain filter are printed.  Conditions, not tolerances; the figures are in DESIGN.md section 15."""
    r = sized_renderer(scene, QRES)
    r.options.seed = QSEED
    r.set_noise_estimate(True); r.set_spectral_bins(B)
    image = render(r, 16, spp_per_launch=4, seed=QSEED)
    mean16 = r.spectral_read()[1]
    plain = r.denoise_spectral(return_image=True)
    demod = r.denoise_spectral(return_image=True, demodulate=True)
    ref = sized_renderer(scene, QRES)
    ref.set_spectral_bins(B)
    ref_image = render(ref, 1024, seed=QREF_SEED)
    ref_bins = ref.spectral_read()[1]
    y = {k: rmse(v[..., 1], ref_image[..., 1]) for k, v in (("unfiltered", image), ("plain", plain[1]), ("demodulated", demod[1]))}
    b = {k: rmse(v, ref_bins) for k, v in (("unfiltered", mean16), ("plain", plain[0]), ("demodulated", demod[0]))}
    if B == 16:
        # the CPU test's figures (tests/test_demod_cpu.py: the same renders from the oracle, rho_c from 16 bins): the arithmetic is bit-exact, so the device's Y
        # figures are its to the last digit.  (At B = 64 rho_c is developed from 64 bins and Y differs in the fourth digit: not comparable.)
        import test_demod_cpu as cpu
        noisy, cpu_var, g, cpu_ref = cpu.noisy_and_reference(scene)
        rho16, wc = cpu.albedo_of(scene)
        cpu_demod, _ = cpu.image_only(noisy, cpu_var, g["prim"], rho16, wc, mr.DEFAULT_FLOOR, 5, mr.DEFAULT_SIGMA_L)
        assert np.array_equal(bits(cpu_demod), bits(demod[1])) and np.array_equal(bits(cpu_ref), bits(ref_image))
        assert y["demodulated"] == cpu.rmse_y(cpu_demod, cpu_ref) and y["unfiltered"] == cpu.rmse_y(noisy, cpu_ref)
    print("QUALITY %s B=%d: Y RMSE %s; bins RMSE %s" % (scene, B, ", ".join("%s %.6g" % kv for kv in y.items()), ", ".join("%s %.6g" % kv for kv in b.items())))
    if scene == "plane-srgb":
        assert y["demodulated"] < y["plain"] and b["demodulated"] < b["plain"]
    else:
        assert y["demodulated"] <= y["unfiltered"] and b["demodulated"] <= b["unfiltered"]
