"""Denoising on the GPU (include/ssx.h "Denoising"): the guide buffers against the oracle, the filter against its numpy restatement (tests/denoise_ref.py),
their composition from a context's own state, and the state rules, refusals and CLI around them.  "equals" is np.array_equal on the integer views.
Image sizes: 72 x 40 (a level-4 tap reaches 32 pixels: interior pixels horizontally, none vertically; the height is no multiple of 16), 20 x 12 (all border,
ragged 8-pixel tiles, no power of two: camera_dir divides), 16 x 8 (a power of two: it multiplies), 5 x 3."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.renderer import SsxError
from test_spectral_gpu import moved_corner_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
TEX = "test-img.png"
SEED = 5
SIZES = ((72, 40), (20, 12), (16, 8), (5, 3))
SCENES = ("cornell-srgb", "plane-srgb", "custom", "cornell-rgb")
bits = dr.bits
OTHER = dict(sigma_l=4.0, sigma_a=0.037)      # non-default scales


def is_rgb(scene):
    return scene.endswith("-rgb") and not scene.endswith("-srgb")


@functools.lru_cache(maxsize=None)
def oracle(scene):
    if scene == "custom":
        return moved_corner_scene().oracle()
    return ol.Oracle("cornell-srgb", texture=TEX, rgb=True) if is_rgb(scene) else ol.Oracle(scene, texture=TEX)


def renderer(scene, res, **opts):
    name = "cornell-srgb" if scene == "custom" or is_rgb(scene) else scene
    r = Renderer(Options(scene_name=name, res=res, seed=SEED, texture=TEX, jit_pass1=False, render_mode="rgb" if is_rgb(scene) else "spectral", **opts))
    if scene == "custom":
        r.upload_scene_desc(moved_corner_scene().desc(oracle(scene)))
    return r


@functools.lru_cache(maxsize=None)
def guides_of_oracle(scene, res):
    g = dr.guides_ref(oracle(scene), res[0], res[1], rgb=is_rgb(scene))
    for a in g.values():
        a.setflags(write=False)
    return g


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def render(r, spp, **over):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    r.render_wait()
    return r.xyza.copy()


# ---- 1. guide buffers ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", SCENES)
def test_guides_equal_the_oracles_first_hits(scene):
    r = renderer(scene, SIZES[0])
    for res in SIZES:
        got, want = r.guides(res), guides_of_oracle(scene, res)
        for k in ("prim", "depth", "normal", "albedo"):
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (scene, res, k)
    g = guides_of_oracle(scene, SIZES[0])
    assert (scene == "plane-srgb" or len(np.unique(g["prim"])) > 1) and (g["albedo"][g["prim"] != dr.MISS] != 0).any()
    again = r.guides(SIZES[1])                        # cached per size: asking again, and after another size, gives the same
    assert same([again[k] for k in again], [guides_of_oracle(scene, SIZES[1])[k] for k in again])
    only = np.zeros((SIZES[3][1], SIZES[3][0]), dtype=np.uint32)   # any pointer may be NULL
    r._check(r._lib.ssx_guides(r._ctx, SIZES[3][0], SIZES[3][1], only.ctypes.data, None, None, None))
    assert np.array_equal(only, guides_of_oracle(scene, SIZES[3])["prim"])


def test_guides_follow_the_uploaded_scene():
    r = renderer("cornell-srgb", SIZES[1])
    a = r.guides()
    r.upload_scene_desc(moved_corner_scene().desc(oracle("custom")))
    b = r.guides()
    want = guides_of_oracle("custom", SIZES[1])
    assert same([b[k] for k in b], [want[k] for k in b]) and not same([a[k] for k in a], [b[k] for k in a])


# ---- 2. the filter ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def filter_context():
    return renderer("cornell-srgb", SIZES[3])


@pytest.mark.parametrize("res", SIZES)
def test_the_filter_equals_its_restatement_on_synthetic_images(res):
    W, H = res
    c, var, prim, albedo = dr.synthetic(W, H, seed=W * 100 + H)
    assert (prim == dr.MISS).any() or W * H < 20
    assert np.isnan(c).sum() == 1 and np.isinf(var).sum() == 1 and (var == 0).any() and ((var > 0) & (var < 1e-38)).any()
    r = filter_context()
    for levels in range(1, 7):
        for sig in (dict(sigma_l=dr.DEFAULTS["sigma_l"], sigma_a=dr.DEFAULTS["sigma_a"]), OTHER):
            got = r.denoise_images(c, var, prim, albedo, levels=levels, return_variance=True, **sig)
            want = dr.atrous(c, var, prim, albedo, levels=levels, **sig)
            assert same(got, want), (res, levels, sig, int((bits(got[0]) != bits(want[0])).sum()), int((bits(got[1]) != bits(want[1])).sum()))
    default = r.denoise_images(c, var, prim, albedo)                                    # the defaults, var_out NULL
    assert np.array_equal(bits(default), bits(dr.atrous(c, var, prim, albedo, **dr.DEFAULTS)[0]))


# ---- 3. composition -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", SIZES[:2])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb", "cornell-rgb"])
def test_denoise_of_the_context_equals_the_pieces(scene, res):
    r = renderer(scene, res)
    r.set_noise_estimate(True)
    image = render(r, 16, spp_per_launch=4)
    _, v = r.noise()
    var = dr.variance_in_image_units(v, rgb=is_rgb(scene))
    g = r.guides()
    r.read_framebuffer()
    assert np.array_equal(bits(image), bits(r.xyza))
    for kw in (dict(dr.DEFAULTS), dict(levels=3, **OTHER)):
        own = r.denoise(return_variance=True, **kw)
        pieces = r.denoise_images(image, var, g["prim"], g["albedo"], return_variance=True, **kw)
        ref = dr.atrous(image, var, g["prim"], g["albedo"], **kw)
        assert same(own, pieces) and same(own, ref), (scene, res, kw)
    assert not np.array_equal(bits(own[0]), bits(image)) and (var > 0).any()


# ---- 4. state -----------------------------------------------------------------------------------------------------------------------------------

def test_denoising_reads_only():
    res = SIZES[1]
    r = renderer("cornell-srgb", res)
    r.set_noise_estimate(True)
    render(r, 16, spp_per_launch=4)
    before = r.export_sums()
    a = r.denoise(return_variance=True)
    b = r.denoise(return_variance=True)
    assert same(a, b)                                                                   # twice: the same
    after = r.export_sums()
    assert np.array_equal(bits(before[1]), bits(after[1])) and np.array_equal(bits(before[2]), bits(after[2])) and bytes(before[0]) == bytes(after[0])
    r.render_continue(16); r.render_wait()
    one_shot = renderer("cornell-srgb", res)
    assert np.array_equal(bits(r.xyza), bits(render(one_shot, 32)))                   # continue after it: the bits of a one-shot render


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------

def refused(call, code, *words):
    with pytest.raises(SsxError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals():
    res = SIZES[1]
    r = renderer("cornell-srgb", res)
    refused(r.denoise, _capi.SSX_ERR_STATE, "no sums")                               # nothing rendered
    render(r, 8, spp_per_launch=4)
    refused(r.denoise, _capi.SSX_ERR_STATE, "noise estimate is off")
    r.set_noise_estimate(True)
    render(r, 8, spp_per_launch=8)
    refused(r.denoise, _capi.SSX_ERR_STATE, "1 batch")
    render(r, 8, spp_per_launch=4)
    assert r.denoise().shape == (res[1], res[0], 4)
    for levels in (0, 7):
        refused(lambda: r.denoise(levels=levels), _capi.SSX_ERR_ARG, "levels")
    c, var, prim, albedo = dr.synthetic(res[0], res[1], 1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: r.denoise(sigma_l=bad), _capi.SSX_ERR_ARG, "sigma_l")
        refused(lambda: r.denoise_images(c, var, prim, albedo, sigma_a=bad), _capi.SSX_ERR_ARG, "sigma_a")
    half = renderer("cornell-srgb", res, tile_stride=2)
    half.set_noise_estimate(True)
    render(half, 8, spp_per_launch=4)
    refused(half.denoise, _capi.SSX_ERR_STATE, "tile_stride")
    # no scene uploaded: a bare context
    lib, ctx = _capi.hip_lib(), C.c_void_p()
    assert lib.ssx_create(0, C.byref(ctx)) == 0
    try:
        out = np.zeros((res[1], res[0], 4), dtype=np.float32)
        assert lib.ssx_denoise(ctx, None, out.ctypes.data, None) == _capi.SSX_ERR_STATE and b"no scene" in lib.ssx_last_error(ctx)
        assert lib.ssx_guides(ctx, res[0], res[1], None, None, None, None) == _capi.SSX_ERR_STATE and b"no scene" in lib.ssx_last_error(ctx)
        p = Renderer._denoise_params(5, 1.0, 0.1)                                    # the pure function needs no scene
        assert lib.ssx_denoise_images(ctx, C.byref(p), res[0], res[1], c.ctypes.data, var.ctypes.data, prim.ctypes.data, albedo.ctypes.data, out.ctypes.data, None) == 0
        assert np.array_equal(bits(out), bits(dr.atrous(c, var, prim, albedo, **dr.DEFAULTS)[0]))
    finally:
        lib.ssx_destroy(ctx)


# ---- 6. CLI -------------------------------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_denoised_image_and_the_guides(tmp_path):
    W, H = SIZES[1]
    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png"]
    r = renderer("cornell-srgb", (W, H))
    r.set_noise_estimate(True)
    render(r, 16, spp_per_launch=2)                                                   # ceil(16 / 8)
    r.framebuffer = r.scene.xyza_to_srgba(r.denoise(levels=4, sigma_l=2.0, sigma_a=0.2))
    r.save(str(tmp_path / "py.pfm"))                                                  # the same writer (libssx_host.so) on the Python result
    want = open(str(tmp_path / "py.pfm"), "rb").read()
    plain = renderer("cornell-srgb", (W, H)); render(plain, 16); plain.save(str(tmp_path / "plain.pfm"))
    assert want != open(str(tmp_path / "plain.pfm"), "rb").read()
    g = r.guides()
    outs = []
    for n, env in ((0, {}), (1, {"SSX_TEST_ONE_GPU": "1"})):
        pfm, npy = str(tmp_path / ("o%d.pfm" % n)), str(tmp_path / ("g%d.npy" % n))
        extra = ["--gpus=2"] if n else []
        p = subprocess.run(common + extra + ["-o=" + pfm, "--denoise", "--denoise-levels=4", "--denoise-sigma=2,0.2", "--guides-output=" + npy], cwd=ROOT,
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr
        outs.append(open(pfm, "rb").read())
        a = np.load(npy)
        assert a.dtype == np.float32 and a.shape == (H, W, 9)
        assert np.array_equal(a[..., 0], np.where(g["prim"] == dr.MISS, -1.0, g["prim"].astype(np.float32)).astype(np.float32))
        assert np.array_equal(bits(a[..., 1]), bits(g["depth"])) and np.array_equal(bits(a[..., 2:5]), bits(g["normal"])) and np.array_equal(bits(a[..., 5:9]), bits(g["albedo"]))
    assert outs[0] == want                                                              # the .pfm equals the Python result
    assert outs[1] == outs[0]                                                           # the multi-device host path: the same bytes
