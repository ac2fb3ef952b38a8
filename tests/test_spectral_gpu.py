"""Spectral radiance output on the GPU (include/ssx.h "Spectral radiance output"): the per-sample hero flux against the CPU oracle, the bins against a
sequential numpy restatement of the definition, and the invariances, kernel variants, refusals and CLI around them.  "equals" is np.array_equal on
the integer views (bit for bit).  Images are 20 x 12: ragged tiles in both directions, three tile columns and two rows."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import custom_scene as cs
import oracle_lib as ol
import spectral_ref
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import Scene, SsxError, spectral_bin_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
TEX = "test-img.png"
W, H, SEED = 20, 12, 5
SCENES = ("cornell-srgb", "plane-srgb", "custom")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@functools.lru_cache(maxsize=None)
def moved_corner_scene():
    """The Cornell box with one corner moved apart from its twin: no built-in mesh topology, so the generic kernel (or, asked for, its own) runs it.
    ONE object for the whole module: the description `desc()` returns points into the scene's own arrays (the texels), which must outlive the upload."""
    c = cs.CustomScene("cornell-srgb")
    pos, st, m = c.quads[0]
    pos = pos.copy(); pos[0, 0] += 1.0
    c.quads[0] = (pos, st, m)
    return c


@functools.lru_cache(maxsize=None)
def oracle(scene):
    return moved_corner_scene().oracle() if scene == "custom" else ol.Oracle(scene, texture=TEX)


def renderer(scene, jit=False, **opts):
    r = Renderer(Options(scene_name="cornell-srgb" if scene == "custom" else scene, res=(W, H), seed=SEED, texture=TEX, jit_pass1=jit, **opts))
    if scene == "custom":
        r.upload_scene_desc(moved_corner_scene().desc(oracle(scene)))
    return r


def start(r, spp, **over):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    r.render_wait()
    return r.xyza.copy()


@functools.lru_cache(maxsize=None)
def per_sample(scene, spp, flat_field=True, indirect_only=False):
    """ssx_debug_sample_flux and ssx_debug_samples of one context: (flux [H, W, spp, 4], lambda_0 [H, W, spp], xyza [H, W, spp, 4]); computed once, read-only."""
    r = renderer(scene, flat_field_correction=flat_field, indirect_only=indirect_only)
    r.set_spectral_bins(4)
    flux, lam = r.debug_sample_flux(spp=spp)
    xyza, _, _ = r.debug_samples(spp=spp)
    assert r.plan_info()["pass1"] == {"cornell-srgb": "cornell topology", "plane-srgb": "plane topology", "custom": "generic"}[scene]
    assert r.plan_info()["kernel"].endswith("_flux")
    for a in (flux, lam, xyza):
        a.setflags(write=False)
    return flux, lam, xyza


@functools.lru_cache(maxsize=None)
def lambda_range(scene):
    """(lambda_min, lambda_step) of the scene's colour tables (the host library's: CIE 1931 for every scene here)."""
    d = Scene("cornell-srgb" if scene == "custom" else scene, texture=TEX).desc.contents
    return np.float32(d.lambda_min), np.float32(d.lambda_step)


@functools.lru_cache(maxsize=None)
def restated(scene, spp, bins):
    """The definition, sequentially: (sums float64 [H, W, B], counts uint32 [H, W, M], mean float32 [H, W, B]) from the per-sample flux and lambda_0."""
    flux, lam, _ = per_sample(scene, spp)
    S, N, mean = spectral_ref.restate_bins(flux, lam, *lambda_range(scene), bins)
    for a in (S, N, mean):
        a.setflags(write=False)
    return S, N, mean


def spectral_of(r):
    _, mean, counts, sums = r.spectral_read(sums=True)
    return sums, counts, mean


def same_spectral(got, ref):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, ref))


# ---- 1. the flux of every sample against the oracle -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("flat_field,indirect_only", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("scene", SCENES)
def test_flux_projects_onto_the_oracles_sample(scene, flat_field, indirect_only):
    spp = 12
    flux, lam, xyza = per_sample(scene, spp, flat_field, indirect_only)
    o = oracle(scene)
    ref, _, _ = o.samples(W, H, spp, seed=SEED, indirect_only=indirect_only, flat_field=flat_field)
    proj, lam_ref = spectral_ref.project_flux(o, flux, lam, SEED, *lambda_range(scene))
    assert np.array_equal(bits(lam), bits(lam_ref))
    assert np.array_equal(bits(xyza), bits(ref))
    same = (bits(proj) == bits(ref[..., :3])) | (np.isnan(proj) & np.isnan(ref[..., :3]))
    assert same.all(), "%d of %d projected components differ" % ((~same).sum(), same.size)


# ---- 2. ... and component by component ---------------------------------------------------------------------------------------------------

def test_flux_components_are_the_emission_at_the_hero_wavelengths():
    """Three XYZ equations do not pin four fluxes.  A scene whose only primitive is a black emissive quad filling the view: every path is the camera ray's hit,
    so flux[i] is the emission spectrum at lambda_0 + i * lambda_step -- a non-flat one (the observer's x-bar table), so a swapped component shows."""
    c = cs.CustomScene("cornell", keep_quads=False)
    orc0 = ol.Oracle("cornell")
    data, low, high, _ = orc0.spectrum("xbar")
    black = c.add_spectrum(np.zeros(2, dtype=np.float32), low, high)
    mat = c.add_material(albedo_spectrum=black, emission_spectrum=c.add_spectrum(data, low, high))
    c.add_quad((-50, -50, -5), (50, -50, -5), (50, 50, -5), (-50, 50, -5), mat)
    c.set_camera((0, 0, 0), (0, 0, -1), vfov_deg=40.0, aspect=W / H)
    orc = c.oracle()
    r = Renderer(Options(scene_name="cornell", res=(W, H), seed=SEED, jit_pass1=False, explicit_light_sampling=False))
    r.upload_scene_desc(c.desc(orc))
    r.set_spectral_bins(8)
    spp = 6
    flux, lam = r.debug_sample_flux(spp=spp)
    d = r.scene.desc.contents
    xbar, out = orc.lib.orc_color_spectrum(orc.color, b"xbar"), (C.c_float * 4)()
    want = np.zeros_like(flux)
    for idx in np.ndindex(H, W, spp):
        orc.lib.orc_spectrum_hero(xbar, C.c_float(float(lam[idx])), C.c_float(d.lambda_step), out)
        want[idx] = out[:]
    assert (want[..., 0] != want[..., 1]).any() and (want[..., 1] != want[..., 2]).any() and (want[..., 2] != want[..., 3]).any()   # not flat
    assert np.array_equal(bits(flux), bits(want))


# ---- 3. the bins, bit for bit ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [4, 8, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_bins_equal_the_sequential_restatement(scene, bins):
    spp = 37
    assert np.array_equal(bits(per_sample(scene, spp)[0][:, :, :12]), bits(per_sample(scene, 12)[0]))   # the samples test 1 checked
    r = renderer(scene)
    r.set_spectral_bins(bins)
    start(r, spp, spp_per_launch=16)           # launches of 16 / 16 / 5
    sums, counts, mean = spectral_of(r)
    S, N, mu = restated(scene, spp, bins)
    assert np.array_equal(counts, N) and (counts.sum(axis=2) == spp).all()
    assert np.array_equal(bits(sums), bits(S))
    assert np.array_equal(bits(mean), bits(mu))
    mean2, counts2, centres = r.spectral_image()
    lmin, lstep = lambda_range(scene)
    w = lstep / np.float32(bins // 4)
    assert np.array_equal(bits(mean2), bits(mean)) and np.array_equal(counts2, counts)
    assert centres.dtype == np.float32 and np.array_equal(centres, lmin + (np.arange(bins, dtype=np.float32) + np.float32(0.5)) * w)


# ---- 4. invariances ---------------------------------------------------------------------------------------------------------------------------

def test_start_plus_continue_equals_one_render():
    r = renderer("cornell-srgb")
    r.set_spectral_bins(8)
    start(r, 16)
    r.render_continue(21); r.render_wait()
    assert r.done_spp() == 37 and same_spectral(spectral_of(r), restated("cornell-srgb", 37, 8))


def test_two_contexts_combined_by_ownership_equal_one():
    S, N, mu = restated("cornell-srgb", 37, 8)
    got = [np.zeros_like(S), np.zeros_like(N), np.zeros_like(mu)]
    for first in (0, 1):
        r = renderer("cornell-srgb", tile_first=first, tile_stride=2, tile_skew=1)
        r.set_spectral_bins(8)
        start(r, 37, spp_per_launch=16)
        part = spectral_of(r)
        mask = tile_owner_mask(W, H, first, 2, 1)
        for g, p in zip(got, part):
            assert not p[~mask].any()          # pixels the context does not own read as 0
            g[mask] = p[mask]
    assert same_spectral(got, (S, N, mu))


@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_image_does_not_depend_on_spectral_output(scene):
    r = renderer(scene)
    off = start(r, 37, spp_per_launch=16)
    r.set_spectral_bins(16)
    on = start(r, 37, spp_per_launch=16)
    assert np.array_equal(bits(on), bits(off))
    assert np.array_equal(bits(off), bits(oracle(scene).render(W, H, 37, seed=SEED)))


# ---- 5. kernel variants -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_narrow_queue_twins(scene, tmp_path):
    out = str(tmp_path / "nq.npz")
    env = dict(os.environ, SSX_DEBUG_ENV="1", SSX_NARROW_QUEUE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spectral_worker.py"), scene, str(W), str(H), "37", "16", str(SEED), "8", out],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    z = np.load(out)
    assert str(z["kernel"]).endswith("_nq_flux"), str(z["kernel"])
    assert same_spectral((z["sums"], z["counts"], z["mean"]), restated(scene, 37, 8))


def test_run_time_compiled_kernel():
    r = renderer("custom", jit=True)           # ssx_set_jit(ctx, SSX_JIT_AT_UPLOAD) before the upload
    assert r._lib.ssx_kernel_variant(r._ctx) == 3
    r.set_spectral_bins(8)
    start(r, 37, spp_per_launch=16)            # the pattern's _flux code object is compiled here, on the calling thread
    assert r._lib.ssx_kernel_variant(r._ctx) == 3 and r.plan_info()["kernel"].startswith("ssx_render_kernel_jit")
    assert same_spectral(spectral_of(r), restated("custom", 37, 8))
    assert np.array_equal(bits(r.xyza), bits(oracle("custom").render(W, H, 37, seed=SEED)))


# ---- 6. refusals and state -----------------------------------------------------------------------------------------------------------------------

def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals():
    import torch
    r = renderer("cornell-srgb")
    for n in (6, 68, 2, 128):
        refused(lambda: r.set_spectral_bins(n), _capi.SSX_ERR_ARG, "multiple of 4")
    refused(r.spectral_read, _capi.SSX_ERR_STATE, "spectral output is off")           # bins of 0: off
    refused(lambda: r.debug_sample_flux(spp=2), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(8)
    refused(r.spectral_read, _capi.SSX_ERR_STATE, "no render")                         # read before any render
    refused(lambda: start(r, 4, tile_major=1), _capi.SSX_ERR_ARG, "tile_major")
    refused(lambda: start(r, 4, libm=_capi.SSX_LIBM_GLIBC_2_35), _capi.SSX_ERR_ARG, "glibc")
    out = torch.zeros((H, W, 4), device="cuda")
    refused(lambda: r.render_device(out.data_ptr(), torch.cuda.current_stream().cuda_stream, spp=4), _capi.SSX_ERR_ARG, "ssx_render_device")
    rgb = renderer("cornell-srgb", render_mode="rgb")
    rgb.set_spectral_bins(8)
    refused(lambda: start(rgb, 4), _capi.SSX_ERR_ARG, "SSX_MODE_RGB")
    rgb.set_spectral_bins(0)
    start(rgb, 4)                                                                       # off again: renders as before
    # a changed bin count clears the state; so does an import, after which a continue renders normally
    start(r, 8)
    spectral_of(r)
    info, sums, s2 = r.export_sums()
    r.set_spectral_bins(16)
    refused(r.spectral_read, _capi.SSX_ERR_STATE, "bin count")
    start(r, 8)
    assert r.spectral_read()[0].bins == 16 and r.spectral_read()[0].done_spp == 8
    r.import_sums(info, sums, s2)
    refused(r.spectral_read, _capi.SSX_ERR_STATE, "ssx_sums_import")
    r.render_continue(4); r.render_wait()
    assert np.array_equal(bits(r.xyza), bits(oracle("cornell-srgb").render(W, H, 12, seed=SEED)))
    refused(r.spectral_read, _capi.SSX_ERR_STATE)


def test_sample_arrays_grow_by_a_third_and_only_while_on():
    r_off, r_on = renderer("cornell-srgb"), renderer("cornell-srgb")
    base = r_off.scratch_info()["sample_bytes"]              # the calibration render's launch
    assert r_on.scratch_info()["sample_bytes"] == base
    r_on.set_spectral_bins(16)
    start(r_off, 64, spp_per_launch=64); start(r_on, 64, spp_per_launch=64)
    off, on = r_off.scratch_info()["sample_bytes"], r_on.scratch_info()["sample_bytes"]
    records = 3 * 2 * 64 * 64
    assert off == max(base, records * 48) == records * 48 and on == records * 64 and 3 * on == 4 * off


# ---- 7. CLI ----------------------------------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_spectral_image(tmp_path):
    npy, png = str(tmp_path / "s.npy"), str(tmp_path / "o.png")
    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=37", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + png]
    p = subprocess.run(common + ["--spectral-output=" + npy, "--spectral-bins=8"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    a = np.load(npy)
    r = renderer("cornell-srgb")
    r.set_spectral_bins(8)
    start(r, 37)
    mean = r.spectral_image()[0]
    assert a.dtype == np.float32 and a.shape == (H, W, 8) and np.array_equal(bits(a), bits(mean))
    assert np.array_equal(bits(mean), bits(restated("cornell-srgb", 37, 8)[2]))
    p = subprocess.run(common + ["--spectral-output=" + npy], cwd=ROOT, capture_output=True, text=True)     # default: 16 bins
    assert p.returncode == 0 and np.load(npy).shape == (H, W, 16), p.stderr
    p = subprocess.run(common + ["--spectral-output=" + npy, "--resume=" + str(tmp_path / "c.ckpt")], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "cannot be combined with `--resume`" in p.stderr
