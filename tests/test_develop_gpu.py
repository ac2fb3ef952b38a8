"""Developing the spectral bins on the GPU (include/ssx.h "Developing the spectral bins"): ssx_develop_images and ssx_spectral_develop against the numpy
restatement (tests/develop_ref.py), ownership, the denoised source against its pieces, the state rules and refusals, two checks against the physics whose
bounds are derived in the test, and the CLI.  "equals" is np.array_equal on the integer views (bit for bit).  Images are 42 x 23: six tile columns and three
rows, the last of each ragged; 37 samples per pixel in launches of 16 / 16 / 5."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import custom_scene as cs
import develop_ref as ref
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import Scene, SsxError, develop_weights, emitter_spectrum, load_spectrum_csv, relight_gain, spectral_bin_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
D65 = os.path.join(ROOT, "data", "d65-300+5+780.csv")
TEX = "test-img.png"
W, H, SEED, SPP = 42, 23, 5, 37
F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


@functools.lru_cache(maxsize=None)
def moved_corner_scene():
    """The Cornell box with one corner moved apart from its twins: no built-in mesh topology, so asked for, its own run-time compiled kernel runs it.  A corner
    that no other test moves: the compiled code of a sharing pattern stays in the process's memory, and tests that upload the pattern of test_spectral_gpu.py's
    scene expect the generic kernel for it when they run first.  ONE object for the module: `desc()` points into the scene's own arrays."""
    c = cs.CustomScene("cornell-srgb")
    pos, st, m = c.quads[4]
    pos = pos.copy(); pos[1, 0] += 0.5
    c.quads[4] = (pos, st, m)
    return c


@functools.lru_cache(maxsize=None)
def custom_oracle():
    return moved_corner_scene().oracle()


def renderer(scene, jit=False, **opts):
    r = Renderer(Options(scene_name="cornell-srgb" if scene == "custom" else scene, res=(W, H), seed=SEED, texture=TEX, jit_pass1=jit, **opts))
    if scene == "custom":
        r.upload_scene_desc(moved_corner_scene().desc(custom_oracle()))
    return r


def start(r, spp=SPP, **over):
    over.setdefault("spp_per_launch", 16)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    r.render_wait()
    return r.xyza.copy()


def lambda_range(r):
    d = r.scene.desc.contents
    return float(d.lambda_min), float(d.lambda_step)


def random_weights(channels, bins, seed):
    return np.random.default_rng(seed).uniform(-2, 3, size=(channels, bins)).astype(F)


def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


# ---- 1. the pure function ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plain_context():
    return renderer("cornell-srgb")


@pytest.mark.parametrize("channels", [1, 3, 7, 16])
@pytest.mark.parametrize("bins", [4, 16, 64])
def test_develop_images_equals_the_restatement(bins, channels):
    g = np.random.default_rng(bins * 100 + channels)
    q = g.uniform(-4, 9, size=(H, W, bins)).astype(F)
    flat = q.reshape(-1, bins)
    at = g.permutation(H * W)
    flat[at[0], 0] = F(np.nan); flat[at[1], bins - 1] = F(np.inf); flat[at[2], 1] = F(-np.inf); flat[at[3], :] = F(-0.0); flat[at[4], 2] = F(-0.0)
    flat[at[5], 0] = F(np.inf); flat[at[5], 1] = F(-np.inf)                                            # inf - inf inside one pixel
    w = random_weights(channels, bins, bins + channels)
    w[0, 0] = F(0.0); w[-1, -1] = F(-0.0)                                                              # 0 * inf and 0 * nan are NaN, not skipped
    got = plain_context().develop_images(q, w)
    want = ref.develop(q, w)
    assert got.shape == (H, W, channels) and got.dtype == np.float32
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), "%d of %d differ" % ((~same).sum(), same.size)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert np.array_equal(bits(got.reshape(-1, channels)[at[3]]), bits(want.reshape(-1, channels)[at[3]]))   # the row of negative zeros, sign and all


# ---- 2. the raw source -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [4, 64])
@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb", "custom"])
def test_raw_develop_equals_the_restatement_on_the_sums(scene, bins):
    r = renderer(scene, jit=(scene == "custom"))
    if scene == "custom":
        assert r._lib.ssx_kernel_variant(r._ctx) == 3                                                   # the run-time compiled kernel
    r.set_spectral_bins(bins)
    start(r)
    info, _, counts, sums = r.spectral_read(sums=True)
    assert info.done_spp == SPP and (counts.sum(axis=2) == SPP).all()
    q = ref.raw_q(sums, SPP)
    assert (q != 0).any()
    for channels in (3, 12):
        w = random_weights(channels, bins, channels)
        assert np.array_equal(bits(r.develop(w)), bits(ref.develop(q, w))), (scene, bins, channels)
    lmin, lstep = lambda_range(r)
    w = develop_weights(bins, lmin, lstep)                                                              # the observer's own weights
    assert np.array_equal(bits(r.develop(w)), bits(ref.develop(q, w)))
    assert np.array_equal(bits(r.develop_images(q, w)), bits(r.develop(w)))                             # the two kernels, held against each other


# ---- 3. ownership -----------------------------------------------------------------------------------------------------------------------------------------

def test_two_contexts_combined_by_ownership_equal_one():
    w = random_weights(5, 8, 1)
    one = renderer("cornell-srgb")
    one.set_spectral_bins(8)
    start(one)
    want = one.develop(w)
    got = np.full_like(want, F(7))
    for first in (0, 1):
        r = renderer("cornell-srgb", tile_first=first, tile_stride=2, tile_skew=1)
        r.set_spectral_bins(8)
        start(r)
        part = r.develop(w)
        mask = tile_owner_mask(W, H, first, 2, 1)
        assert not bits(part[~mask]).any()                                                              # foreign pixels read +0 (not -0) in every channel
        got[mask] = part[mask]
    assert np.array_equal(bits(got), bits(want))


# ---- 4. the denoised source --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [8, 64])
def test_denoised_develop_equals_develop_images_of_the_filtered_bins(bins):
    r = renderer("cornell-srgb")
    r.set_noise_estimate(True)
    r.set_spectral_bins(bins)
    start(r, 16, spp_per_launch=4)
    for kw in ({}, dict(levels=3, sigma_l=4.0, sigma_a=0.037)):
        filtered = r.denoise_spectral(**kw)
        for channels in (3, 16):
            w = random_weights(channels, bins, channels + 1)
            got = r.develop(w, denoise=kw)
            assert np.array_equal(bits(got), bits(r.develop_images(filtered, w))), (bins, kw, channels)
            assert np.array_equal(bits(got), bits(ref.develop(filtered, w)))
        assert np.array_equal(bits(r.denoise_spectral(**kw)), bits(filtered))                           # develop left the filter's buffers as ssx_denoise_spectral needs them
    assert not np.array_equal(bits(r.develop(w)), bits(got))                                            # raw and denoised differ


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------------------------------

def test_develop_reads_only_and_continues():
    w = random_weights(3, 8, 2)
    one = renderer("cornell-srgb")
    one.set_noise_estimate(True)
    one.set_spectral_bins(8)
    image = start(one)
    spectral = one.spectral_read(sums=True)
    developed = one.develop(w)
    r = renderer("cornell-srgb")
    r.set_noise_estimate(True)
    r.set_spectral_bins(8)
    start(r, 16, spp_per_launch=8)                                                                      # two batches: the denoised source needs a variance
    r.develop(w); r.develop(w, denoise={})
    r.render_continue(21); r.render_wait()
    assert r.done_spp() == SPP and np.array_equal(bits(r.xyza), bits(image))
    again = r.spectral_read(sums=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], spectral[1:]))
    assert np.array_equal(bits(r.develop(w)), bits(developed))                                          # start + continue: the developed bits of one render


def test_refusals():
    r = renderer("cornell-srgb")
    w = random_weights(3, 8, 3)
    refused(lambda: r.develop(w), _capi.SSX_ERR_STATE, "spectral output is off")
    r.set_spectral_bins(8)
    refused(lambda: r.develop(w), _capi.SSX_ERR_STATE, "no spectral bins", "no render")
    start(r, 8)
    r.develop(w)
    refused(lambda: r.develop(w, denoise={}), _capi.SSX_ERR_STATE, "noise estimate is off")            # what ssx_denoise_spectral refuses
    refused(lambda: r.develop(w, denoise=dict(levels=7)), _capi.SSX_ERR_ARG, "levels")
    info, sums, s2 = r.export_sums()
    r.import_sums(info, sums, s2)
    refused(lambda: r.develop(w), _capi.SSX_ERR_STATE, "no spectral bins", "ssx_sums_import")
    start(r, 8)
    r.set_spectral_bins(16)
    refused(lambda: r.develop(random_weights(3, 16, 3)), _capi.SSX_ERR_STATE, "bin count")
    r.set_spectral_bins(8)
    # arguments
    for channels in (0, 17):
        refused(lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, channels, None)), _capi.SSX_ERR_ARG, "channels")
    refused(lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, None, 3, None)), _capi.SSX_ERR_ARG, "weights")
    q = np.zeros((H, W, 8), dtype=F)
    out = np.zeros((H, W, 3), dtype=F)
    call = lambda bins=8, qp=q.ctypes.data, wp=w.ctypes.data, ch=3, op=out.ctypes.data, width=W: r._check(r._lib.ssx_develop_images(r._ctx, width, H, bins, qp, wp, ch, op))
    call()
    for bins in (0, 6, 68, 128):
        refused(lambda: call(bins=bins), _capi.SSX_ERR_ARG, "multiple of 4")
    for ch in (0, 17):
        refused(lambda: call(ch=ch), _capi.SSX_ERR_ARG, "channels")
    refused(lambda: call(qp=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: call(wp=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: call(op=None), _capi.SSX_ERR_ARG, "NULL")
    refused(lambda: call(width=0), _capi.SSX_ERR_ARG)
    # while a render runs
    start(r, 8)
    r._check(r._lib.ssx_render_continue(r._ctx, 1 << 16))
    try:
        refused(lambda: r.develop(w), _capi.SSX_ERR_STATE, "render in progress")
        refused(call, _capi.SSX_ERR_STATE, "render in progress")
    finally:
        r.render_stop(); r.render_wait()
    r.develop(w)                                                                                        # the stopped render: developed at the count it reached


# ---- 6. physics: the develop under the render's own observer against the render's image --------------------------------------------------------------------

def test_raw_develop_under_the_renders_observer_is_the_image_up_to_the_bin_average():
    """out_c - image_c = (1/n) sum_k sum_i f_ki (avg_b(bar_c) - bar_c(lambda_ki)) lambda_step with b the bin of sample k's component i: the develop replaces the
    observer by its bin average (include/ssx.h).  So |difference| <= (1/n) sum_k sum_i |f_ki| max over the bin of |bar_c - avg_b(bar_c)| lambda_step, the maximum
    of a piecewise-linear function being taken at its knots and the bin's edges, plus the binary32 rounding slack (B + 4) 2^-23 sum_b |q_b W_cb|.  Every pixel and
    channel is held to it.  The largest relative difference of the image-mean Y at B = 4, 16, 64 is printed, not asserted."""
    flux_r = renderer("cornell-srgb")
    flux_r.set_spectral_bins(4)
    flux, lam = flux_r.debug_sample_flux(spp=SPP)
    lmin, lstep = lambda_range(flux_r)
    tables = ref.observer_tables(flux_r.scene)
    r = renderer("cornell-srgb")
    report = {}
    for bins in (4, 16, 64):
        r.set_spectral_bins(bins)
        image = start(r)
        if bins == 64:
            assert np.array_equal(bits(image), bits(ol.Oracle("cornell-srgb", texture=TEX).render(W, H, SPP, seed=SEED)))   # the image is the oracle's
        w, w64 = develop_weights(bins, lmin, lstep, return_float64=True)
        out = r.develop(w)
        report[bins] = abs(float(out[..., 1].astype(np.float64).mean()) / float(image[..., 1].astype(np.float64).mean()) - 1.0)
        if bins != 64:
            continue
        q = ref.raw_q(r.spectral_read(sums=True)[3], SPP)
        bound = ref.bin_average_bound(flux, lam, q, w, w64, tables, bins, lmin, lstep, SPP)             # the docstring's bound, slack included
        diff = np.abs(out.astype(np.float64) - image[..., :3].astype(np.float64))
        assert np.isfinite(diff).all() and (diff <= bound).all(), "largest excess %g" % float((diff - bound).max())
        print("develop vs image at B = 64: largest |difference| / bound = %.4f" % float((diff[diff > 0] / bound[diff > 0]).max()))   # (a black pixel is 0 against 0)
    print("relative difference of the image-mean Y, develop against render: " + ", ".join("B = %d: %.3e" % kv for kv in sorted(report.items())))


# ---- 7. a known spectrum -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bins", [8, 16])
def test_unit_weights_return_bins_that_lie_inside_the_emission(bins):
    """The scene of test_flux_components_are_the_emission...: one black emissive quad filling the view, emission = the observer's x-bar table.  Every flux that
    falls into bin b is the emission somewhere in bin b, so S[b] / N[b % M] lies between the emission's minimum and maximum over the bin; with unit weights the
    develop returns q[b] = S[b] M / n = (S[b] / N[b % M]) (N[b % M] M / n).  q is therefore held to [min, max] of the bin times that known count factor, widened by
    one binary32 ulp (q[b] itself lies in [min, max] only where the sub-bin holds exactly n / M samples: the counts are random).  A swapped or shifted bin falls
    outside: the table is not flat."""
    c = cs.CustomScene("cornell", keep_quads=False)
    data, low, high, _ = ol.Oracle("cornell").spectrum("xbar")
    black = c.add_spectrum(np.zeros(2, dtype=np.float32), low, high)
    mat = c.add_material(albedo_spectrum=black, emission_spectrum=c.add_spectrum(data, low, high))
    c.add_quad((-50, -50, -5), (50, -50, -5), (50, 50, -5), (-50, 50, -5), mat)
    c.set_camera((0, 0, 0), (0, 0, -1), vfov_deg=40.0, aspect=W / H)
    r = Renderer(Options(scene_name="cornell", res=(W, H), seed=SEED, jit_pass1=False, explicit_light_sampling=False))
    r.upload_scene_desc(c.desc(c.oracle()))
    r.set_spectral_bins(bins)
    start(r)
    M = bins // 4
    q = r.develop(np.eye(bins, dtype=F))                                                                # C = B: at 16, all four channel groups
    counts = r.spectral_read()[2]
    lmin, lstep = lambda_range(r)
    factor = np.tile(counts, (1, 1, 4)).astype(np.float64) * M / SPP                                    # [H, W, B]
    ext = np.array([ref.table_extrema_over((data, low, high), ref.bin_edge(b, bins, lmin, lstep), ref.bin_edge(b + 1, bins, lmin, lstep)) for b in range(bins)])
    assert (ext[:, 1] > ext[:, 0]).all() and len(set(ext[:, 1])) == bins                                # not flat, and no two bins alike
    lo = np.nextafter((ext[:, 0] * factor).astype(F), F(-np.inf))
    hi = np.nextafter((ext[:, 1] * factor).astype(F), F(np.inf))
    assert (factor > 0).any() and ((q >= lo) & (q <= hi)).all(), "%d bins outside" % int((~((q >= lo) & (q <= hi))).sum())
    assert (q[factor == 0] == 0).all()
    shifted = np.roll(q, 1, axis=2)
    assert not ((shifted >= lo) & (shifted <= hi)).all()                                                # the interval does tell a shifted bin


# ---- 8. CLI -----------------------------------------------------------------------------------------------------------------------------------------------

def save_developed(r, xyz, path, scene=None):
    xyza = np.concatenate([xyz, r.xyza[..., 3:]], axis=2)
    r.framebuffer = (scene or r.scene).xyza_to_srgba(xyza)
    r.save(path)


def test_cli_writes_the_developed_image(tmp_path):
    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + str(tmp_path / "o.pfm"),
              "--spectral-bins=8"]
    r = renderer("cornell-srgb")
    r.set_noise_estimate(True)
    r.set_spectral_bins(8)
    start(r, 16, spp_per_launch=2)                                                                      # ceil(16 / 8): --spectral-denoise's launch rule
    lmin, lstep = lambda_range(r)
    w = develop_weights(8, lmin, lstep)
    kw = dict(levels=4, sigma_l=2.0, sigma_a=0.2)
    save_developed(r, r.develop(w), str(tmp_path / "raw.pfm"))
    save_developed(r, r.develop(w, denoise=kw), str(tmp_path / "den.pfm"))
    d = r.scene.desc.contents
    e = d.spectra[emitter_spectrum(r.scene.desc)]
    emitter = (np.array(d.samples[e.offset:e.offset + e.n], dtype=F), e.low, e.high)
    d65 = load_spectrum_csv(D65)
    w2 = develop_weights(8, lmin, lstep, observer=2006, filter=d65, gain=relight_gain(emitter, d65, 8, lmin, lstep))
    save_developed(r, r.develop(w2), str(tmp_path / "other.pfm"), Scene("cornell-srgb", observer=2006, texture=TEX))
    raw, den, other = (open(str(tmp_path / n), "rb").read() for n in ("raw.pfm", "den.pfm", "other.pfm"))
    assert raw != den and raw != other
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    filt = ["--spectral-denoise", "--denoise-levels=4", "--denoise-sigma=2,0.2"]
    cases = ((raw, []), (den, filt), (raw, ["--gpus=2"]), (den, filt + ["--gpus=2"]),
             (other, ["--develop-observer=2006", "--develop-filter=" + D65, "--develop-relight=" + D65]))
    for n, (want, extra) in enumerate(cases):
        path = str(tmp_path / ("d%d.pfm" % n))
        p = subprocess.run(common + ["--develop-output=" + path] + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr
        assert open(path, "rb").read() == want, extra
