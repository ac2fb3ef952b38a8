"""The kernels behind the path tracer -- the _flux twins, the bin, export and develop-state kernels, the guides, the variance, the three a-trous kernels, pack,
unpack, spectral channels and ratio, the develop kernels -- held to their references where the path kernel itself is tested: the scene and option matrix of
tests/crafted.py (1), a whole-image context with a tile skew (2), sizes at which every level is interior and degenerate ones (3), and values at the edges of
binary32 (4).  "equals" is np.array_equal on the integer views, NaN matching NaN where the parity tests allow it.  tests/test_pipeline_matrix_cpu.py shows,
without a GPU, that every input reaches what it is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

import crafted
import custom_scene as cs
import denoise_ref as dr
import denoise_spectral_ref as sr
import develop_ref as ref
import oracle_lib as ol
import spectral_ref
from simple_spectral_amd import Options, Renderer
from simple_spectral_amd.renderer import develop_weights

pytestmark = pytest.mark.gpu
F = np.float32
W, H, SEED = 20, 12, 5
BIG = (72, 40)
LARGE = (150, 134)
DEGENERATE = ((1, 37), (37, 1), (1, 1))
OTHER = dict(sigma_l=4.0, sigma_a=0.037)
DEFAULT_SIGMAS = dict(sigma_l=dr.DEFAULTS["sigma_l"], sigma_a=dr.DEFAULTS["sigma_a"])
SIGMAS = (DEFAULT_SIGMAS, OTHER)
bits = dr.bits


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def same_or_both_nan(a, b):
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def start(r, spp, **over):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    r.render_wait()
    return r.xyza.copy()


def random_weights(channels, bins, seed):
    return np.random.default_rng(seed).uniform(-2, 3, size=(channels, bins)).astype(F)


def lambda_range(case):
    col = C.cast(case.oracle.color, C.POINTER(dr._OrcColorHead)).contents
    return F(col.lambda_min), F(col.lambda_step)


# ---- 1. the scene and option matrix ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def per_sample(name):
    """ssx_debug_sample_flux and ssx_debug_samples of the case at 37 spp: (flux [H, W, 37, 4], lambda_0, xyza, levels); computed once, read-only.  A sample does
    not depend on how many follow it: (a) checks the first 12 against the oracle, (b) restates the bins from all 37."""
    case = crafted.matrix_case(name)
    r = case.renderer((W, H))
    r.set_spectral_bins(4)
    flux, lam = r.debug_sample_flux(spp=37)
    xyza, _, levels = r.debug_samples(spp=37)
    info = r.plan_info()
    assert info["pass1"] == case.pass1, info
    if case.jit:                                              # the kernels compiled for this scene's topology, with -DSSX_JIT_FLUX now that spectral output is on
        assert info["pass1"].startswith("scene topology") and info["kernel"].startswith("ssx_render_kernel_jit") and r._lib.ssx_kernel_variant(r._ctx) == 3, info
    else:
        assert info["kernel"].endswith("_flux"), info
    for a in (flux, lam, xyza, levels):
        a.setflags(write=False)
    return flux, lam, xyza, levels


@functools.lru_cache(maxsize=None)
def restated(name, bins):
    """The definition, sequentially, with the case's own lambda_min and lambda_step: (sums float64 [H, W, B], counts uint32 [H, W, M], mean float32 [H, W, B])"""
    flux, lam, _, _ = per_sample(name)
    return spectral_ref.restate_bins(flux, lam, *lambda_range(crafted.matrix_case(name)), bins)


@pytest.mark.parametrize("name", crafted.MATRIX_CASES)
def test_a_flux_projects_onto_the_oracles_sample(name):
    spp = 12
    case = crafted.matrix_case(name)
    flux, lam, xyza, levels = (a[:, :, :spp] for a in per_sample(name))
    o = case.oracle
    want, _, _ = case.samples_ref(W, H, spp, seed=SEED)
    lmin, lstep = lambda_range(case)
    proj, lam_ref = spectral_ref.project_flux(o, flux, lam, SEED, lmin, lstep)
    assert np.array_equal(bits(lam), bits(lam_ref))
    assert same_or_both_nan(xyza, want)
    assert same_or_both_nan(proj, want[..., :3]), "%d projected components differ" % int((bits(proj) != bits(want[..., :3])).sum())
    if name in crafted.MATRIX_BLACK:
        assert not flux.any()
    else:
        assert (flux != 0).any()
    if not case.flags["els"]:                     # an emission term below the first level: two or more levels, a first hit that emits nothing, flux all the same
        first = dr.sample_first_hits(o, W, H, spp, SEED)
        deep = (first >= 0) & ~np.isin(first, np.array(sorted(case.light_prims()))) & (flux != 0).any(axis=-1) & (levels >= 2)
        assert deep.any()
    if name in ("prims128-2006", "observer2006"):
        assert lmin != F(380)


@pytest.mark.parametrize("name", crafted.MATRIX_CASES)
def test_b_bins_equal_the_sequential_restatement(name):
    spp = 37
    case = crafted.matrix_case(name)
    r = case.renderer((W, H))
    off = start(r, spp, spp_per_launch=16)                       # launches of 16 / 16 / 5
    assert same_or_both_nan(off, case.render_ref(W, H, spp, seed=SEED))
    for B in (4, 64):
        r.set_spectral_bins(B)
        on = start(r, spp, spp_per_launch=16)
        assert np.array_equal(bits(on), bits(off))               # the image does not depend on spectral output
        _, mean, counts, sums = r.spectral_read(sums=True)
        S, N, mu = restated(name, B)
        assert np.array_equal(counts, N) and (counts.sum(axis=2) == spp).all()
        assert same_or_both_nan(sums, S) and same_or_both_nan(mean, mu), (name, B)
        assert (ref.raw_q(sums, spp) != 0).any() or name in crafted.MATRIX_BLACK


@pytest.mark.parametrize("name", crafted.MATRIX_CASES)
def test_c_guides_equal_the_oracles_first_hits(name):
    case = crafted.matrix_case(name)
    r = case.renderer((W, H))
    for res in ((W, H), BIG):
        got, want = r.guides(res), dr.guides_ref(case.oracle, res[0], res[1])
        for k in ("prim", "depth", "normal"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (name, res, k)
        assert same_or_both_nan(got["albedo"], want["albedo"]), (name, res)
        ids = set(got["prim"][got["prim"] != dr.MISS].tolist())
        assert len(ids) > (0 if name in crafted.MATRIX_BLACK else 1)
        if name == "triangles":
            assert ids & set(case.scene.kinds)
        if name == "mirror":
            assert any(q >= 9 for q in ids)
        if name == "textures" and res == BIG:
            mats = [case.scene.materials[case.scene.quads[int(p)][2]] for p in ids]
            assert len({m["albedo_texture"] for m in mats if m["albedo_mode"] == 1}) >= 5


@pytest.mark.parametrize("name", crafted.MATRIX_CASES)
def test_d_e_filter_chain_and_develop_from_the_contexts_state(name):
    B, spp = 16, 16
    case = crafted.matrix_case(name)
    r = case.renderer((W, H))
    r.set_noise_estimate(True)
    r.set_spectral_bins(B)
    image = start(r, spp, spp_per_launch=4)
    info, mean, counts, sums = r.spectral_read(sums=True)
    assert info.done_spp == spp and (counts.sum(axis=2) == spp).all()
    _, v = r.noise()
    var = dr.variance_in_image_units(v)
    g = r.guides()
    black = name in crafted.MATRIX_BLACK
    assert (var > 0).any() or black
    q = ref.raw_q(sums, spp)
    assert (q != 0).any() or black
    lmin, lstep = lambda_range(case)
    weights = (random_weights(5, B, 5), develop_weights(B, float(lmin), float(lstep), observer=case.options.get("observer", 1931)))
    for w in weights:
        assert same_or_both_nan(r.develop(w), ref.develop(q, w)), name
    for kw in (dict(dr.DEFAULTS), dict(levels=3, **OTHER)):
        own = r.denoise_spectral(return_image=True, **kw)
        want = sr.denoise_spectral(sums, counts, spp, image, var, g["prim"], g["albedo"], **kw)
        assert all(same_or_both_nan(a, b) for a, b in zip(own, want)), (name, kw)
        for w in weights:
            assert same_or_both_nan(r.develop(w, denoise=kw), ref.develop(want[0], w)), (name, kw)


def test_e_raw_develop_under_the_2006_observer_is_the_image_up_to_the_bin_average():
    """The bound of tests/test_develop_gpu.py (develop_ref.bin_average_bound) with the 2006 tables, B = 64, 37 spp: every pixel and channel is held to it."""
    case = crafted.matrix_case("observer2006")
    bins, spp = 64, 37
    flux, lam, _, _ = per_sample("observer2006")
    lmin, lstep = (float(x) for x in lambda_range(case))
    r = case.renderer((W, H))
    r.set_spectral_bins(bins)
    image = start(r, spp, spp_per_launch=16)
    w, w64 = develop_weights(bins, lmin, lstep, observer=2006, return_float64=True)
    out = r.develop(w)
    q = ref.raw_q(r.spectral_read(sums=True)[3], spp)
    bound = ref.bin_average_bound(flux, lam, q, w, w64, ref.observer_tables(r.scene), bins, lmin, lstep, spp)
    diff = np.abs(out.astype(np.float64) - image[..., :3].astype(np.float64))
    assert lmin == 390.0 and (image[..., :3] != 0).any()
    assert np.isfinite(diff).all() and (diff <= bound).all(), "largest excess %g" % float((diff - bound).max())


# ---- 2. a whole-image context with a tile skew -------------------------------------------------------------------------------------------------------------------

SKEW_RES = (42, 23)


@functools.lru_cache(maxsize=None)
def skewed(skew):
    """Everything a whole-image context (tile_stride = 1) with this tile_skew returns: cornell-srgb, 42 x 23, 8 bins, noise estimate, 16 spp in 4 launches."""
    r = Renderer(Options(scene_name="cornell-srgb", res=SKEW_RES, seed=SEED, texture=crafted.MATRIX_TEX, jit_pass1=False, tile_stride=1, tile_skew=skew))
    r.set_noise_estimate(True)
    r.set_spectral_bins(8)
    out = {"image": start(r, 16, spp_per_launch=4)}
    out["spectral"] = r.spectral_read(sums=True)[1:]
    out["noise"] = r.noise()[1]
    for tag, kw in (("default", {}), ("other", dict(levels=3, **OTHER))):
        out["denoise " + tag] = r.denoise(return_variance=True, **kw)
        out["denoise_spectral " + tag] = r.denoise_spectral(return_image=True, **kw)
        for channels in (3, 12):
            w = random_weights(channels, 8, channels)
            out["develop %d %s" % (channels, tag)] = (r.develop(w), r.develop(w, denoise=kw))
    r.render_continue(16); r.render_wait()
    out["continued"] = (r.xyza.copy(),) + tuple(r.spectral_read(sums=True)[1:])
    return out


@pytest.mark.parametrize("skew", [1, 5, 2 ** 31 + 5])
def test_a_tile_skew_changes_nothing_a_whole_image_context_returns(skew):
    assert (SKEW_RES[0] + 7) // 8 == 6 and skew % 6 != 0
    plain, got = skewed(0), skewed(skew)
    assert (plain["noise"] > 0).any() and (ref.raw_q(plain["spectral"][2], 16) != 0).any()
    for key, want in plain.items():
        have = got[key]
        if isinstance(want, np.ndarray):
            want, have = (want,), (have,)
        assert same(have, want), (skew, key)
    one_shot = Renderer(Options(scene_name="cornell-srgb", res=SKEW_RES, seed=SEED, texture=crafted.MATRIX_TEX, jit_pass1=False))
    one_shot.set_spectral_bins(8)
    image = start(one_shot, 32)
    assert same(got["continued"], (image,) + tuple(one_shot.spectral_read(sums=True)[1:]))


# ---- 3. sizes ------------------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pure_context():
    return Renderer(Options(scene_name="cornell-srgb", res=(5, 3), seed=SEED, texture=crafted.MATRIX_TEX, jit_pass1=False))


LARGE_INPUTS = ("blobs", "one-primitive")      # denoise_ref.synthetic: primitive edges at every step; synthetic_large: pixels that count all 25 taps at step 32


@functools.lru_cache(maxsize=None)
def sized_inputs(res, kind="blobs"):
    w, h = res
    if w * h < 8:                                             # `synthetic` places eight special pixels
        g = np.random.default_rng(w * 100 + h)
        c = g.uniform(0, 4, size=(h, w, 4)).astype(F)
        var, prim, albedo = np.full((h, w), F(0.04)), np.ones((h, w), dtype=np.uint32), g.uniform(0, 1, size=(h, w, 4)).astype(F)
        e = g.uniform(-2, 6, size=(h, w, 80)).astype(F)
        e[..., 4] = np.uint32(0x00000123).view(F)
    else:
        c, var, prim, albedo = (dr.synthetic_large if kind == "one-primitive" else dr.synthetic)(w, h, seed=w * 100 + h)
        e = dr.extras_with_specials(c, var, w + h)
    for a in (c, var, prim, albedo, e):
        a.setflags(write=False)
    return c, var, prim, albedo, e


@functools.lru_cache(maxsize=None)
def restated_levels(res, extreme=False, sigma=0, kind="blobs"):
    """[(c, var, e)] after levels 1 .. 6 of the restatement (80 channels), accumulated level by level"""
    c, var, prim, albedo, e = extreme_inputs() if extreme else sized_inputs(res, kind)
    out, cur = [], (np.ascontiguousarray(c), var, e)
    for level in range(6):
        cur = sr.channels_level(cur[0], cur[1], prim, albedo, cur[2], 1 << level, **SIGMAS[sigma])
        out.append(cur)
    return out


@pytest.mark.parametrize("kind", LARGE_INPUTS)
def test_the_image_and_variance_at_a_size_where_every_level_is_interior(kind):
    assert dr.interior_pixels(LARGE[0], LARGE[1], 32) >= 1 and all(v > 0 for v in dr.lds_tile_classes(LARGE[0], LARGE[1], 2).values())
    c, var, prim, albedo, _ = sized_inputs(LARGE, kind)
    counted = dr.level_trace(c, var, prim, albedo, 32, **DEFAULT_SIGMAS)["counted"]
    assert counted.all(axis=0).any() if kind == "one-primitive" else (len(np.unique(prim)) == 4 and not counted.all(axis=0).any())
    r = pure_context()
    for levels in range(1, 7):
        got = r.denoise_images(c, var, prim, albedo, levels=levels, return_variance=True)
        assert same(got, dr.atrous(c, var, prim, albedo, levels=levels)), levels
        assert same(got, restated_levels(LARGE, kind=kind)[levels - 1][:2]), levels


@pytest.mark.parametrize("kind", LARGE_INPUTS)
@pytest.mark.parametrize("E", [5, 80])
def test_the_extra_channels_at_a_size_where_every_level_is_interior(E, kind):
    c, var, prim, albedo, e = sized_inputs(LARGE, kind)
    r = pure_context()
    for levels in (1, 2, 3, 6):
        want = restated_levels(LARGE, kind=kind)[levels - 1]
        got = r.denoise_channels(c, var, prim, albedo, e[..., :E], levels=levels, return_image=True)
        assert same_or_both_nan(got[0], want[2][..., :E]), (E, levels, int((bits(got[0]) != bits(want[2][..., :E])).sum()))
        assert same(got[1:], want[:2]), (E, levels)


@pytest.mark.parametrize("bins,channels", [(64, 16), (4, 1)])
def test_develop_images_at_the_large_size(bins, channels):
    w, h = LARGE
    g = np.random.default_rng(bins + channels)
    q = g.uniform(-4, 9, size=(h, w, bins)).astype(F)
    q[0, 0, 0] = F(np.nan); q[-1, -1, -1] = F(np.inf); q[h // 2, w // 2, :] = F(-0.0)
    wt = random_weights(channels, bins, bins * channels)
    got, want = pure_context().develop_images(q, wt), ref.develop(q, wt)
    assert got.shape == (h, w, channels) and same_or_both_nan(got, want)
    assert np.array_equal(bits(got[h // 2, w // 2]), bits(want[h // 2, w // 2]))


@pytest.mark.parametrize("res", DEGENERATE)
def test_degenerate_sizes(res):
    w, h = res
    c, var, prim, albedo, e = sized_inputs(res)
    r = pure_context()
    for levels in range(1, 7):
        want = restated_levels(res)[levels - 1]
        assert same(r.denoise_images(c, var, prim, albedo, levels=levels, return_variance=True), want[:2]), (res, levels)
        for E in (5, 80):
            got = r.denoise_channels(c, var, prim, albedo, e[..., :E], levels=levels, return_image=True)
            assert same_or_both_nan(got[0], want[2][..., :E]) and same(got[1:], want[:2]), (res, levels, E)
    got, want = r.guides(res), dr.guides_ref(ol.Oracle("cornell-srgb", texture=crafted.MATRIX_TEX), w, h)
    assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in want), res
    q = np.random.default_rng(w + h).uniform(-4, 9, size=(h, w, 16)).astype(F)
    wt = random_weights(7, 16, w * h)
    assert np.array_equal(bits(r.develop_images(q, wt)), bits(ref.develop(q, wt)))


# ---- 4. values at the edges of binary32 ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def extreme_inputs():
    w, h = BIG
    c, var, prim, albedo = dr.synthetic_extreme(w, h, seed=w * 100 + h)
    e = dr.extras_extreme(c, var, w + h)
    for a in (c, var, prim, albedo, e):
        a.setflags(write=False)
    return c, var, prim, albedo, e


@pytest.mark.parametrize("sigma", [0, 1])
def test_the_filter_on_values_at_the_edges_of_binary32(sigma):
    """The inputs of denoise_ref.synthetic_extreme: weights that are +0 or denormal, den at its floor of 1e-6f, sums that overflow, a non-finite albedo in a valid
    pixel, pixels that are valid on input and invalid after a later level (they keep what they have; their neighbours go on without them)."""
    c, var, prim, albedo, e = extreme_inputs()
    r = pure_context()
    levels_ref = restated_levels(BIG, True, sigma)
    valid0 = dr.valid_mask(c, var)
    later = valid0 & ~dr.valid_mask(*levels_ref[5][:2])
    x, y = dr.EXTREME_NAN_ALBEDO
    assert later.sum() > 1 and later[y, x] and dr.is_denormal(levels_ref[5][2][..., 4]).any() and np.isinf(levels_ref[0][2][..., 6][valid0]).any()
    for levels in range(1, 7):
        want = levels_ref[levels - 1]
        image = r.denoise_images(c, var, prim, albedo, levels=levels, return_variance=True, **SIGMAS[sigma])
        assert all(same_or_both_nan(a, b) for a, b in zip(image, want[:2])), (levels, int((bits(image[0]) != bits(want[0])).sum()), int((bits(image[1]) != bits(want[1])).sum()))
        assert np.array_equal(np.isnan(image[0]), np.isnan(want[0])) and np.array_equal(bits(image[0][later]), bits(want[0][later])) and np.array_equal(bits(image[1][later]), bits(want[1][later]))
        for E in (5, 80):
            got = r.denoise_channels(c, var, prim, albedo, e[..., :E], levels=levels, return_image=True, **SIGMAS[sigma])
            assert same_or_both_nan(got[0], want[2][..., :E]), (levels, E, int(((bits(got[0]) != bits(want[2][..., :E])) & ~(np.isnan(got[0]) & np.isnan(want[2][..., :E]))).sum()))
            assert all(same_or_both_nan(a, b) for a, b in zip(got[1:], want[:2])), (levels, E)


@pytest.mark.parametrize("bins,channels", [(4, 5), (16, 7), (64, 16)])
def test_develop_images_on_denormals_and_overflows(bins, channels):
    q, w = ref.extreme_inputs(42, 23, bins, channels, bins * 100 + channels)
    got, want = pure_context().develop_images(q, w), ref.develop(q, w)
    assert dr.is_denormal(want).any() and np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want).any()
    assert same_or_both_nan(got, want), "%d of %d differ" % (int(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum()), want.size)


@functools.lru_cache(maxsize=None)
def faint_emitter():
    """The scene of tests/test_develop_gpu.py test_unit_weights_return_bins...: one black emissive quad filling the view, its emission the observer's x-bar table
    scaled by 4e-38 -- the fluxes lie around the smallest normal binary32 number, the bins' q = S M / n and the channels S / n below it."""
    c = cs.CustomScene("cornell", keep_quads=False)
    data, low, high, _ = ol.Oracle("cornell").spectrum("xbar")
    black = c.add_spectrum(np.zeros(2, dtype=np.float32), low, high)
    mat = c.add_material(albedo_spectrum=black, emission_spectrum=c.add_spectrum((data.astype(np.float64) * 4e-38).astype(F), low, high))
    c.add_quad((-50, -50, -5), (50, -50, -5), (50, 50, -5), (-50, 50, -5), mat)
    c.set_camera((0, 0, 0), (0, 0, -1), vfov_deg=40.0, aspect=42 / 23)
    return c, c.oracle()


def test_the_state_kernel_and_the_ratio_on_denormal_bins():
    c, orc = faint_emitter()
    res, B, spp = (42, 23), 16, 16
    r = Renderer(Options(scene_name="cornell", res=res, seed=SEED, jit_pass1=False, explicit_light_sampling=False))
    r.upload_scene_desc(c.desc(orc))
    r.set_noise_estimate(True)
    r.set_spectral_bins(B)
    image = start(r, spp, spp_per_launch=4)
    _, mean, counts, sums = r.spectral_read(sums=True)
    q = ref.raw_q(sums, spp)
    assert dr.is_denormal(q).any() and (sums != 0).any()
    for w in (np.eye(B, dtype=F), random_weights(5, B, 9)):
        assert np.array_equal(bits(r.develop(w)), bits(ref.develop(q, w)))
    assert dr.is_denormal(ref.develop(q, np.eye(B, dtype=F))).any()
    var = dr.variance_in_image_units(r.noise()[1])
    g = r.guides()
    e0 = sr.spectral_channels(sums, counts, spp)
    for kw in (dict(dr.DEFAULTS), dict(levels=3, **OTHER)):
        own = r.denoise_spectral(return_image=True, **kw)
        eL = r.denoise_channels(image, var, g["prim"], g["albedo"], e0, **kw)
        den = eL[..., B + np.arange(B) % (B // 4)]
        assert (dr.is_denormal(eL[..., :B]) & (den > 0) & (den < 1)).any()                       # a denormal numerator over a count channel in (0, 1)
        assert np.array_equal(bits(own[0]), bits(sr.spectral_ratio(eL, B))), kw
        assert same(own, sr.denoise_spectral(sums, counts, spp, image, var, g["prim"], g["albedo"], **kw)), kw
        w = random_weights(5, B, 10)
        assert np.array_equal(bits(r.develop(w, denoise=kw)), bits(ref.develop(own[0], w)))
