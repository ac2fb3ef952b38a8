"""The preconditions of tests/test_pipeline_matrix_gpu.py, shown without a GPU: every case of the scene and option matrix reaches what it is listed for (with
the oracle alone), the large image has pixels and workgroups of every kind, and the inputs at the edges of binary32 reach every branch they are there for (on
the numpy restatements).  These are conditions, not measurements; the counts are printed."""
import ctypes as C
import functools

import numpy as np
import pytest

import crafted
import denoise_ref as dr
import denoise_spectral_ref as sr
import develop_ref as ref

F = np.float32
W, H, SEED, SPP = 20, 12, 5, 12
BIG = (72, 40)
LARGE = (150, 134)
SIGMAS = (dict(sigma_l=dr.DEFAULTS["sigma_l"], sigma_a=dr.DEFAULTS["sigma_a"]), dict(sigma_l=4.0, sigma_a=0.037))


@functools.lru_cache(maxsize=None)
def guides(name, res):
    return dr.guides_ref(crafted.matrix_case(name).oracle, res[0], res[1])


def lambda_range(case):
    col = C.cast(case.oracle.color, C.POINTER(dr._OrcColorHead)).contents
    return F(col.lambda_min), F(col.lambda_step)


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", crafted.MATRIX_CASES)
def test_every_case_has_light_and_more_than_one_primitive(name):
    case = crafted.matrix_case(name)
    image = case.render_ref(W, H, SPP, seed=SEED)
    if name in crafted.MATRIX_BLACK:                                               # a plane under a light has no indirect light: every flux is 0, the counts are not
        assert not image[..., :3].any() and (image[..., 3] == 1).all()
        return
    assert (image[..., :3] != 0).any()                                             # some flux: q != 0
    for res in ((W, H), BIG):
        g = guides(name, res)
        ids = np.unique(g["prim"][g["prim"] != dr.MISS])
        assert len(ids) > 1, (name, res, ids)
    per_pixel = case.samples_ref(W, H, SPP, seed=SEED)[0][..., 1]
    assert (np.nanvar(per_pixel.astype(np.float64), axis=2) > 0).any()             # samples of a pixel differ: the noise estimate has a variance to find


def test_triangles_are_first_hits():
    case = crafted.matrix_case("triangles")
    tris = set(case.scene.kinds)
    for res in ((W, H), BIG):
        assert tris & set(guides("triangles", res)["prim"].ravel().tolist()), res


def texture_of_first_hits(case, g):
    hit = g["prim"][g["prim"] != dr.MISS]
    mats = [case.scene.materials[case.scene.quads[int(p)][2]] for p in np.unique(hit)]
    return {m["albedo_texture"] for m in mats if m["albedo_mode"] == 1}


def test_first_hits_land_on_five_textures():
    case = crafted.matrix_case("textures")
    seen = texture_of_first_hits(case, guides("textures", BIG))
    print("textures hit at 72 x 40: %d of %d" % (len(seen), len(case.scene.textures)))
    assert len(case.scene.textures) == 9 and len(seen) >= 5


def test_the_2006_cases_have_another_wavelength_range():
    for name in ("prims128-2006", "observer2006"):
        lmin, lstep = lambda_range(crafted.matrix_case(name))
        assert lmin != F(380) and lmin == F(390) and lstep == F(110)
    assert lambda_range(crafted.matrix_case("prims70")) == (F(380), F(100))


def deep_emission_samples(case, xyza, first):
    """samples whose first hit is no emitter and whose flux is not zero: without explicit light sampling, emission is the only source, so it was found at a
    deeper level of the path"""
    lights = np.array(sorted(case.light_prims()))
    return (first >= 0) & ~np.isin(first, lights) & (xyza[..., :3] != 0).any(axis=-1)


@pytest.mark.parametrize("name", ["cornell-no-els", "prims70-no-els"])
def test_without_explicit_light_sampling_emission_is_found_below_the_first_level(name):
    case = crafted.matrix_case(name)
    assert not case.flags["els"]
    xyza = case.samples_ref(W, H, SPP, seed=SEED)[0]
    first = dr.sample_first_hits(case.oracle, W, H, SPP, SEED)
    deep = deep_emission_samples(case, xyza, first)
    print("%s: %d of %d samples carry emission from below their first level" % (name, int(deep.sum()), deep.size))
    assert deep.any()


def test_mirrors_are_first_hits():
    case = crafted.matrix_case("mirror")
    g = guides("mirror", (W, H))
    on_mirror = (g["prim"] != dr.MISS) & (g["prim"] >= 9)
    assert on_mirror.any()
    plain = dr.guides_ref(crafted.matrix_case("cornell-no-ffc").oracle, W, H)       # the same scene, Lambertian
    assert np.array_equal(dr.bits(g["albedo"]), dr.bits(plain["albedo"]))          # the guides report the material's albedo whatever its kind
    assert (g["albedo"][on_mirror] != 0).any()
    assert not np.array_equal(dr.bits(case.render_ref(W, H, 4)), dr.bits(crafted.matrix_case("cornell-no-ffc").oracle.render(W, H, 4, seed=SEED)))


def test_the_uplifts_and_the_observer_change_the_guide_albedo():
    base = dr.guides_ref(crafted.matrix_case("cornell-no-els").oracle, W, H)["albedo"]
    for name in ("jh", "meng", "observer2006"):
        assert not np.array_equal(dr.bits(guides(name, (W, H))["albedo"]), dr.bits(base)), name


# ---- 3. sizes ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_large_size_has_pixels_and_workgroups_of_every_kind():
    w, h = LARGE
    assert w % 8 and h % 8 and (w * h) % 256 and ((w + 15) // 16, (h + 15) // 16) == (10, 9)
    print("150 x 134: pixels with all 25 taps inside at step 32: %d, at step 16: %d" % (dr.interior_pixels(w, h, 32), dr.interior_pixels(w, h, 16)))
    assert dr.interior_pixels(w, h, 32) >= 1 and dr.interior_pixels(72, 40, 16) == 0
    n = dr.lds_tile_classes(w, h, 2)
    print("150 x 134, step 2, 24 x 24 tiles: %r" % (n,))
    assert all(v > 0 for v in n.values())
    c, var, prim, albedo = dr.synthetic_large(w, h, seed=w * 100 + h)
    for level in range(6):                                                         # at every level some pixel takes all 25 taps
        cnt = dr.level_trace(c, var, prim, albedo, 1 << level, **SIGMAS[0])["counted"]
        assert cnt.all(axis=0).any(), level


# ---- 4. values ---------------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def extreme():
    w, h = BIG
    c, var, prim, albedo = dr.synthetic_extreme(w, h, seed=w * 100 + h)
    e = dr.extras_extreme(c, var, w + h)
    for a in (c, var, prim, albedo, e):
        a.setflags(write=False)
    return c, var, prim, albedo, e


@pytest.mark.parametrize("sig", SIGMAS)
def test_the_extreme_inputs_reach_every_branch(sig):
    c, var, prim, albedo, e = extreme()
    w, h = BIG
    patch = lambda name: (slice(dr.EXTREME_PATCHES[name][1], dr.EXTREME_PATCHES[name][3]), slice(dr.EXTREME_PATCHES[name][0], dr.EXTREME_PATCHES[name][2]))
    assert np.isfinite(c[patch("colour_max")]).all() and np.isfinite(var[patch("variance_max")]).sum() == var[patch("variance_max")].size - 1
    ref_l = (np.ascontiguousarray(c), var, e)
    valid0 = dr.valid_mask(c, var)
    x, y = dr.EXTREME_NAN_ALBEDO
    assert valid0[y, x] and not np.isfinite(albedo[y, x]).all()
    seen = dict(zero_weight=0, den_floor=0, denormal_weight=0, albedo_inf=0, lonely=0, later_invalid=0, variance_overflow=0)
    valid = valid0
    turned_at = np.zeros((h, w), dtype=np.int32)
    for level in range(6):
        tr = dr.level_trace(ref_l[0], ref_l[1], prim, albedo, 1 << level, **sig)
        cnt = tr["counted"]
        sw = np.where(cnt, tr["w"], F(0)).sum(axis=0)
        zero = cnt & np.isinf(tr["xl2"]) & (tr["w"] == 0) & ~np.signbit(tr["w"])
        seen["zero_weight"] += int((zero & (sw >= F(9.0 / 64.0))[None]).sum())
        seen["den_floor"] += int((valid & (tr["den"] == F(1e-6))).sum())
        seen["denormal_weight"] += int((cnt & dr.is_denormal(tr["w"])).sum())
        seen["albedo_inf"] += int((cnt & np.isinf(tr["da2s"]) & np.isfinite(tr["xl2"])).sum())
        lx, ly = dr.EXTREME_LONELY
        assert cnt[:, ly, lx].sum() == 1 and cnt[12, ly, lx]                       # only the centre counts, at every step
        seen["lonely"] += 1
        seen["variance_overflow"] += int((valid & np.isinf(tr["gs"])).sum())      # the 3x3 sum of near-FLT_MAX variances overflows: den = +inf
        nxt = sr.channels_level(ref_l[0], ref_l[1], prim, albedo, ref_l[2], 1 << level, **sig)
        now = dr.valid_mask(nxt[0], nxt[1])
        assert not (now & ~valid).any()                                            # an invalid pixel stays invalid ...
        gone = valid & ~now
        assert np.array_equal(dr.bits(nxt[0][~valid]), dr.bits(ref_l[0][~valid])) and np.array_equal(dr.bits(nxt[1][~valid]), dr.bits(ref_l[1][~valid]))  # ... as it is
        turned_at[gone] = level + 1
        seen["later_invalid"] += int(gone.sum())
        assert not (valid & ~np.isfinite(nxt[1]) & np.isfinite(nxt[0][..., :3]).all(axis=-1)).any()   # never through the variance alone (synthetic_extreme)
        if level == 0:
            nan = np.isnan(nxt[0][..., :3]).any(axis=-1) & valid0
            assert np.array_equal(np.argwhere(nan), np.array([[y, x]])), np.argwhere(nan)             # the pixel of the non-finite albedo, and no other
            assert np.isinf(nxt[2][..., 6][valid0]).any() and np.isfinite(e[..., 6]).all()           # a tap sum of +-FLT_MAX rounds past FLT_MAX
        ref_l, valid = nxt, now
    print("extreme inputs, sigma %r: %r; pixels invalid after level 1..6: %r" % (sig, seen, [int((turned_at == l).sum()) for l in range(1, 7)]))
    assert all(v > 0 for v in seen.values()), seen
    assert (turned_at[patch("colour_max")] >= 1).any() and (turned_at >= 2).any()                     # valid on input, invalid after a level; some after a later one
    den4 = dr.is_denormal(ref_l[2][..., 4])
    print("filtered channel of denormals: %d of %d still denormal" % (int(den4.sum()), den4.size))
    assert den4.any()


def test_a_single_tap_cannot_carry_a_finite_variance_to_infinity():
    """sv / (sw * sw) with the centre tap alone, w = 9/64: fl(fl(w * w * v) / (w * w)) for the 2^16 largest finite v"""
    v = (np.uint32(0x7F7FFFFF) - np.arange(1 << 16, dtype=np.uint32)).view(F)
    w = F(9.0 / 64.0)
    with np.errstate(all="ignore"):
        out = ((w * w) * v) / (w * w)
    assert out.dtype == F and np.isfinite(out).all()


@pytest.mark.parametrize("bins,channels", [(4, 5), (16, 7), (64, 16)])
def test_the_extreme_develop_inputs_give_denormals_and_infinities(bins, channels):
    q, w = ref.extreme_inputs(42, 23, bins, channels, bins * 100 + channels)
    assert dr.is_denormal(q).any() and dr.is_denormal(w).any() and np.isfinite(q).all() and np.isfinite(w).all()
    with np.errstate(all="ignore"):
        prod = q[..., None, :] * w
    assert dr.is_denormal(prod).any() and np.isinf(prod).any()
    out = ref.develop(q, w)
    print("develop at B = %d, C = %d: %d denormal, %d +inf, %d -inf, %d NaN of %d" % (bins, channels, int(dr.is_denormal(out).sum()), int(np.isposinf(out).sum()),
                                                                                      int(np.isneginf(out).sum()), int(np.isnan(out).sum()), out.size))
    assert dr.is_denormal(out).any() and np.isposinf(out).any() and np.isneginf(out).any()
