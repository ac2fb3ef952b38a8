"""The path kernels with the render switches compiled in (csrc/ssx_kernels.hip render_body's PLAIN, the "_plain" twins; csrc/ssx_api.hip variant_of).
A plain render of a plain scene -- explicit light sampling, not indirect_only, no mirror, no triangle light, uplift "ours", XYZ mode, flat-field
correction, no kept samples -- runs them and must produce the oracle's bits; any one trait sends the render to the general kernels, at the next render
of a context that has rendered plain as well.  ssx_debug_samples keeps every sample (keep_samples is one of the traits), so its renders are the general
kernels' by construction: the per-sample arrays pin those, the images pin the compiled-in ones, and the two must agree with the same oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from plain_switches_worker import BUILTIN, builtin_render
from unit_cases import same_or_both_nan
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T = "test-img.png"
W, H, SPP, SEED = 16, 16, 4, 7   # the trait cases


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render(r):
    r.render_start(); r.render_wait()
    return r.xyza.copy(), r.plan_info()["switches"]


@pytest.fixture(scope="module")
def builtin():
    """the built-in renders in this process (compiled-in kernels), once: scene -> (image, switches, xyza, state, levels, switches after the next render)"""
    out = {}
    for scene, w, h, spp, seed in BUILTIN:
        r, image, switches, xyza, state, levels = builtin_render(scene, w, h, spp, seed)
        after_samples = r.plan_info()["switches"]
        again, back = render(r)
        assert np.array_equal(bits(again), bits(image))
        out[scene] = (image, switches, xyza, state, levels, after_samples, back)
    return out


@pytest.mark.parametrize("scene,w,h,spp,seed", BUILTIN)
def test_builtin_scenes_run_the_compiled_in_kernel_and_equal_the_oracle(builtin, scene, w, h, spp, seed):
    image, switches, xyza, state, levels, after_samples, back = builtin[scene]
    assert switches == "compiled in" and after_samples == "run time" and back == "compiled in"   # (ssx_debug_samples: the general kernel; the render after it: plain again)
    orc = ol.Oracle(scene, texture=T)
    assert np.array_equal(bits(image), bits(orc.render(w, h, spp, seed=seed)))
    ref_xyza, ref_state, st = orc.samples(w, h, spp, seed=seed)
    assert np.array_equal(state, ref_state) and np.array_equal(bits(xyza), bits(ref_xyza))
    assert levels.shape == (h, w, spp) and int(levels.astype(np.int64).sum()) <= st.interactions and levels.max() <= 9


def test_forced_general_kernels_return_identical_arrays(builtin, tmp_path):
    out = str(tmp_path / "general.npz")
    env = dict(os.environ, SSX_DEBUG_ENV="1", SSX_PLAIN_KERNEL="0")
    subprocess.run([sys.executable, os.path.join(HERE, "plain_switches_worker.py"), out], env=env, check=True, capture_output=True, timeout=300)
    z = np.load(out)
    for scene, *_ in BUILTIN:
        image, _sw, xyza, state, levels, _a, _b = builtin[scene]
        assert str(z[scene + "/switches"]) == "run time"
        assert np.array_equal(bits(z[scene + "/image"]), bits(image)) and np.array_equal(bits(z[scene + "/xyza"]), bits(xyza))
        assert np.array_equal(z[scene + "/state"], state) and np.array_equal(z[scene + "/levels"], levels)


@pytest.mark.parametrize("option,value,oracle_kw", [("indirect_only", True, dict(indirect_only=True)), ("explicit_light_sampling", False, dict(els=False)),
                                                    ("flat_field_correction", False, dict(flat_field=False))])
def test_a_render_switch_falls_back_and_back_again(option, value, oracle_kw):
    """the per-render traits, each alone, flipped on a context that has just rendered plain -- the case in which a stale choice would go wrong"""
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), spp=SPP, seed=SEED, texture=T))
    orc = ol.Oracle("cornell-srgb", texture=T)
    plain_ref = orc.render(W, H, SPP, seed=SEED)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(plain_ref))
    was = getattr(r.options, option)
    setattr(r.options, option, value)
    got, sw = render(r)
    ref = orc.render(W, H, SPP, seed=SEED, **oracle_kw)
    assert sw == "run time" and np.array_equal(bits(got), bits(ref)) and not np.array_equal(bits(ref), bits(plain_ref))
    setattr(r.options, option, was)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(plain_ref))
    # ... and alone, on a context of its own
    fresh = Renderer(Options(scene_name="cornell-srgb", res=(W, H), spp=SPP, seed=SEED, texture=T, **{option: value}))
    got, sw = render(fresh)
    assert sw == "run time" and np.array_equal(bits(got), bits(ref))


def _mirror_scene():
    import custom_scene as cs
    c = cs.CustomScene("cornell-srgb")
    mirror = c.add_material(kind=1, albedo_spectrum=c.materials[0]["albedo_spectrum"])
    pos, st, _m = c.quads[9]                          # one face of a block becomes a mirror (MaterialMirror, src/material.cpp:146-167)
    c.quads[9] = (pos, st, mirror)
    return "cornell-srgb", c, {}


def _triangle_light_scene():
    import crafted
    return "cornell", crafted.triangle_scene(), {}


@pytest.mark.parametrize("make", [_mirror_scene, _triangle_light_scene])
def test_a_scene_trait_falls_back_and_back_again(make):
    """a mirror quad / a top-level triangle light: uploaded into a context that has rendered its plain base scene, then the base scene again"""
    base, c, _ = make()
    tex = None if base == "cornell" else T
    r = Renderer(Options(scene_name=base, res=(W, H), spp=SPP, seed=SEED, texture=tex))
    base_ref = ol.Oracle(base, texture=tex).render(W, H, SPP, seed=SEED)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(base_ref))
    orc = c.oracle()
    desc = c.desc(orc)
    assert _capi.hip_lib().ssx_scene_traits(C.byref(desc)) in (_capi.SSX_TRAIT_MIRROR, _capi.SSX_TRAIT_TRI_LIGHT)
    r.upload_scene_desc(desc)
    assert r.plan_info()["switches"] == "run time"
    got, sw = render(r)
    ref = orc.render(W, H, SPP, seed=SEED)
    assert sw == "run time" and np.array_equal(bits(got), bits(ref)) and not np.array_equal(bits(ref), bits(base_ref))
    r.upload_scene_desc(r.scene.desc)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(base_ref))
    # ... and alone, on a context that never rendered anything else
    fresh = Renderer(Options(scene_name=base, res=(W, H), spp=SPP, seed=SEED, texture=tex))
    fresh.upload_scene_desc(desc)
    got, sw = render(fresh)
    assert sw == "run time" and np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("kw", [dict(render_mode="rgb"), dict(uplift="jh", jh_res=16)])
def test_rgb_mode_and_another_uplift_fall_back_and_back_again(kw):
    """the two traits that come with the scene's colour tables: that scene uploaded into a context that has rendered the plain one, and back"""
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), spp=SPP, seed=SEED, texture=T))
    plain_ref = ol.Oracle("cornell-srgb", texture=T).render(W, H, SPP, seed=SEED)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(plain_ref))
    other = Renderer(Options(scene_name="cornell-srgb", res=(W, H), spp=SPP, seed=SEED, texture=T, **kw))
    orc = ol.Oracle("cornell-srgb", texture=T, rgb=True) if "render_mode" in kw else ol.Oracle("cornell-srgb", texture=T, jh=other.scene.jh_model())
    ref = orc.render(W, H, SPP, seed=SEED)
    got, sw = render(other)                                      # alone
    assert sw == "run time" and same_or_both_nan(got, ref) and not np.array_equal(bits(ref), bits(plain_ref))
    r.upload_scene_desc(other.scene.desc)                        # flipped on the context that rendered plain
    assert r.plan_info()["switches"] == "run time"
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params())))
    r._check(r._lib.ssx_render_wait(r._ctx, r.xyza.ctypes.data))
    assert r.plan_info()["switches"] == "run time" and same_or_both_nan(r.xyza, ref)
    r.upload_scene_desc(r.scene.desc)
    got, sw = render(r)
    assert sw == "compiled in" and np.array_equal(bits(got), bits(plain_ref))


def test_scene_compiled_at_upload_has_one_cache_entry_per_choice(tmp_path):
    """A Cornell box with one corner moved gets kernels of its own pattern from the run-time compiler: the compiled-in pair for its plain renders (asked for
    at upload), the general pair when a render with a switch first needs it -- different compile flags, different cache entries -- and both equal the oracle."""
    import custom_scene as cs
    cache = tmp_path / "cache"
    old = os.environ.get("SSX_CACHE_DIR")
    os.environ["SSX_CACHE_DIR"] = str(cache)
    try:
        c = cs.CustomScene("cornell-srgb")
        pos, st, m = c.quads[3]
        pos = pos.copy(); pos[1, 2] += 0.375             # a pattern of this test's own (the in-memory cache is per process)
        c.quads[3] = (pos, st, m)
        orc = c.oracle()
        r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), spp=SPP, seed=SEED, texture=T, jit_pass1=True))
        r.upload_scene_desc(c.desc(orc))
        info = r.plan_info()
        assert info["pass1"].startswith("scene topology") and info["kernel"].startswith("ssx_render_kernel_jit") and info["switches"] == "compiled in"
        assert len(list(cache.glob("pass1-*.co"))) == 1
        got, sw = render(r)
        ref = orc.render(W, H, SPP, seed=SEED)
        assert sw == "compiled in" and np.array_equal(bits(got), bits(ref))
        assert len(list(cache.glob("pass1-*.co"))) == 1
        r.options.indirect_only = True                   # the general pair of the pattern: compiled now
        got, sw = render(r)
        assert sw == "run time" and np.array_equal(bits(got), bits(orc.render(W, H, SPP, seed=SEED, indirect_only=True)))
        assert r.plan_info()["kernel"].startswith("ssx_render_kernel_jit") and len(list(cache.glob("pass1-*.co"))) == 2
        r.options.indirect_only = False
        xyza, state, _levels = r.debug_samples()
        ref_xyza, ref_state, _st = orc.samples(W, H, SPP, seed=SEED)
        assert np.array_equal(state, ref_state) and np.array_equal(bits(xyza), bits(ref_xyza))
        got, sw = render(r)
        assert sw == "compiled in" and np.array_equal(bits(got), bits(ref)) and len(list(cache.glob("pass1-*.co"))) == 2
    finally:
        if old is None:
            os.environ.pop("SSX_CACHE_DIR", None)
        else:
            os.environ["SSX_CACHE_DIR"] = old
