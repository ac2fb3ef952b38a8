"""libm = glibc-2.35 on the GPU: the _glibc kernel twins against the shim oracle (tests/glibc_oracle.py), which evaluates glibc 2.35's
x86-64 sinf / cosf / acosf as include/ssx_glibc_math.h restates them -- bit for bit, per sample and per image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import crafted
import custom_scene as cs
import glibc_oracle as go
from simple_spectral_amd import Options, Renderer, SsxError, _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLIBC = "glibc-2.35"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def render(**kw):
    r = Renderer(Options(**kw))
    r.render_start()
    r.render_wait()
    return r.xyza.copy(), r


def jit_counters():
    a, b = C.c_uint64(), C.c_uint64()
    _capi.hip_lib().ssx_jit_counters(C.byref(a), C.byref(b))
    return a.value, b.value


def test_shim_oracle_is_there():
    assert os.path.exists(go.library_path()), "the glibc-mode oracle was not built (__graft_entry__.build())"
    go.load()


@pytest.mark.parametrize("scene,observer,W,H,spp,seed,io,els", [
    ("cornell", 1931, 24, 24, 4, 0, False, True),
    ("cornell-srgb", 1931, 32, 24, 4, 1, False, True),
    ("plane-srgb", 1931, 32, 24, 4, 2, False, True),
    ("cornell-srgb", 2006, 24, 16, 3, 3, False, True),     # CIE 2006
    ("cornell-srgb", 1931, 24, 16, 4, 4, True, True),      # indirect only
    ("plane-srgb", 1931, 24, 16, 4, 5, False, False),      # no explicit light sampling (plane-srgb's textured quad is then a Mirror)
    ("cornell-srgb", 1931, 24, 16, 4, 6, False, False),
])
def test_debug_samples_equal_the_shim_oracle(scene, observer, W, H, spp, seed, io, els):
    """ssx_debug_samples in glibc mode: every sample's XYZA, final PCG32 state and level count as the shim oracle has them."""
    tex = None if scene == "cornell" else "test-img.png"
    r = Renderer(Options(scene_name=scene, observer=observer, res=(W, H), spp=spp, seed=seed, indirect_only=io, texture=tex,
                         explicit_light_sampling=els, libm=GLIBC))
    xyza, state, levels = r.debug_samples()
    o = go.Oracle(scene, observer=observer, texture=tex)
    if not els and scene == "plane-srgb":   # (the reference's scene.cpp:346-355; the oracle is told, the host does it itself)
        o.lib.orc_scene_set_material_kind(o.scene, o.lib.orc_scene_quad_material(o.scene, 0), 1)
    rx, rs, st = o.samples(W, H, spp, seed=seed, indirect_only=io, els=els)
    assert np.array_equal(state, rs)
    assert np.array_equal(bits(xyza), bits(rx))
    # levels = interactions that continued (tests/test_gpu_units.py): every sample has its count, bounded by the oracle's interactions
    assert np.bincount(levels.ravel(), minlength=10).sum() == W * H * spp
    assert int(levels.astype(np.int64).sum()) <= st.interactions
    assert r.plan_info()["kernel"].endswith("_glibc")


@pytest.mark.parametrize("uplift", ["jh", "meng", "rgb"])
def test_uplifts_and_rgb_mode_equal_the_shim_oracle(uplift, tmp_path):
    """Jakob-Hanika and Meng uplifts, and the RGB render mode, in glibc mode."""
    kw, okw = {}, {}
    if uplift == "meng":
        import ref_lib
        from simple_spectral_amd import meng
        table = ref_lib.meng_table()
        path = str(tmp_path / "grid.bin")
        meng.save_table(path, table)
        kw, okw = dict(uplift="meng", meng_grid_path=path), dict(meng=table)
    elif uplift == "jh":
        kw = dict(uplift="jh", jh_res=16)
    else:
        kw, okw = dict(render_mode="rgb"), dict(rgb=True)
    r = Renderer(Options(scene_name="cornell-srgb", res=(32, 24), spp=4, seed=7, texture="test-img.png", libm=GLIBC, **kw))
    r.render_start(); r.render_wait()
    if uplift == "jh":
        okw = dict(jh=r.scene.jh_model())
    ref = go.Oracle("cornell-srgb", texture="test-img.png", **okw).render(32, 24, 4, seed=7)
    ok = (bits(r.xyza) == bits(ref)) | (np.isnan(r.xyza) & np.isnan(ref))
    assert ok.all()


def test_triangle_scene_and_degenerate_lights_equal_the_shim_oracle():
    for c in (crafted.triangle_scene(), crafted.degenerate_light_scene("edge_ab"), crafted.origin_light_scene()):
        r = Renderer(Options(scene_name="cornell", res=(16, 16), spp=4, seed=2, libm=GLIBC))
        o = go.custom_oracle(c)
        r.upload_scene_desc(c.desc(o))
        xyza, state, _ = r.debug_samples()
        rx, rs, _ = o.samples(16, 16, 4, seed=2)
        assert np.array_equal(state, rs) and np.array_equal(bits(xyza), bits(rx))


def test_baseline_config1_bit_exact():
    """BASELINE.json configs[0]: cornell-srgb 128x128 spp=16 CIE 1931, lizard texture, in glibc mode."""
    got, _ = render(scene_name="cornell-srgb", res=(128, 128), spp=16, texture="crystal-lizard-512.png", libm=GLIBC)
    ref = go.Oracle("cornell-srgb", texture="crystal-lizard-512.png").render(128, 128, 16)
    assert np.array_equal(bits(got), bits(ref))


def test_headline_image_bit_exact_and_different_from_the_default_mode():
    """The bench's workload (cornell-srgb 512x512 spp=256, lizard texture, seed 0) in glibc mode: the WHOLE image equals the shim
    oracle's; and it differs from the default mode's image of the same seed (the switch takes effect)."""
    kw = dict(scene_name="cornell-srgb", res=(512, 512), spp=256, texture="crystal-lizard-512.png")
    got, r = render(libm=GLIBC, **kw)
    assert r.plan_info()["kernel"].endswith("_glibc")
    ref = go.Oracle("cornell-srgb", texture="crystal-lizard-512.png").render(512, 512, 256, nthreads=0)
    assert np.array_equal(bits(got), bits(ref))
    base, rb = render(**kw)
    assert not rb.plan_info()["kernel"].endswith("_glibc")
    differ = (bits(got) != bits(base)).any(axis=-1)
    print("pixels that differ between the modes: %d of %d (%.2f %%)" % (differ.sum(), differ.size, 100.0 * differ.mean()))
    assert differ.any()


def test_the_same_context_switches_between_modes():
    r = Renderer(Options(scene_name="plane-srgb", res=(32, 16), spp=4, seed=9, texture="test-img.png"))
    r.render_start(); r.render_wait(); a = r.xyza.copy()
    r.options.libm = GLIBC
    r.render_start(); r.render_wait(); g = r.xyza.copy()
    r.options.libm = "build"
    r.render_start(); r.render_wait(); a2 = r.xyza.copy()
    assert np.array_equal(bits(a), bits(a2)) and not np.array_equal(bits(a), bits(g))
    assert np.array_equal(bits(g), bits(go.Oracle("plane-srgb", texture="test-img.png").render(32, 16, 4, seed=9)))


def test_unknown_libm_and_old_struct_size():
    r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1))
    with pytest.raises(SsxError) as e:
        r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(libm=7))))
    assert e.value.code == _capi.SSX_ERR_ARG
    with pytest.raises(ValueError):
        Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, libm="glibc-2.41")).params()
    # a caller built before the field: struct_size = offsetof(libm) -> the default mode, whatever follows
    p = r.params(libm=1)
    p.struct_size = _capi.SsxRenderParams.libm.offset
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(p))); r.render_wait()
    old = r.xyza.copy()
    ref, _ = render(scene_name="cornell", res=(8, 8), spp=1)
    assert np.array_equal(bits(old), bits(ref))


def _custom_topology_case():
    """(runs in a child process: see the test below)"""
    c = cs.CustomScene("cornell-srgb")
    pos, st, m = c.quads[0]
    pos = pos.copy(); pos[0, 1] += 0.75
    c.quads[0] = (pos, st, m)
    o = go.custom_oracle(c)
    r = Renderer(Options(scene_name="cornell-srgb", res=(32, 24), spp=4, seed=3, texture="test-img.png", jit_pass1=True, libm=GLIBC))
    n0 = jit_counters()[0]
    r.upload_scene_desc(c.desc(o))
    assert r.plan_info()["pass1"].startswith("scene topology")
    n1 = jit_counters()[0]
    assert n1 == n0 + 1                                          # the default mode's kernels, at upload
    r.render_start(); r.render_wait()
    assert jit_counters()[0] == n1 + 1                           # the glibc mode's, at the first glibc-mode render
    assert np.array_equal(bits(r.xyza), bits(o.render(32, 24, 4, seed=3)))
    xyza, state, _ = r.debug_samples()
    rx, rs, _ = o.samples(32, 24, 4, seed=3)
    assert np.array_equal(state, rs) and np.array_equal(bits(xyza), bits(rx))
    r.render_start(); r.render_wait()
    assert jit_counters()[0] == n1 + 1                           # kept: no third compilation
    r.options.libm = "build"                                     # and the default mode still runs its own code object
    r.render_start(); r.render_wait()
    assert np.array_equal(bits(r.xyza), bits(c.oracle().render(32, 24, 4, seed=3)))
    assert jit_counters()[0] == n1 + 1
    print("custom topology case: ok")


def _custom_topology_background_case():
    """(child process) SSX_JIT_BACKGROUND: a scene rendered in glibc mode asks for the glibc kernels of its pattern, swaps to them, and a
    later default-mode render compiles the default mode's on the calling thread."""
    c = cs.CustomScene("cornell-srgb")
    pos, st, m = c.quads[2]
    pos = pos.copy(); pos[1, 2] -= 0.5
    c.quads[2] = (pos, st, m)
    o = go.custom_oracle(c)
    r = Renderer(Options(scene_name="cornell-srgb", res=(32, 24), spp=4, seed=5, texture="test-img.png", libm=GLIBC))
    r.upload_scene_desc(c.desc(o))
    n0 = jit_counters()[0]
    r.render_start(); r.render_wait()                            # generic glibc kernel meanwhile
    assert r.plan_info()["kernel"] == "ssx_render_kernel_nq_glibc" or r.plan_info()["kernel"] == "ssx_render_kernel_glibc"
    ref = o.render(32, 24, 4, seed=5)
    assert np.array_equal(bits(r.xyza), bits(ref))
    r.jit_status(wait_ms=-1)                                     # ask now (the render was below the sample mark) and wait
    assert jit_counters()[0] == n0 + 1                           # the glibc mode's code object
    r.render_start(); r.render_wait()
    assert r.plan_info()["pass1"].startswith("scene topology") and r.plan_info()["kernel"].startswith("ssx_render_kernel_jit")
    assert np.array_equal(bits(r.xyza), bits(ref))
    r.options.libm = "build"
    r.render_start(); r.render_wait()
    assert jit_counters()[0] == n0 + 2                           # the default mode's, compiled for this render
    assert np.array_equal(bits(r.xyza), bits(c.oracle().render(32, 24, 4, seed=5)))
    print("custom topology case: ok")


@pytest.mark.parametrize("case", ["_custom_topology_case", "_custom_topology_background_case"])
def test_custom_topology_compiled_per_mode(case, tmp_path):
    """A topology of its own (the Cornell box with one corner moved), compiled at upload or in the background: each libm gets its own code
    object of the pattern, compiled once, and its images equal its oracle's.
    In a child process with a disk cache of its own: the code objects it makes must not reach the other tests of the session, which
    expect that pattern to be uncompiled (tests/test_gpu_parity.py::test_pass1_variants_specialised_for_builtin_topologies_generic_otherwise)."""
    import sys
    env = dict(os.environ, SSX_CACHE_DIR=str(tmp_path / "jit_cache"))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_glibc_mode_gpu as t; t.%s()" % (ROOT, os.path.join(ROOT, "tests"), case)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "custom topology case: ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])


def test_cli_libm_on_two_devices_equals_python(tmp_path):
    from PIL import Image
    cli = os.path.join(ROOT, "simple-spectral")
    out = str(tmp_path / "g.png")
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    p = subprocess.run([cli, "-s=cornell-srgb", "-w=40", "-h=24", "-spp=4", "-o=" + out, "--texture=data/scenes/test-img.png", "--seed=4",
                        "--gpus=2", "--libm=glibc-2.35"], cwd=ROOT, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    _, r = render(scene_name="cornell-srgb", res=(40, 24), spp=4, seed=4, texture="test-img.png", libm=GLIBC)
    from test_cli import _png_of
    assert np.array_equal(np.asarray(Image.open(out)), _png_of(r.framebuffer))
    bad = subprocess.run([cli, "-s=cornell", "-w=8", "-h=8", "-spp=1", "-o=" + str(tmp_path / "b.png"), "--libm=musl"], cwd=ROOT,
                         capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0
