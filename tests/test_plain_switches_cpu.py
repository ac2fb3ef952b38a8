"""Which scenes and renders may run the path kernels with the render switches compiled in: the trait derivation of csrc/ssx_api.hip (scene_traits_of,
render_traits_of) through ssx_scene_traits / ssx_render_traits, which are host arithmetic on the caller's structs -- no device, no context.  A plain
scene and plain parameters first, then each trait in turn, alone.  (What a context makes of the traits -- spectral output, SSX_PLAIN_KERNEL=0, kept
samples -- needs a device: tests/test_plain_switches_gpu.py.)"""
import ctypes as C

import pytest

import crafted
import custom_scene as cs
from simple_spectral_amd import Options, _capi, build as sbuild
from simple_spectral_amd.renderer import Scene


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(sbuild.HIP_LIB)
    lib.ssx_scene_traits.argtypes = [C.c_void_p]
    lib.ssx_render_traits.argtypes = [C.c_void_p]
    return lib


def scene_traits(lib, desc):
    return lib.ssx_scene_traits(C.byref(desc) if not hasattr(desc, "contents") else desc)


def params(**kw):
    p = _capi.SsxRenderParams()
    p.struct_size = C.sizeof(_capi.SsxRenderParams)
    p.width, p.height, p.spp, p.tile_stride = 16, 16, 4, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_the_entry_points_are_declared():
    for s in ("ssx_scene_traits", "ssx_render_traits", "ssx_switches_info"):
        assert s in _capi.HIP_SYMBOLS
    bits = [_capi.SSX_TRAIT_INDIRECT_ONLY, _capi.SSX_TRAIT_NO_ELS, _capi.SSX_TRAIT_MIRROR, _capi.SSX_TRAIT_TRI_LIGHT, _capi.SSX_TRAIT_UPLIFT, _capi.SSX_TRAIT_RGB_MODE,
            _capi.SSX_TRAIT_NO_FLAT_FIELD, _capi.SSX_TRAIT_KEEP_SAMPLES, _capi.SSX_TRAIT_LIBM, _capi.SSX_TRAIT_SPECTRAL_BINS, _capi.SSX_TRAIT_FORCED_OFF]
    assert bits == [1 << i for i in range(11)]


@pytest.mark.parametrize("scene", ["cornell", "cornell-srgb", "plane-srgb"])
def test_builtin_scenes_are_plain(lib, scene):
    s = Scene(scene, texture=None if scene == "cornell" else "test-img.png")
    assert scene_traits(lib, s.desc) == 0


def test_custom_scenes_of_lambertian_quads_and_quad_lights_are_plain(lib):
    c = cs.CustomScene("cornell-srgb")
    pos, st, m = c.quads[0]
    pos = pos.copy(); pos[0, 0] += 1.0               # a moved corner changes the mesh pattern, not the traits
    c.quads[0] = (pos, st, m)
    assert scene_traits(lib, c.desc(c.oracle())) == 0
    c = crafted.degenerate_light_scene("room")       # two quad lights, one of them degenerate
    assert scene_traits(lib, c.desc(c.oracle())) == 0


def test_one_mirror_quad(lib):
    c = cs.CustomScene("cornell-srgb")
    mirror = c.add_material(kind=1, albedo_spectrum=c.materials[0]["albedo_spectrum"])
    assert scene_traits(lib, c.desc(c.oracle())) == 0    # a mirror material no primitive uses: no kernel ever sees it
    pos, st, _m = c.quads[9]
    c.quads[9] = (pos, st, mirror)
    assert scene_traits(lib, c.desc(c.oracle())) == _capi.SSX_TRAIT_MIRROR


def test_triangle_light_but_not_a_triangle_occluder(lib):
    c = crafted.triangle_scene()
    assert scene_traits(lib, c.desc(c.oracle())) == _capi.SSX_TRAIT_TRI_LIGHT
    c = cs.CustomScene("cornell")
    c.add_tri((0.1, 0.1, 0.1), (0.3, 0.1, 0.1), (0.1, 0.3, 0.1), 0)   # a Lambertian triangle is no trait: only sample_light looks at the kind of a LIGHT
    assert scene_traits(lib, c.desc(c.oracle())) == 0


def test_uplift_and_rgb_mode(lib):
    base = Scene("cornell-srgb", texture="test-img.png")
    for uplift, want in ((_capi.SSX_UPLIFT_OURS, 0), (_capi.SSX_UPLIFT_JH, _capi.SSX_TRAIT_UPLIFT), (_capi.SSX_UPLIFT_MENG, _capi.SSX_TRAIT_UPLIFT),
                         (_capi.SSX_MODE_RGB, _capi.SSX_TRAIT_RGB_MODE)):
        d = _capi.SsxSceneDesc.from_buffer_copy(base.desc.contents)   # (the derivation reads the field, not the tables that would come with it)
        d.uplift = uplift
        assert scene_traits(lib, d) == want


def test_render_parameters_each_alone(lib):
    assert lib.ssx_render_traits(C.byref(params())) == 0
    assert lib.ssx_render_traits(C.byref(params(seed=123, spp=77, tile_first=1, tile_stride=4, tile_skew=3, spp_per_launch=5))) == 0   # what a render is not compiled for
    for field, want in (("indirect_only", _capi.SSX_TRAIT_INDIRECT_ONLY), ("no_explicit_light_sampling", _capi.SSX_TRAIT_NO_ELS),
                        ("no_flat_field_correction", _capi.SSX_TRAIT_NO_FLAT_FIELD), ("libm", _capi.SSX_TRAIT_LIBM)):
        assert lib.ssx_render_traits(C.byref(params(**{field: 1}))) == want
    assert lib.ssx_render_traits(C.byref(params(indirect_only=1, no_explicit_light_sampling=1))) == _capi.SSX_TRAIT_INDIRECT_ONLY | _capi.SSX_TRAIT_NO_ELS


def test_bad_arguments(lib):
    assert lib.ssx_scene_traits(None) == -1 and lib.ssx_render_traits(None) == -1
    p = params(); p.struct_size -= 4
    assert lib.ssx_render_traits(C.byref(p)) == -1
    d = _capi.SsxSceneDesc.from_buffer_copy(Scene("cornell").desc.contents); d.struct_size = 8
    assert scene_traits(lib, d) == -1


def test_options_map_onto_the_parameters(lib):
    """Options -> ssx_render_params as Renderer.params builds them (the same three lines, without a context)"""
    for kw, want in ((dict(), 0), (dict(indirect_only=True), _capi.SSX_TRAIT_INDIRECT_ONLY), (dict(explicit_light_sampling=False), _capi.SSX_TRAIT_NO_ELS),
                     (dict(flat_field_correction=False), _capi.SSX_TRAIT_NO_FLAT_FIELD), (dict(libm="glibc-2.35"), _capi.SSX_TRAIT_LIBM)):
        o = Options(scene_name="cornell", **kw)
        p = params(indirect_only=int(o.indirect_only), no_explicit_light_sampling=int(not o.explicit_light_sampling),
                   no_flat_field_correction=int(not o.flat_field_correction), libm=_capi.LIBM_MODES[o.libm])
        assert lib.ssx_render_traits(C.byref(p)) == want
