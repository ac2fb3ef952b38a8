"""csrc/ssx_kernels.hip material_albedo -- spectrum-table lookup, nearest-texel fetch through the sRGB table, the three uplifts
and RGB mode -- through the debug op SSX_DBG_ALBEDO, against the oracle's orc_quad_albedo (src/material.cpp:45-143,
src/util/color.cpp:167-232), bit for bit, on the items of tests/albedo_cases.py: texel boundaries and st outside [0, 1], every
entry of the sRGB table, every tie and the black texel of the Jakob-Hanika fetch, inside and fan cells of Meng's grid, hero
wavelengths on table nodes and table indices clamped on both sides.  tests/test_albedo_units_cpu.py proves on the oracle alone
that the items reach those branches.  Run with -m gpu on MI355X."""
import numpy as np
import pytest

import albedo_cases as ac
from unit_cases import f2u, same_or_both_nan
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu


def renderer_of(v, orc):
    if isinstance(v.scene, str):
        kw = dict(texture=v.texture, render_mode="rgb") if v.uplift == "rgb" else dict(observer=v.observer)
        return Renderer(Options(scene_name=v.scene, res=(8, 8), spp=1, **kw))
    r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, observer=v.observer))
    r.upload_scene_desc(v.desc(orc))
    return r


@pytest.mark.parametrize("name", list(ac.VARIANTS))
def test_albedo_equals_the_oracle_bit_for_bit(name):
    v = ac.variant(name)
    orc = v.oracle()
    r = renderer_of(v, orc)
    it = v.items
    n_quads = r.scene.desc.contents.n_quads if isinstance(v.scene, str) else len(v.scene.quads)
    assert 0 <= it.quad.min() and it.quad.max() < n_quads                  # the op reads the quad table at this index
    got = r.debug_eval(_capi.SSX_DBG_ALBEDO, it.words(), 4).view(np.float32)
    ref = orc.albedo(it.quad, it.st, it.lam)
    if v.uplift == "jh":
        assert np.isnan(ref).any()                                         # the black texels: NaN on both sides, of any payload
        ok = same_or_both_nan(got, ref)
    else:
        ok = np.array_equal(f2u(got), f2u(ref))
    bad = np.argwhere((f2u(got) != f2u(ref)) & ~(np.isnan(got) & np.isnan(ref)))
    assert ok, (len(bad), [(it.group[k], int(it.quad[k]), it.st[k].tolist(), float(it.lam[k]), got[k].tolist(), ref[k].tolist()) for k in bad[:3, 0]])
