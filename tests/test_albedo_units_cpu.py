"""What the items of tests/albedo_cases.py reach, proved on the oracle alone (no GPU): tests/test_albedo_units_gpu.py compares
csrc/ssx_kernels.hip material_albedo with orc_quad_albedo on exactly these items, and would pass on cases that miss a branch.
Here: the new entry point equals the composition of the oracle's already exported pieces on every item, and the items select
every texel, every entry of the sRGB table, every tie of the Jakob-Hanika maximum, the branches of Meng's cell lookup and every
clamped table index."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import albedo_cases as ac
import ref_lib
from unit_cases import f2u

F = np.float32


@pytest.fixture(scope="module", params=list(ac.VARIANTS))
def case(request):
    v = ac.variant(request.param)
    orc = v.oracle()
    return v, orc, orc.albedo(v.items.quad, v.items.st, v.items.lam)


def case_of(name):
    v = ac.variant(name)
    orc = v.oracle()
    return v, orc, orc.albedo(v.items.quad, v.items.st, v.items.lam)


def srgb_table(lib):
    """orc_srgb_to_lrgb of px * (1 / 255) for the 256 bytes (material.cpp:52-56)"""
    lut = np.zeros(256, dtype=F)
    a, o = (C.c_float * 3)(), (C.c_float * 3)()
    for b in range(256):
        a[0] = a[1] = a[2] = float(F(b) * (F(1) / F(255)))
        lib.orc_srgb_to_lrgb(a, o)
        lut[b] = o[0]
    return lut


def texels(v, group):
    """(rows of the group, the byte triple each selects by the clamp rule restated in numpy, texel column, texel row)"""
    k = v.items.of(group)
    tex = v.textures[group]
    i, j = ac.texel_index(tex.shape[1], tex.shape[0], v.items.st[k])
    return k, tex[j, i], i, j


def test_the_entry_point_is_the_composition_of_the_exported_pieces(case):
    """constant albedo: orc_spectrum_hero of the material's table (RGB mode: the material's triple); textured: the texel the
    test picks itself, through orc_srgb_to_lrgb and orc_lrgb_to_specrefl (RGB mode: the linear triple and 0)"""
    v, orc, got = case
    lib, it = orc.lib, v.items
    want = np.zeros_like(got)
    o4 = (C.c_float * 4)()
    view = np.frombuffer(o4, dtype=F)
    for group, (data, low, high) in v.spectra.items():
        sp = ac.OrcSpectrum.make(data, low, high)
        for k in it.of(group):
            lib.orc_spectrum_hero(C.byref(sp), float(it.lam[k]), C.c_float(v.lambda_step), o4)
            want[k] = view
    if v.uplift == "rgb":
        six = (C.c_float * 6)()
        for k in it.of("box"):
            assert lib.orc_scene_material_rgb(orc.scene, lib.orc_scene_quad_material(orc.scene, int(it.quad[k])), six) == 0   # constant albedo
            want[k] = [six[3], six[4], six[5], 0.0]
    lut = srgb_table(lib)
    l3 = (C.c_float * 3)()
    for group in v.textures:
        k, px, _, _ = texels(v, group)
        for row, p in zip(k, px):
            l3[0], l3[1], l3[2] = (float(lut[b]) for b in p)
            if v.uplift == "rgb":
                want[row] = [l3[0], l3[1], l3[2], 0.0]
            else:
                lib.orc_lrgb_to_specrefl(orc.color, l3, float(it.lam[row]), o4)
                want[row] = view
    assert set(it.group) <= set(v.spectra) | set(v.textures) | {"box"}                                    # every item was composed
    same = (f2u(got) == f2u(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (v.name, it.group[np.argwhere(~same)[0][0]], np.argwhere(~same)[:5])


@pytest.mark.parametrize("name", list(ac.SMALL))
def test_small_textures_every_texel_and_the_clamp(name):
    """every texel of every small texture is selected, and the oracle returns that texel's value (the value of the item at its
    centre, at the same lambda_0); st outside [0, 1] selects an edge texel"""
    v, orc, got = case_of("ours-1931")
    w, h = ac.SMALL[name]
    k, px, i, j = texels(v, name)
    assert {(a, b) for a, b in zip(i.tolist(), j.tolist())} == {(a, b) for a in range(w) for b in range(h)}
    st = v.items.st[k]
    out_x, out_y = (st[:, 0] < 0) | (st[:, 0] > 1), (st[:, 1] < 0) | (st[:, 1] > 1)
    assert out_x.sum() > 100 and out_y.sum() > 100
    assert np.isin(i[out_x], (0, w - 1)).all() and np.isin(j[out_y], (0, h - 1)).all()
    assert ((i[st[:, 0] < 0] == 0).all() and (i[st[:, 0] > 1] == w - 1).all()
            and (j[st[:, 1] < 0] == h - 1).all() and (j[st[:, 1] > 1] == 0).all())      # st.y = 1 is the image's first row (material.cpp:70-72)
    # the centre items: every lambda_0 at every texel
    cen = ac.centres(w, h)
    at_centre = {}
    for row, (s, t), lam in zip(k, st.tolist(), v.items.lam[k].tolist()):
        for c, (cs_, ct) in enumerate(cen.tolist()):
            if (s, t) == (cs_, ct):
                at_centre[(c % w, c // w, lam)] = row
    for row, a, b, lam in zip(k, i.tolist(), j.tolist(), v.items.lam[k].tolist()):
        assert np.array_equal(f2u(got[row]), f2u(got[at_centre[(a, b, lam)]])), (name, row)
    # neighbouring texels differ in the oracle's output, so a wrong row or column shows
    centre_rows = np.array([at_centre[(a, b, float(v.items.lam[k][0]))] for b in range(h) for a in range(w)])
    assert len({got[r].tobytes() for r in centre_rows}) == w * h


def test_ramp_reaches_every_entry_of_the_srgb_table_in_every_channel():
    for name in ("ours-1931", "jh-16", "meng"):
        v = ac.variant(name)
        k, px, i, j = texels(v, "ramp")
        assert {(c, x) for c, x in zip(j.tolist(), i.tolist())} == {(c, x) for c in range(3) for x in range(256)}
        assert all(px[n][c] == x and px[n].sum() == x for n, (c, x) in enumerate(zip(j.tolist(), i.tolist())))   # byte x in channel c alone
    lut = srgb_table(ac.ol.load())
    assert len(np.unique(lut)) == 256 and lut[0] == 0 and lut[255] == 1


def test_rgb_mode_lattice_and_edges():
    v, orc, got = case_of("rgb")
    k, px, i, j = texels(v, "lattice")
    assert len({(a, b) for a, b in zip(i.tolist(), j.tolist())}) == 4096
    st = v.items.st[k]
    assert ((st < 0) | (st > 1)).any(axis=1).sum() > 20
    assert np.array_equal(got[k][:, 3], np.zeros(len(k), dtype=F)) and got[k][:, :3].max() == 1
    assert not got[v.items.of("box")].any()                                             # the light box is black (scene.cpp:357-413)


@pytest.mark.parametrize("name", ["jh-16", "jh-7"])
def test_jakob_hanika_black_is_nan_everything_else_in_range_every_tie(name):
    v, orc, got = case_of(name)
    lut = srgb_table(orc.lib)
    ties = Counter()
    textured = 0
    for group in v.textures:
        k, px, _, _ = texels(v, group)
        black = ~px.any(axis=1)
        nan = np.isnan(got[k])
        assert np.array_equal(nan.any(axis=1), black) and np.array_equal(nan.all(axis=1), black), group   # rgb2spec.c:88-91: 0 / 0
        ok = got[k][~black]
        assert np.isfinite(ok).all() and ok.min() >= 0 and ok.max() <= 1
        textured += len(k)
        if group == "lattice":
            assert black.sum() == 2
            ties.update(ac.jh_tie(lut[p]) for p in px)
    assert textured > 10000
    assert all(ties[t] >= 2 for t in ("rg", "gb", "rb", "rgb", "")), ties
    assert not np.isnan(got[np.concatenate([v.items.of(g) for g in v.spectra])]).any()
    # the model's ends: the interval search returns the first interval for the darkest and the last for the brightest maxima
    res, scale, _ = v.uplift_scene().jh_model()
    z = np.array([lut[p].max() for g in ("ramp", "lattice") for p in texels(v, g)[1] if p.any()])
    assert res == v.jh_res and (z < scale[1]).any() and (z > scale[res - 2]).any() and (z == 1).any()


def test_meng_branches():
    """The lattice's 4096 colours in Meng's grid, classified by the numpy restatement of the cell lookup
    (albedo_cases.meng_branch: reads the grid's cells, its xy -> uv transform and the points' uv, not a spectrum):
    3876 inside cells, 68 in the first triangle of a fan, 56 in a middle and 95 in the last one, 1 black.  No colour of the
    lattice leaves the grid (the second early return), falls into a cell without points or into a fan none of whose triangles
    accepts it (`found == false`): those three branches are not reached by these items, and none is made up."""
    v, orc, got = case_of("meng")
    table = ref_lib.meng_table()
    lut = srgb_table(orc.lib)
    k, px, _, _ = texels(v, "lattice")
    branch = [ac.meng_branch(table, lut[p]) for p in px]
    n = len(branch)
    kind = Counter(b if isinstance(b, str) else ("first" if b[1] == 0 else "last" if b[1] == b[2] - 1 else "middle") for b in branch)
    assert n == 2 * 4096 and {b: c // 2 for b, c in kind.items()} == {"inside": 3876, "first": 68, "middle": 56, "last": 95, "black": 1}   # (every colour twice)
    assert kind["inside"] >= 0.01 * n and kind["first"] >= 0.01 * n and kind["middle"] + kind["last"] >= 0.01 * n
    assert kind["middle"] > 0 and kind["last"] > 0
    assert any(isinstance(b, tuple) and b[2] > 2 for b in branch)
    # the early returns give exactly zero, and nothing else of the lattice does
    zero = ~got[k].any(axis=1)
    early = np.array([b in ("black", "offgrid", "empty", "notfound") for b in branch])
    assert kind["black"] >= 1 and np.array_equal(zero, early)
    assert np.isfinite(got).all()
    # the ramp: the three primaries at every level, black at level 0
    kr, pxr, _, _ = texels(v, "ramp")
    assert np.array_equal(~got[kr].any(axis=1), ~pxr.any(axis=1))


def clamp_counts(low, high, n, lam0, lambda_step):
    x, i0, c = ac.table_index(low, high, n, ac.hero_wavelengths(lam0, lambda_step))
    return Counter(c.ravel().tolist()), x, i0, c


@pytest.mark.parametrize("name", ["ours-1931", "ours-2006", "jh-16", "meng", "cornell-1931", "cornell-2006"])
def test_table_lookups_reach_every_clamped_index_and_the_nodes(name):
    """every table a constant albedo reads (the short spectra, n = 3 and n = 2; the Cornell box's), and the basis tables a
    textured "ours" albedo reads: the index clamped to [-2, n] takes each of -2, -1, n - 1 and n, and hero wavelengths sit
    exactly on the first and the last node"""
    v, orc, got = case_of(name)
    tables = {g: (low, high, len(data), v.items.of(g)) for g, (data, low, high) in v.spectra.items()}
    if name.startswith("ours"):
        data, low, high, dr = orc.spectrum("basis_r")
        assert (low, high, len(data)) == v.basis_grid() and F(dr) == ac.delta_recip(low, high, len(data))   # orc_spectrum_info
        tables["basis"] = (low, high, len(data), np.concatenate([v.items.of(g) for g in v.textures]))
    assert tables
    for g, (low, high, n, rows) in tables.items():
        count, x, i0, c = clamp_counts(low, high, n, v.items.lam[rows], v.lambda_step)
        assert all(count[i] > 0 for i in (-2, -1, 0, n - 2, n - 1, n)), (g, count)
        assert (i0 < -2).any() and (i0 > n).any()                                        # the clamp itself acts
        on_node = x == i0
        assert (on_node & (c == 0)).any(), g
        assert (on_node & (c == n - 1)).any() or not ac.node_lambda(low, high, n, n - 1)[1], g   # (no float sits on the last node of [390, 830] x 2)
        # outside the table the oracle returns 0: both neighbours are padding
        both_out = (c == -2) | (c == n)
        assert not got[rows][both_out].any()


def test_shipped_basis_tables_share_one_grid():
    """csrc/ssx_pack.h sets the header's basis_one_grid when the three basis tables have one (low, delta_recip, n); material_albedo
    then takes its fast path for "ours" (descriptor by address, interleaved tables).  Both observers' tables come from one CSV
    file each, so they do: the general "ours" path (three separate lookups) is not run by these cases."""
    for name in ("ours-1931", "ours-2006"):
        ac.variant(name).basis_grid()      # asserts one grid
