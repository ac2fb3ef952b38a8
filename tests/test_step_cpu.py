"""The oracle's side of tests/test_step_gpu.py: orc_debug_level -- one level of L() for a given ray, radiance_L's own body stopped where it would call itself --
is tied to orc_render_sample, and the rows of tests/step_cases.py are counted for what they reach.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fold_cases as fc
import step_cases as sc
from simple_spectral_amd import _capi as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CONTEXTS = list(sc.CONTEXTS)   # cornell-glibc included: its rows come from the shim oracle (tests/glibc_oracle.py), which the build makes and no GPU is needed for


@pytest.mark.parametrize("flags", sc.FLAG_SETS)
@pytest.mark.parametrize("name", CPU_CONTEXTS)
def test_chained_levels_reproduce_render_sample(name, flags):
    """chaining orc_debug_level from the camera ray gives orc_render_sample's level record, its final stream and -- through orc_fold_levels -- its xyza"""
    ctx = sc.context(name)
    ctx.cases()
    rows, records = ctx.replays[flags]
    lib = sc.bind(ctx.oracle.lib)
    assert len(records) == 64 * sc.SPP * (sc.REPLAY_TILES[flags] if ctx.mat.n_quads <= 40 else max(1, sc.REPLAY_TILES[flags] // 2))
    deepest = 0
    for first, rec, final, xyza, chain, chained_final in records:
        n = int(rec[fc.N])
        assert len(chain) == n + 1, (first, n, len(chain))
        again = rec.copy()
        for d, lev in enumerate(chain):
            want = rec[fc.LEVEL0 + d * fc.LEVEL_WORDS:fc.LEVEL0 + (d + 1) * fc.LEVEL_WORDS]
            got = lev[sc.L_LEVEL:sc.L_LEVEL + fc.LEVEL_WORDS]
            assert fc.LEVEL_WORDS == sc.LEVEL_WORDS - sc.L_LEVEL
            assert (got == want).all() or (np.isnan(sc.u2f(got)) == np.isnan(sc.u2f(want))).all() and ((got == want) | np.isnan(sc.u2f(got))).all(), (first, d)
            again[fc.LEVEL0 + d * fc.LEVEL_WORDS:fc.LEVEL0 + (d + 1) * fc.LEVEL_WORDS] = got
        assert chained_final == final, first
        assert int(rec[fc.HIT]) == int(chain[0][sc.L_HIT_PRIM].view(np.int32) >= 0)
        out = np.zeros(4, dtype=np.uint32)
        lib.orc_fold_levels(ctx.oracle.color, ctx.oracle.scene, again.ctypes.data, 1, flags, None, out.ctypes.data)
        assert ((out == xyza) | (np.isnan(sc.u2f(out)) & np.isnan(sc.u2f(xyza)))).all(), first
        deepest = max(deepest, n)
    assert deepest >= 1


def test_debug_level_leaves_render_sample_alone():
    """the stop flag is off in a render: the same sample before and after a call of orc_debug_level, results, draws and counters"""
    ctx = sc.context("cornell-srgb")
    import oracle_lib as ol
    def sample():
        rng, out, st = ol.Rng(), (C.c_float * 4)(), ol.Stats()
        ctx.oracle.lib.orc_seed_sample(7, 5, 1, C.byref(rng))
        ctx.oracle.lib.orc_render_sample(ctx.oracle.color, ctx.oracle.scene, C.byref(rng), 5, 0, 16, 8, 0, out, C.byref(st))
        return list(out), rng.state, st.as_dict()
    before = sample()
    sc.oracle_levels(ctx.oracle, ctx.cases()[0].rows[:8], 0)
    assert sample() == before


# what every context must reach, and what only some can: a family that reaches nothing is a failing test
EVERYWHERE = ("hit", "miss_depth0", "miss_deeper", "continued", "recurse_but_stopped", "depth9_no_draws", "emission", "emission_deeper",
              "emission_suppressed_indirect_only", "parked", "visible", "faces_away", "light_hit", "light_front", "light_back", "hit_tri1", "same_triangle_visible")
ONLY = {
    "occluded": ("cornell-srgb", "cornell-2006", "cornell-black", "cornell-rgb", "cornell-glibc", "degenerate", "prims128-2006"),
    "other_triangle_visible": ("folded-light",),   # the shadow ray ends on the sampled quad's OTHER triangle: visible, the rule compares quads
    "mirror_front": ("cornell-black", "degenerate"),
    "mirror_back": ("cornell-black", "degenerate"),
    "pdf_inf": ("cornell-black", "degenerate"),
    "zero_term_not_parked": ("cornell-black", "plane-srgb", "degenerate"),   # black surfaces, mirrors, the zero-area light triangle
    "emission_flag_not_emissive": tuple(n for n in sc.CONTEXTS),              # rule 3: L() adds an all-zero table, the kernel has no term
    "mirror": ("cornell-black", "degenerate"),
    "textured": ("cornell-srgb", "cornell-black", "cornell-rgb", "cornell-glibc", "plane-srgb", "plane-inf"),
    "black": ("cornell-black", "plane-srgb"),
    "parked_nan": ("plane-inf",),
    "light_pdf_inf": ("degenerate",),
    "occluded_by_other_light": ("prims128-2006",),
    "quad127_hit": ("prims128-2006",),
    "quad127_light": ("prims128-2006",),
    "emissive_and_continues": ("cornell-black",),
}


@pytest.mark.parametrize("name", CPU_CONTEXTS)
def test_rows_reach_every_branch_that_applies(name):
    ctx = sc.context(name)
    c = sc.reach(ctx)
    print(name, {k: v for k, v in c.items() if not isinstance(v, set)})
    for k in EVERYWHERE:
        assert c[k] > 0, (name, k)
    for k, where in ONLY.items():
        if name in where:
            assert c[k] > 0, (name, k)
    assert c["depths"] == set(range(10))
    assert {0, sc.NO_SLOT - 1, sc.NO_SLOT} <= c["prev_slots"]
    assert 500 <= c["rows"] <= 8000          # a few thousand rows per context (paths without explicit light sampling run ten levels)
    assert ctx.mat.n_quads <= 128


def test_queue_sequences_do_what_they_claim():
    ev = {n: sc.queue_events(s) for n, s in sc.QUEUE_SEQUENCES.items()}
    assert set(sc.QUEUE_SEQUENCES["each-count"]) == {0, 1, 31, 33, 64}
    assert {"63->64", "remainder", "127", "drain-alone"} <= ev["boundaries"]
    assert "drain-alone" in ev["drain-only"] and "partial" in ev["drain-only"]
    assert "remainder" in ev["each-count"]


@pytest.mark.parametrize("name", CPU_CONTEXTS)
def test_queue_cases_park_the_counts_they_claim(name):
    """from the oracle's park decisions alone (rule 2): round k of a queue case parks QUEUE_SEQUENCES[...][k] lanes, and not a prefix of the wave"""
    ctx = sc.context(name)
    seen = 0
    for case in ctx.cases():
        if not case.name.startswith("queue/"):
            continue
        seq = sc.QUEUE_SEQUENCES[case.name.split("/")[1]]
        lev, _ = case.reference(ctx)
        parked = sc.decisions(case.rows, lev, case.flags)[2].reshape(len(seq), 64)
        assert tuple(parked.sum(axis=1).tolist()) == seq, case.name
        for k, n in enumerate(seq):
            if 0 < n < 64:
                assert not parked[k, :n].all(), (case.name, k)
        seen += 1
    assert seen == len(sc.QUEUE_SEQUENCES) + 1   # every sequence with explicit light sampling, "boundaries" once more in an indirect-only render


def test_mirrors_match_the_header():
    text = open(os.path.join(ROOT, "include", "ssx.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (SSX_STEP_\w+) (0x[0-9A-Fa-f]+|\d+)u", text)}
    assert len(defs) == 34
    for name, v in defs.items():
        assert getattr(K, name) == v, name
    otext = open(os.path.join(ROOT, "oracle", "oracle.h")).read()
    assert "orc_level_out" in otext and sc.LEVEL_WORDS == 23 + fc.LEVEL_WORDS
    assert sc.NO_SLOT == 0x1FFF and sc.MAX_DEPTH == 10
