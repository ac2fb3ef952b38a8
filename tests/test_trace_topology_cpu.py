"""CPU side of tests/test_trace_topology_gpu.py, on the oracle and tests/pass1_ref.py alone (no device): what the candidate rules of pass 1 may
remove, and what the crafted rays of unit_cases.trace_topo_inputs reach.

Soundness: the triangle the oracle accepts -- quad and which of its two -- is a candidate of the restated pass 1, under the generic rule (mixed
signs of the float edge values) and under the plane topology's rule (that, and not wholly behind the origin): neither filter ever removes a hit,
so a trace that finishes exactly the candidates returns the oracle's answer.

Reach: the counts below are conditions on the INPUTS, met by the reference alone; the GPU test re-asserts none of them, it shares the generator.
The minimums are what every scene of crafted.TRACE_TOPO_SCENES meets with room (the smallest count over the scenes is quoted next to each)."""
import numpy as np
import pytest

import crafted
import pass1_ref
import unit_cases as uc

SCENES = [name for name, _ in crafted.TRACE_TOPO_SCENES]
_cache = {}


def case(name):
    """per scene, once per process: rows, families, the oracle's answers, its f64 fallbacks per row and the restated pass 1 -- live rows only"""
    if name not in _cache:
        c, _ = crafted.trace_topo_scene(name)
        quads, sts = [q[0] for q in c.quads], [q[1] for q in c.quads]
        w, fam, live = uc.trace_topo_inputs(quads)
        w, fam = w[live], fam[live]
        orc = c.oracle()
        ref, f64 = uc.oracle_trace_detail(orc, w, quads, sts)
        plain, _ = uc.oracle_trace(orc, w)
        p1 = pass1_ref.candidates(quads, uc.u2f(w[:, :3]), uc.u2f(w[:, 3:6]), w[:, 6].view(np.int32))
        _cache[name] = dict(w=w, fam=fam, ref=ref, plain=plain, f64=f64, p1=p1, nq=len(quads), all_live=live)
    return _cache[name]


@pytest.mark.parametrize("name", SCENES)
def test_the_oracles_hit_is_a_candidate_under_both_rules(name):
    k = case(name)
    ref, p1 = k["ref"], k["p1"]
    assert np.array_equal(ref[:, [0, 2, 3, 4]], k["plain"][:, [0, 2, 3, 4]])      # the detailed walk is the oracle's intersection, with the triangle added
    rows = np.nonzero(ref[:, 0] != 0xFFFFFFFF)[0]
    tri = (2 * ref[rows, 0] + ref[rows, 1]).astype(np.int64)
    assert p1["generic"][rows, tri].all()                                          # the mixed-sign filter never removes the accepted triangle
    assert not p1["culled"][rows, tri].any() and p1["plane"][rows, tri].all()      # nor does the behind-the-origin cull
    # where all three scaled depths of a triangle are NaN the cull's flag is the sign of a NaN: such a triangle must not be the hit either way
    assert not p1["undetermined"][rows, tri].any()
    # and the ignored quad is never hit
    ign = k["w"][rows, 6].view(np.int32)
    assert (ref[rows, 0].astype(np.int64) != ign).all()


@pytest.mark.parametrize("name", SCENES)
def test_the_rays_reach_the_edge_cases(name):
    k = case(name)
    w, fam, ref, p1 = k["w"], k["fam"], k["ref"], k["p1"]
    n = len(w)
    depth = p1["depth"].reshape(n, -1)
    bits = depth.view(np.uint32)
    hit = ref[:, 0] != 0xFFFFFFFF
    got = dict(
        f64=int((k["f64"] > 0).sum()),                       # rays with a triangle whose float edge values hold a zero: the f64 fallback
        cull_decides=int(p1["culled"].any(axis=1).sum()),    # rays with a triangle the mixed-sign filter keeps and the behind flag removes
        depth_pos0=int((bits == 0).any(axis=1).sum()), depth_neg0=int((bits == 0x80000000).any(axis=1).sum()), depth_nan=int(np.isnan(depth).any(axis=1).sum()),
        tie=int(p1["tie"].sum()),
        behind=int(p1["behind_quad"].any(axis=1).sum()),     # family (e): a whole quad behind the origin
        straddle=int(p1["straddle"].any(axis=1).sum()),      # ... and a quad on both sides of the origin's kz plane
        tri1=int((ref[hit, 1] == 1).sum()), hits=int(hit.sum()))
    print(name, n, got, "hit share of family a %.3f" % hit[fam == "a"].mean())
    need = dict(f64=700,            # smallest over the scenes: 971 (warped-plane-a); the Cornell box 4106
                cull_decides=350,   # 528 (warped-plane-b); plane-srgb 3040
                depth_pos0=300, depth_neg0=300,   # 441 / 424 (the warped planes)
                depth_nan=100,      # 134
                tie=300,            # 416
                behind=1500, straddle=2500, tri1=600, hits=1500)   # 2943, 3407, 939, 2202
    for key, least in need.items():
        assert got[key] >= least, (key, got[key], least)
    assert hit[fam == "a"].mean() > 0.5                      # the existing condition of the generic test, on the rows of trace_inputs
    for f in uc.TRACE_FAMILIES:
        assert (fam == f).sum() >= 40 and hit[fam == f].any(), f
    # every axis is dominant, in both directions, among the rays that hit
    assert set(np.unique(p1["kz"][hit])) == {0, 1, 2}
    # has_ray = 0 rows sit between live ones: no wave of the full array is all live, and one wave is all idle
    live = k["all_live"]
    waves = [live[i:i + 64] for i in range(0, len(live), 64)]
    assert all((~wv).any() for wv in waves[:-1]) and any((~wv).all() for wv in waves if len(wv) == 64)
    assert len(live) % 64 != 0


def test_the_extreme_patterns_are_what_they_claim():
    """islands32: 32 quads, 128 distinct corners (both accumulators of pass 1 full, the largest vertex-table offsets); fan: one corner in eight
    quads, every corner slot, and two quads that share two edges with each other; the warped scenes keep their base scene's sharing pattern."""
    def vids(c):
        ids, rows = {}, []
        for pos, _, _ in c.quads:
            rows.append([ids.setdefault(np.asarray(p, dtype=np.float32).tobytes(), len(ids)) for p in pos])
        return np.array(rows)
    isl = vids(crafted.trace_topo_scene("islands32")[0])
    assert isl.shape == (32, 4) and len(np.unique(isl)) == 128
    fan = vids(crafted.trace_topo_scene("fan")[0])
    counts = np.bincount(fan.ravel())
    apex = int(counts.argmax())
    assert counts[apex] == 8 and {int(np.nonzero(r == apex)[0][0]) for r in fan if apex in r} == {0, 1, 2, 3}
    edges = lambda r: {frozenset((int(r[i]), int(r[(i + 1) % 4]))) for i in range(4)}
    assert max(len(edges(fan[i]) & edges(fan[j])) for i in range(len(fan)) for j in range(i)) == 2
    for warped, base in (("warped-cornell-a", "cornell-srgb"), ("warped-cornell-b", "cornell"), ("warped-plane-a", "plane-srgb"), ("warped-plane-b", "plane-srgb")):
        a, b = crafted.trace_topo_scene(warped)[0], crafted.trace_topo_scene(base)[0]
        assert np.array_equal(vids(a), vids(b))
        assert not np.array_equal(np.array([q[0] for q in a.quads]), np.array([q[0] for q in b.quads]))
