"""The topology-specialised bodies of trace() -- the ones every built-in scene's renders run for bounce and shadow rays, and the one compiled at
upload for a scene's own pattern -- held to the oracle ray by ray, through SSX_DBG_TRACE_TOPO.  Bit for bit, no tolerances.

Per scene of crafted.TRACE_TOPO_SCENES, on the rows of unit_cases.trace_topo_inputs (what they reach is proved without a device in
tests/test_trace_topology_cpu.py): the op equals the oracle -- same quad or both none, and for hits the same triangle, distance and st words --;
it equals SSX_DBG_TRACE (the generic body) from the same context, row for row, triangle word included; rows with has_ray = 0 come back empty.
Run with -m gpu on MI355X."""
import numpy as np
import pytest

import crafted
import unit_cases as uc
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu

PASS1 = {1: "cornell topology", 2: "plane topology", 3: "scene topology"}
_cases, _contexts = {}, {}


def rows_and_reference(name):
    if name not in _cases:
        c, opts = crafted.trace_topo_scene(name)
        quads, sts = [q[0] for q in c.quads], [q[1] for q in c.quads]
        w, fam, live = uc.trace_topo_inputs(quads)
        orc = c.oracle()
        ref, _ = uc.oracle_trace_detail(orc, w[live], quads, sts)
        _cases[name] = (c, opts, orc, w, fam, live, ref)
    return _cases[name]


@pytest.fixture(scope="module")
def context():
    """name -> Renderer with the scene uploaded: one per scene and module, so each pattern of topology 3 compiles once"""
    def get(name):
        if name not in _contexts:
            c, opts, orc = rows_and_reference(name)[:3]
            r = Renderer(Options(**opts))
            r.upload_scene_desc(c.desc(orc))
            _contexts[name] = r
        return _contexts[name]
    yield get
    for r in _contexts.values():
        r.close()
    _contexts.clear()


@pytest.mark.parametrize("name,topology", crafted.TRACE_TOPO_SCENES)
def test_topology_trace_equals_the_oracle_and_the_generic_trace(context, name, topology):
    c, opts, orc, w, fam, live, ref = rows_and_reference(name)
    r = context(name)
    assert r.plan_info()["pass1"].startswith(PASS1[topology]), r.plan_info()
    got = r.debug_eval(_capi.SSX_DBG_TRACE_TOPO, w, 5)
    generic = r.debug_eval(_capi.SSX_DBG_TRACE, w, 5)              # (reads the first seven words of a row: every row traced)
    g = got[live]
    hit = ref[:, 0] != 0xFFFFFFFF
    bad = np.nonzero(g[:, 0] != ref[:, 0])[0]
    assert bad.size == 0, (name, "quad", len(bad), [(fam[live][i], uc.u2f(w[live][i, :6]).tolist(), int(w[live][i, 6]), g[i].tolist(), ref[i].tolist()) for i in bad[:3]])
    bad = np.nonzero((g[hit] != ref[hit]).any(axis=1))[0]            # triangle, distance and st words of the hits
    assert bad.size == 0, (name, "hit words", len(bad), [(fam[live][hit][i], g[hit][i].tolist(), ref[hit][i].tolist()) for i in bad[:3]])
    assert np.array_equal(g[~hit][:, 1:], np.broadcast_to(np.array(uc.EMPTY_TRACE[1:], dtype=np.uint32), g[~hit][:, 1:].shape))
    # the generic body on the same upload: every word of every live row
    bad = np.nonzero((g != generic[live]).any(axis=1))[0]
    assert bad.size == 0, (name, "generic", len(bad), [(fam[live][i], g[i].tolist(), generic[live][i].tolist()) for i in bad[:3]])
    # a lane without a ray takes part in pass 1 and returns nothing
    assert (~live).sum() > 1000
    assert (got[~live] == np.array(uc.EMPTY_TRACE, dtype=np.uint32)).all()


def test_the_op_refuses_a_context_on_the_generic_kernel():
    """topology 0: the op would be SSX_DBG_TRACE; and a row shorter than eight words is refused"""
    c = crafted.shared_edge_scene()
    orc = c.oracle()
    r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, observer=c.observer))
    try:
        r.upload_scene_desc(c.desc(orc))
        assert r.plan_info()["pass1"] == "generic"
        w = np.zeros((4, 8), dtype=np.uint32)
        with pytest.raises(RuntimeError, match="SSX_DBG_TRACE_TOPO"):
            r.debug_eval(_capi.SSX_DBG_TRACE_TOPO, w, 5)
    finally:
        r.close()
    r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1))
    try:
        with pytest.raises(RuntimeError, match="has_ray"):
            r.debug_eval(_capi.SSX_DBG_TRACE_TOPO, np.zeros((4, 7), dtype=np.uint32), 5)
    finally:
        r.close()
