"""One iteration of the path loop -- trace, path_step, the end of a path, the flush of the parked shadow rays: ssx_debug_step -- against one level of the
oracle's L() (orc_debug_level), bit for bit under the three rules of tests/step_cases.py, read back through the level logs and the tail word as the fold
reads them.  tests/test_step_cpu.py ties orc_debug_level to orc_render_sample and counts what the rows reach.  Run with -m gpu on MI355X."""
import ctypes as C

import numpy as np
import pytest

import step_cases as sc
from simple_spectral_amd import _capi as K
from test_fold_gpu import queue_entries

pytestmark = pytest.mark.gpu

_made = {}


def renderer(name):
    if name not in _made:
        ctx = sc.context(name)
        r = ctx.renderer()
        assert r._lib.ssx_kernel_variant(r._ctx) == ctx.topology, (name, r.plan_info())
        _made[name] = r
    return _made[name]


def params_of(flags, ctx):
    over = dict(indirect_only=flags & 1, no_explicit_light_sampling=(flags >> 1) & 1)
    return over


def run_case(name, case, narrow, rows=None):
    ctx, r = sc.context(name), renderer(name)
    with queue_entries(narrow):
        return r.debug_step(case.rows if rows is None else rows, case.n_rounds, **params_of(case.flags, ctx))


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("name", list(sc.CONTEXTS))
def test_step_equals_the_oracle(name, narrow):
    ctx = sc.context(name)
    with queue_entries(narrow):
        is_narrow = "_nq" in renderer(name).plan_info()["kernel"]
    bad = []
    for case in ctx.cases():
        lev, after = case.reference(ctx)
        exp, mask = sc.expected(case.rows, lev, after, case.flags, ctx.mat, is_narrow)
        got = run_case(name, case, narrow)
        diff = sc.compare(got, exp, mask)
        if len(diff):
            i, w = (int(v) for v in diff[0])
            bad.append((case.name, len(diff), "row %d word %d: 0x%08X against 0x%08X" % (i, w, got[i, w], exp[i, w]), case.rows[i].tolist()))
    assert not bad, "%d of %d cases differ; the first: %r" % (len(bad), len(ctx.cases()), bad[0])


def test_queue_entries_switch_takes_effect():
    """the narrow runs above are narrow: the render of the same context picks the _nq twin under the switch, and the two answers differ where they must --
    an occluded term stays in the log of narrow entries and is zeros in the finished term of wide ones"""
    name = "cornell-srgb"
    r, ctx = renderer(name), sc.context(name)
    with queue_entries(False):
        assert not r.plan_info()["kernel"].endswith("_nq")
    with queue_entries(True):
        assert "_nq" in r.plan_info()["kernel"]
    case = ctx.cases()[0]
    wide, nq = run_case(name, case, False), run_case(name, case, True)
    occluded = (wide[:, K.SSX_STEP_O_FLAGS] & (K.SSX_STEP_PARKED | K.SSX_STEP_VISIBLE)) == K.SSX_STEP_PARKED
    assert occluded.any()
    t = slice(K.SSX_STEP_O_NEE, K.SSX_STEP_O_NEE + 4)
    assert (wide[occluded, t] == 0).all() and (nq[occluded, t] != 0).any(axis=1).all()
    rest = np.ones(sc.OUT, dtype=bool); rest[t] = False; rest[K.SSX_STEP_O_SLOT:] = False
    assert (wide[:, rest] == nq[:, rest]).all()


@pytest.mark.parametrize("name", ["cornell-srgb", "plane-srgb", "degenerate"])
def test_rows_may_sit_in_any_lane_and_round(name):
    """permuting a call's rows among lanes, rounds and tiles changes no row's answer (its slot aside)"""
    ctx = sc.context(name)
    g = np.random.default_rng(5)
    for case in [c for c in ctx.cases() if c.name.startswith(("replay/flags0", "queue/boundaries"))]:
        perm = g.permutation(len(case.rows))
        a, b = run_case(name, case, False), run_case(name, case, False, rows=case.rows[perm])
        assert (a[perm, :K.SSX_STEP_O_SLOT] == b[:, :K.SSX_STEP_O_SLOT]).all(), case.name


def test_arguments_are_checked():
    name = "cornell-srgb"
    r, ctx = renderer(name), sc.context(name)
    rows = ctx.cases()[0].rows[:128].copy()
    with pytest.raises(RuntimeError, match="multiple of 64"):
        r.debug_step(rows[:96], 1)
    with pytest.raises(RuntimeError, match=r"64 \* n_rounds"):
        r.debug_step(rows[:64], 2)
    with pytest.raises(RuntimeError, match="n_rounds must be"):
        r.debug_step(np.tile(rows[:64], (9, 1)), 9)
    for word, value, what in ((K.SSX_STEP_R_DEPTH, 10, "depth"), (K.SSX_STEP_R_IGNORE, ctx.mat.n_quads, "ignore"), (K.SSX_STEP_R_IGNORE, 0xFFFFFFFE, "ignore"),
                              (K.SSX_STEP_R_PREV_SLOT, sc.NO_SLOT + 1, "prev_slot"), (K.SSX_STEP_R_LAMBDA0, int(sc.f2u([np.nan])[0]), "lambda_0"),
                              (K.SSX_STEP_R_LAMBDA0, int(sc.f2u([ctx.lambda_min + 2 * ctx.lambda_step])[0]), "lambda_0")):
        x = rows.copy(); x[77, word] = value
        with pytest.raises(RuntimeError, match="row 77: " + what):
            r.debug_step(x, 2)
    # level logs the kernels' 32-bit offsets could not address, and more tiles than a call takes: refused from the sizes alone, before a row is read
    dummy = np.zeros(sc.ROW, dtype=np.uint32)
    assert r._lib.ssx_debug_step(r._ctx, C.byref(r.params()), 65537 * 64, 1, dummy.ctypes.data, dummy.ctypes.data) == -2   # SSX_ERR_ARG
    assert b"65536 tiles" in r._lib.ssx_last_error(r._ctx)
    assert r._lib.ssx_debug_step(r._ctx, C.byref(r.params()), 65536 * 64 * 8, 8, dummy.ctypes.data, dummy.ctypes.data) == -2
    assert b"4 GiB" in r._lib.ssx_last_error(r._ctx)
