"""The path kernel's fold -- resolve_records in unit_fold's loop, run by ssx_debug_fold on levels the test supplies -- against the oracle's
orc_fold_levels, bit for bit (NaN against NaN counts as equal): per-sample hero flux and {X, Y, Z, alpha}, and the pixels' binary64 sums.
tests/fold_cases.py makes the rows; tests/test_fold_cpu.py ties orc_fold_levels to the oracle's recursion and counts what the rows reach.
Run with -m gpu on MI355X."""
import os

import numpy as np
import pytest

import fold_cases as fc
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer

pytestmark = pytest.mark.gpu

ORDER_SEEDS = (0, 0x9E3779B9, 0x51ED27AF)   # bit 7 (the order of a sample's own levels) clear, set, set


def same(got, ref):
    """uint32 arrays of float32 bits: equal, or NaN on both sides"""
    g, r = np.asarray(got), np.asarray(ref)
    return (g == r) | (np.isnan(g.view(np.float32)) & np.isnan(r.view(np.float32)))


def same64(got, ref):
    g, r = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    return (g.view(np.uint64) == r.view(np.uint64)) | (np.isnan(g) & np.isnan(r))


CONTEXTS = {   # what decides the kernel twin and the tables: observer, RGB mode, libm, the _flux twin (spectral output on)
    "1931": dict(observer=1931), "2006": dict(observer=2006), "rgb": dict(observer=1931, render_mode="rgb"),
    "1931-glibc": dict(observer=1931, libm="glibc-2.35"), "2006-glibc": dict(observer=2006, libm="glibc-2.35"),
    "1931-flux": dict(observer=1931, flux=True), "2006-flux": dict(observer=2006, flux=True),
}
_made = {}


def context(key):
    """(Renderer, Oracle, synthetic cases for its lambda range + the replayed tiles recorded under its observer), made once"""
    if key not in _made:
        kw = dict(CONTEXTS[key])
        flux = kw.pop("flux", False)
        scene = "cornell-srgb" if kw["observer"] == 1931 else "cornell"
        r = Renderer(Options(scene_name=scene, res=(8, 8), spp=1, texture="test-img.png", **kw))
        if flux:
            r.set_spectral_bins(16)
        rgb = kw.get("render_mode") == "rgb"
        orc = ol.Oracle(scene, observer=kw["observer"], texture="test-img.png", rgb=rgb)
        d = r.scene.desc.contents
        cases = fc.synthetic_cases(d.lambda_min, d.lambda_step)
        for rk, (_, observer, _, _) in fc.REPLAY_CONFIGS.items():
            if observer == kw["observer"] and not rgb:
                cases += fc.replay_cases(rk)[2]
        _made[key] = (r, orc, cases, flux, rgb)
    return _made[key]


_refs = {}


def reference(key, flat_field):
    """orc_fold_levels and the restated sums for every case of the context, computed once and left alone"""
    if (key, flat_field) not in _refs:
        r, orc, cases, flux, rgb = context(key)
        out = []
        for c in cases:
            fl, xyza = fc.oracle_fold(orc, c.rows, flat_field=flat_field)
            out.append((fl, xyza, fc.pixel_sums(xyza, c.spp, rgb)))
        _refs[(key, flat_field)] = out
    return _refs[(key, flat_field)]


class queue_entries:
    """narrow queue entries through the switch the A/B runs and tests/test_gpu_variants.py use; without it a context gets what a render of it picks: wide for
    the CIE 1931 tables, narrow for the larger CIE 2006 ones (tests/test_gpu_parity.py: test_shadow_queue_layouts_...)"""

    def __init__(self, narrow):
        self.env = {"SSX_DEBUG_ENV": "1", "SSX_NARROW_QUEUE": "1"} if narrow else {}

    def __enter__(self):
        self.was = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check(key, narrow, flat_field, parked, seeds=(ORDER_SEEDS[0],)):
    r, orc, cases, flux, rgb = context(key)
    refs = reference(key, flat_field)
    bad = []
    with queue_entries(narrow):
        for c, (ref_flux, ref_xyza, ref_sums) in zip(cases, refs):
            for seed in seeds:
                fl, xyza, sums = r.debug_fold(c.rows, c.spp, order_seed=seed, parked=parked, flux=flux, no_flat_field_correction=int(not flat_field))
                ok = same(xyza, ref_xyza).all(axis=1)
                if flux:
                    ok &= same(fl, ref_flux).all(axis=1)
                if not ok.all() or not same64(sums, ref_sums).all():
                    s = int(np.argmin(ok)) if not ok.all() else -1
                    bad.append((c.name, seed, s, None if s < 0 else (xyza[s], ref_xyza[s]), None if s < 0 or not flux else (fl[s], ref_flux[s])))
    assert not bad, "%d of %d runs differ; the first: %r" % (len(bad), len(cases) * len(seeds), bad[0])


@pytest.mark.parametrize("parked", [0, 1])
@pytest.mark.parametrize("flat_field", [True, False])
@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("key", list(CONTEXTS))
def test_fold_equals_the_oracle(key, narrow, flat_field, parked):
    check(key, narrow, flat_field, parked)


@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("key", ["1931", "rgb", "2006-flux"])
def test_slot_order_is_immaterial(key, narrow):
    """three order seeds: the same bits, and the oracle's (csrc/ssx_kernels.hip LogRef: "the order of the slots within one wave iteration is immaterial")"""
    check(key, narrow, True, 0, seeds=ORDER_SEEDS)
    check(key, narrow, False, 1, seeds=ORDER_SEEDS[1:])


def test_queue_entries_switch_takes_effect():
    """the narrow runs above are narrow: the render of the same context picks the _nq twin under the switch"""
    r = context("1931")[0]
    with queue_entries(False):
        assert not r.plan_info()["kernel"].endswith("_nq")
    with queue_entries(True):
        assert "_nq" in r.plan_info()["kernel"]


def test_arguments_are_checked():
    r, _, cases, _, _ = context("1931")
    c = cases[0]
    with pytest.raises(RuntimeError, match="multiple of 64"):
        r.debug_fold(c.rows[:c.spp * 32], c.spp)
    with pytest.raises(RuntimeError, match="spp must be"):
        r.debug_fold(np.zeros((64 * 9, fc.ROW), dtype=np.uint32), 9)
    with pytest.raises(RuntimeError, match="out_flux needs spectral output"):
        r.debug_fold(c.rows, c.spp, flux=True)
    # level logs the kernels' 32-bit offsets could not address: refused from the sizes alone, before a row is read
    import ctypes as C
    dummy = np.zeros(fc.ROW, dtype=np.uint32)
    assert r._lib.ssx_debug_fold(r._ctx, C.byref(r.params()), 1 << 20, 8, dummy.ctypes.data, 0, 0, None, None, None) == -2   # SSX_ERR_ARG
    assert b"4 GiB" in r._lib.ssx_last_error(r._ctx)
