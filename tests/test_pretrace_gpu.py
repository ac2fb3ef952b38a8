"""The camera-ray pre-trace (SsxKernelArgs::pre_hits) off the Cornell box, in three layers, each against a plain reference:

  1. ssx_tile_mask_kernel, read back through ssx_debug_tile_mask: bit for bit the mask of its documented rule restated in numpy binary64
     (tests/tile_mask_ref.py), and -- independent of the rule -- never without a primitive that a ray of the tile hits in the oracle;
  2. the masked pass 1 of trace<0> as a unit (SSX_DBG_TRACE_MASKED) against the oracle's Scene::intersect, under full masks, masks that keep
     a prefix of the primitive list plus random others, and masks that leave out exactly what the oracle finds;
  3. whole samples and images of crafted and random scenes with the pre-trace forced on, and forced off, in fresh processes
     (tests/pretrace_worker.py), against the oracle.

Scenes with more than 16 and more than 32 primitives, ragged last groups, triangle primitives, the permuted table in HBM, cameras with
primitives behind them, ragged images shared out with a stride: what the built-in scenes, which are the only ones whose calibration turns the
pre-trace on, never present.  tests/test_pretrace_cpu.py holds the self-checks of the references.  Run with -m gpu on MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pretrace_cases as pc
import tile_mask_ref as tm
import unit_cases as uc
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

_renderers = {}


def renderer_of(name):
    """one context per scene, shared by the tests of layers 1 and 2 (read-only use: masks and unit ops)"""
    build = pc.MASK_CASES[name][0]
    if build not in _renderers:
        c, orc, _, _ = pc.mask_case(name)
        r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, observer=c.observer))
        r.upload_scene_desc(c.desc(orc))
        _renderers[build] = r
    return _renderers[build]


# ---- 1. the tile mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.MASK_CASES))
def test_tile_mask_equals_its_rule_and_keeps_what_the_tile_rays_hit(name):
    c, orc, (W, H), lay = pc.mask_case(name)
    r = renderer_of(name)
    got = r.debug_tile_mask(width=W, height=H, **lay)
    ref, tiles, _ = pc.reference(name)
    n = ref.keep.shape[1]
    assert got.shape == ref.words.shape == (len(tiles), 4)
    keep = tm.unpack(got, n)
    assert np.array_equal(tm.pack(keep), got), "bits set at or above the number of primitives"
    # (a) the rule, bit for bit; exempt: primitives with a comparison within rounding of the threshold in that tile (none in these scenes: the CPU test)
    exempt = ref.banded.any(axis=(2, 3))
    differ = (keep != ref.keep) & ~exempt
    print("%s: %d slots x %d primitives, kept per tile %.2f (device) %.2f (rule), exempt %d" % (name, len(tiles), n, keep.sum(axis=1).mean(),
                                                                                            ref.kept_per_tile().mean(), int(exempt.sum())))
    assert exempt.mean() <= 0.001
    assert not differ.any(), [(int(s), tiles[s], int(q)) for s, q in np.argwhere(differ)[:8]]
    # (b) ground truth, no exemptions: what the oracle's intersection finds along the tile's rays is in the mask
    must = pc.ground_truth(name)
    assert not (must & ~keep).any(), [(int(s), tiles[s], int(q)) for s, q in np.argwhere(must & ~keep)[:8]]
    # (c) it culls
    if name == "prims70":
        assert keep.sum(axis=1).mean() < n


def test_tile_mask_call_leaves_the_context_alone_and_checks_its_arguments():
    """nothing of it runs during a render, and it touches neither the sums nor the sample arrays: a render can be continued across it"""
    c, orc, (W, H), lay = pc.mask_case("prims33")
    r = Renderer(Options(scene_name="cornell", res=(W, H), spp=4, seed=3, observer=c.observer))
    r.upload_scene_desc(c.desc(orc))
    r.render_start(); r.render_wait()
    before = r.xyza.copy()
    got = r.debug_tile_mask()
    assert np.array_equal(got, pc.reference("prims33")[0].words)
    r.xyza[:] = 0.0
    r.read_framebuffer()
    assert r.done_spp() == 4 and np.array_equal(r.xyza.view(np.uint32), before.view(np.uint32))
    r.render_continue(4); r.render_wait()
    assert np.array_equal(r.xyza.view(np.uint32), orc.render(W, H, 8, seed=3).view(np.uint32))
    # another layout of the same image: the slots are the strided places of the tile list
    whole = r.debug_tile_mask()
    for first in range(3):
        part = r.debug_tile_mask(tile_first=first, tile_stride=3)
        assert np.array_equal(part, whole[first::3])
    p = r.params(width=0)
    out = np.zeros((1, 4), dtype=np.uint32)
    assert r._lib.ssx_debug_tile_mask(r._ctx, r.params(width=0), out.ctypes.data) == _capi.SSX_ERR_ARG
    assert r._lib.ssx_debug_tile_mask(r._ctx, p, None) == _capi.SSX_ERR_ARG and r._lib.ssx_debug_tile_mask(r._ctx, None, out.ctypes.data) == _capi.SSX_ERR_ARG


# ---- 2. the masked trace -----------------------------------------------------------------------------------------------------------------------
def masked_trace(name, blocks):
    return renderer_of(name).debug_eval(_capi.SSX_DBG_TRACE_MASKED, blocks.rows(), 5)


def assert_equals_oracle(got, exp):
    hit = exp[:, 0] != pc.MISS
    assert np.array_equal(got[:, 0], exp[:, 0]), np.flatnonzero(got[:, 0] != exp[:, 0])[:8]           # same primitive (or both none)
    assert np.array_equal(got[hit][:, 2:5], exp[hit][:, 2:5])                                             # same dist and st, bit for bit


@pytest.mark.parametrize("name", pc.TRACE_SCENES)
def test_masked_trace_with_every_primitive_kept_equals_the_oracle(name):
    b = pc.full_blocks(name)
    got = masked_trace(name, b)
    exp = b.expected()
    assert (exp[:, 0] != pc.MISS).mean() > 0.5
    assert_equals_oracle(got, exp)
    # and the unmasked op on the same rows: the two branches of pass 1 agree word for word
    assert np.array_equal(got, renderer_of(name).debug_eval(_capi.SSX_DBG_TRACE, np.ascontiguousarray(b.rows()[:, :7]), 5))


@pytest.mark.parametrize("name", pc.TRACE_SCENES)
def test_masked_trace_with_a_prefix_and_random_primitives_kept_equals_the_oracle(name):
    b = pc.prefix_blocks(name)
    seen, exist, empty = pc.coverage(b)
    assert seen == exist and empty                    # survivors at q = 15, 16, 17, 31 of every group that has them; a group left empty
    assert_equals_oracle(masked_trace(name, b), b.expected())


@pytest.mark.parametrize("name", pc.TRACE_SCENES)
def test_masked_trace_never_finds_what_the_mask_leaves_out(name):
    b = pc.masked_out_blocks(name)
    got, exp, kept = masked_trace(name, b), b.expected(), b.kept()
    w = b.rows()
    hit = got[:, 0] != pc.MISS
    rows = np.flatnonzero(hit)
    assert kept[rows, got[rows, 0].astype(np.int64)].all()                                              # never a masked-out primitive
    assert (got[rows, 0].astype(np.int64) != w[rows, 6].view(np.int32)).all()                           # nor the ignored one
    d_got = np.where(hit, uc.u2f(got[:, 2]), np.float32(np.inf))
    assert (d_got >= uc.u2f(exp[:, 2])).all()                                                          # no closer than the unmasked closest hit
    # Where a block leaves out one primitive P and the row ignores none, the masked trace IS the oracle's intersection with P ignored
    pick = np.flatnonzero((b.single >= 0) & (w[:, 6].view(np.int32) == -1))
    assert len(pick) > 200
    again = np.ascontiguousarray(w[pick, :7]).copy()
    again[:, 6] = b.single[pick].astype(np.int32).view(np.uint32)
    ref, _ = uc.oracle_trace(pc.mask_case(name)[1], again)
    assert_equals_oracle(got[pick], ref)


# ---- 3. whole samples with the pre-trace forced on and off -----------------------------------------------------------------------------------
MODES = {"1": "pre-traced (generate kernel)", "0": "path loop"}


@pytest.fixture(scope="module")
def sample_workers(tmp_path_factory):
    """the oracle's samples and images, computed once and passed by file; one fresh process per mode, side by side"""
    W, H = pc.SAMPLE_RES
    ref = {}
    for name in pc.SAMPLE_CASES:
        c, flags, seed = pc.sample_case(name)
        orc = c.oracle()
        xyza, state, _ = orc.samples(W, H, pc.SAMPLE_SPP, seed=seed, **flags)
        ref[name + "/xyza"], ref[name + "/state"] = xyza, state
        ref[name + "/image"] = orc.render(W, H, pc.SAMPLE_SPP, seed=seed, **flags)
    path = str(tmp_path_factory.mktemp("pretrace") / "oracle.npz")
    np.savez(path, **ref)
    procs = {}
    for mode in MODES:
        env = dict(os.environ, SSX_DEBUG_ENV="1", SSX_PRE_HITS=mode)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        procs[mode] = subprocess.Popen([sys.executable, os.path.join(HERE, "pretrace_worker.py"), path], cwd=ROOT, env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()


@pytest.mark.parametrize("mode", list(MODES))
def test_samples_and_images_in_the_forced_mode_equal_the_oracle(sample_workers, mode):
    p = sample_workers[mode]
    try:
        out, err = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        pytest.fail("SSX_PRE_HITS=%s: worker timed out" % mode)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, err[-2000:])
    rep = json.loads(lines[-1])
    assert rep["env"].get("SSX_PRE_HITS") == mode and set(rep["scenes"]) == set(pc.SAMPLE_CASES)
    for name, s in rep["scenes"].items():
        assert s["camera_rays"] == MODES[mode], (name, s)            # the forced mode ran, not the calibration's choice
        assert s["states"] and s["samples"] and s["image"], (name, s)
    assert max(s["n_prims"] for s in rep["scenes"].values()) == 128 and sum(s["n_prims"] > 32 for s in rep["scenes"].values()) >= 2
