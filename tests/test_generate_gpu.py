"""Sample generation -- ssx_generate_kernel, the first stage of a render -- read back through ssx_debug_generate and held to the oracle record by record,
word by word: the camera ray and lambda_0 (orc_camera_sample), the PCG32 stream after the sample's draws, and, where camera rays are pre-traced, the first
hit (orc_debug_camera_hit) or the end-of-path form of a ray that leaves the scene.  Both sides divide and take square roots in IEEE binary64 and round once
to float: every comparison is on 32-bit words, with no tolerance.

Cases (tests/generate_cases.py): the two built-in topologies, crafted scenes of 33 / 70 / 128 primitives, triangle primitives, a camera with primitives
behind it, an RGB-mode context, both observers; power-of-two, mixed and ragged image sizes, degenerate ones, and the largest the API admits; k0 > 0 and k
up to 2^32 - 2; seeds up to 2^64 - 1; strided and skewed tile layouts; pre_hits 0 and 1 on every scene.  A failure names the array, the field and the
record.  tests/test_generate_cpu.py holds the self-checks of the reference.  The fused path (plane topology: the path kernel's refill calls
generate_sample itself) runs in fresh processes, fused and unfused, against the oracle's samples.  Run with -m gpu on MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import generate_cases as gc
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

FIELDS = {"ray": ("dir.x", "dir.y", "dir.z", "lambda_0"), "st": ("state lo | lambda_0 bits", "state hi | tail word", "inc lo | state lo", "inc hi | state hi"),
          "hit": ("dist", "st.x", "st.y", "2 * quad + which")}
_renderers = {}


def renderer_of(name):
    """one context per scene, shared by its cases (the op leaves the context alone)"""
    if name not in _renderers:
        _renderers[name] = gc.context(name).renderer()
    return _renderers[name]


def generate(name, case, pre_hits):
    return renderer_of(name).debug_generate(case.k0, case.n_k, pre_hits, width=case.W, height=case.H, seed=case.seed, tile_first=case.first,
                                            tile_stride=case.stride, tile_skew=case.skew)


def assert_words(name, case, pre_hits, array, got, exp, ref):
    """got == exp, or the first record that differs: its array and field, slot / k / lane, its pixel and whether the oracle's ray hits"""
    assert got.shape == exp.shape, (name, case.name, array, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    if len(bad) == 0:
        return
    s, kk, lane, w = (int(x) for x in bad[0])
    tx, ty = gc.slot_tiles(case)[s]
    i, j = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
    inside = bool(ref.inside[s, kk, lane])
    what = "outside the image: must hold the fill" if not inside else ("fill expected" if exp[s, kk, lane, w] == gc.FILL else "")
    pytest.fail("%s %s pre_hits=%d: %s[slot %d][k %d][lane %d].%s = 0x%08X, oracle 0x%08X; pixel (%d, %d) of %dx%d, seed %d %s; %d words differ in %d records"
                % (name, case.name, pre_hits, array, s, case.k0 + kk, lane, FIELDS[array][w], got[s, kk, lane, w], exp[s, kk, lane, w], i, j, case.W, case.H,
                   case.seed, what, len(bad), len(np.unique(bad[:, :3], axis=0))))


# ---- the records against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre_hits", [0, 1])
@pytest.mark.parametrize("name", gc.CONTEXTS)
def test_records_equal_the_oracle_word_for_word(name, pre_hits):
    ctx = gc.context(name)
    n_rec = n_hit = 0
    for case in gc.cases_of(name):
        ref = gc.reference(name, case)
        ray, st, hit = generate(name, case, pre_hits)
        e_ray, e_st, e_hit = ref.words(pre_hits)
        assert_words(name, case, pre_hits, "ray", ray, e_ray, ref)      # direction and lambda_0; the fill outside a ragged image
        assert_words(name, case, pre_hits, "st", st, e_st, ref)         # {state, inc} after the draws; on a pre-traced miss {lambda_0, tail word, state}
        assert_words(name, case, pre_hits, "hit", hit, e_hit, ref)      # pre_hits 0: the fill throughout
        if pre_hits:
            inside, miss = ref.inside, ~ref.hit
            tri = hit[inside][:, 3].view(np.int32)
            assert np.array_equal(tri[miss], np.full(int(miss.sum()), -1)) and (tri[~miss] >= 0).all() and (tri[~miss] >> 1 < ctx.n_prims).all()
            y = st[inside][miss][:, 1]       # the tail word as resolve_records reads it: no hit, no emission, zero levels, no previous slot
            assert ((y & 1) == 0).all() and (((y >> 1) & 1) == 0).all() and (((y >> 2) & 0xF) == 0).all() and (((y >> 6) & 0x1FFF) == gc.NO_SLOT).all()
            plain = ~miss & (ctx.albedo_mode[tri.clip(0) >> 1] == 0)
            assert (hit[inside][plain][:, 1:3] == 0).all()                # +0 where the quad's albedo is no texture
            n_hit += int((~miss).sum())
        else:
            assert (hit == gc.FILL).all()
        assert (ray[~ref.inside] == gc.FILL).all() and (st[~ref.inside] == gc.FILL).all() and (hit[~ref.inside] == gc.FILL).all()
        n_rec += int(ref.inside.sum())
    print("%s pre_hits=%d: %d cases, %d records, %d hits" % (name, pre_hits, len(gc.cases_of(name)), n_rec, n_hit))
    assert n_rec > 8000 and (not pre_hits or n_hit >= 0.3 * n_rec)


def by_pixel(case, *arrays):
    """{(i, j, k): the record's words of every array, joined} of the records inside the image"""
    i, j, k, inside = gc.record_pixels(case)
    rows = np.concatenate([a[inside] for a in arrays], axis=1)
    return {key: row for key, row in zip(zip(i[inside].tolist(), j[inside].tolist(), k[inside].tolist()), rows)}


@pytest.mark.parametrize("name", ["cornell-srgb", "plane-srgb", "prims70"])
def test_a_sample_is_the_same_words_in_every_layout_mode_and_launch(name):
    """device against device: records of the same (pixel, k) across the tile layouts, with and without the pre-trace, and from a launch that starts at k0 = 5
    against sample 5 of a launch that starts at 0"""
    whole = {}
    for pre in (0, 1):
        full = gc.LAYOUT_CASES[0]
        assert (full.first, full.stride, full.skew) == (0, 1, 0)
        whole[pre] = by_pixel(full, *generate(name, full, pre))
        assert len(whole[pre]) == full.W * full.H
        for case in gc.LAYOUT_CASES[1:]:
            part = by_pixel(case, *generate(name, case, pre))
            assert len(part) == int(gc.record_pixels(case)[3].sum()) > 0
            for key, row in part.items():
                assert np.array_equal(row, whole[pre][key]), (name, case.name, pre, key)
    n_hit = 0
    for key, row1 in whole[1].items():
        row0 = whole[0][key]
        assert np.array_equal(row0[:4], row1[:4]), (name, key)                      # ray
        if row1[11] != 0xFFFFFFFF:                                                   # a hit: the live stream in both modes
            assert np.array_equal(row0[4:8], row1[4:8]), (name, key)
            n_hit += 1
        else:                                                                        # a miss: the same final state, in the end-of-path places
            assert np.array_equal(row0[4:6], row1[6:8]) and row1[4] == row0[3], (name, key)
    assert n_hit > 0
    short, long = gc.K_CASES
    assert (short.k0, short.n_k, long.k0, long.n_k) == (5, 1, 0, 8) and short[1:3] == long[1:3] and short.seed == long.seed
    for pre in (0, 1):
        a, b = by_pixel(short, *generate(name, short, pre)), by_pixel(long, *generate(name, long, pre))
        assert len(a) == short.W * short.H
        for key, row in a.items():
            assert key[2] == 5 and np.array_equal(row, b[key]), (name, pre, key)


# ---- the call itself ----------------------------------------------------------------------------------------------------------------------------
def test_generate_call_leaves_the_context_alone_and_checks_its_arguments():
    """it touches neither the sums nor the sample arrays: a render can be continued across it; and what it refuses"""
    name, (W, H) = "prims33", (24, 20)
    ctx = gc.context(name)
    orc = ctx.oracle
    r = Renderer(Options(scene_name="cornell", res=(W, H), spp=4, seed=3, observer=ctx.observer))
    r.upload_scene_desc(ctx._custom.desc(orc))
    r.render_start(); r.render_wait()
    before = r.xyza.copy()
    case = gc.Case("24x20", W, H, 2, 3, 3, 0, 1, 0)
    ref = gc.reference(name, case)
    for pre in (1, 0, -1):
        ray, st, hit = r.debug_generate(case.k0, case.n_k, pre)
        mode = r.plan_info()["camera_rays"].startswith("pre-traced") if pre < 0 else bool(pre)
        for array, got, exp in zip(("ray", "st", "hit"), (ray, st, hit), ref.words(mode)):
            assert_words(name, case, pre, array, got, exp, ref)
    r.xyza[:] = 0.0
    r.read_framebuffer()
    assert r.done_spp() == 4 and np.array_equal(r.xyza.view(np.uint32), before.view(np.uint32))
    r.render_continue(4); r.render_wait()
    assert np.array_equal(r.xyza.view(np.uint32), orc.render(W, H, 8, seed=3).view(np.uint32))
    # arguments
    lib, p = r._lib, r.params()
    n = ((W + 7) // 8) * ((H + 7) // 8) * 64
    buf = [np.zeros((n * 3, 4), dtype=np.uint32) for _ in range(3)]
    ptr = [b.ctypes.data for b in buf]

    def refused(k0, n_k, pre, hit=ptr[2], params=p, ray=ptr[0], st=ptr[1]):
        rc = lib.ssx_debug_generate(r._ctx, params, k0, n_k, pre, ray, st, hit)
        return rc == _capi.SSX_ERR_ARG and (params is None or ray is None or st is None or b"ssx_debug_generate" in lib.ssx_last_error(r._ctx)
                                            or params.width == 0)
    assert refused(0, 0, 0)                                         # n_k == 0
    assert refused(0xFFFFFFFE, 2, 0) and refused(0xFFFFFFFF, 1, 0)   # k0 + n_k beyond 32 bits
    assert lib.ssx_debug_generate(r._ctx, p, 0xFFFFFFFC, 3, 0, *ptr) == _capi.SSX_OK      # ... and the largest that fits
    assert refused(0, 1, 1, hit=None)                               # camera rays pre-traced and nowhere to put the hits
    assert lib.ssx_debug_generate(r._ctx, p, 0, 1, 0, ptr[0], ptr[1], None) == _capi.SSX_OK
    assert refused(0, 1, 2) and refused(0, 1, -2)
    assert refused(0, 65537, 0, params=r.params(width=8, height=8))  # more samples per pixel than any plan gives one launch
    assert refused(0, 1, 0, params=r.params(width=0)) and refused(0, 1, 0, params=None) and refused(0, 1, 0, ray=None) and refused(0, 1, 0, st=None)
    r.render_continue(2); r.render_wait()                            # the refusals left it alone, too
    assert np.array_equal(r.xyza.view(np.uint32), orc.render(W, H, 10, seed=3).view(np.uint32))
    r.close()


# ---- fused generation: the path kernel's refill against the generate kernel ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_workers(tmp_path_factory):
    """the oracle's samples and image, computed once and passed by file; one fresh process per mode, side by side"""
    (W, H), spp, seed = gc.FUSED_RES, gc.FUSED_SPP, gc.FUSED_SEED
    orc = ol.Oracle("plane-srgb", texture="test-img.png")
    xyza, state, _ = orc.samples(W, H, spp, seed=seed)
    path = str(tmp_path_factory.mktemp("generate") / "oracle.npz")
    np.savez(path, xyza=xyza, state=state, image=orc.render(W, H, spp, seed=seed))
    procs = {}
    for mode in gc.FUSED_MODES:
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SSX_FUSE_GEN", "SSX_PRE_HITS", "SSX_GENERIC_KERNEL"):
            env.pop(k, None)
        if mode != "default":
            env.update(SSX_DEBUG_ENV="1", SSX_FUSE_GEN=mode)
        procs[mode] = subprocess.Popen([sys.executable, os.path.join(HERE, "generate_worker.py"), path], cwd=ROOT, env=env,
                                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    yield procs
    for p in procs.values():
        if p.poll() is None:
            p.kill()


@pytest.mark.parametrize("mode", list(gc.FUSED_MODES))
def test_fused_and_unfused_generation_equal_the_oracle(fused_workers, mode):
    p = fused_workers[mode]
    try:
        out, err = p.communicate(timeout=300)
    except subprocess.TimeoutExpired:
        p.kill()
        pytest.fail("SSX_FUSE_GEN=%s: worker timed out" % mode)
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, err[-2000:])
    rep = json.loads(lines[-1])
    print(rep)
    assert rep["env"].get("SSX_FUSE_GEN") == (None if mode == "default" else mode)
    assert rep["pass1"] == "plane topology" and rep["camera_rays"] == "path loop"
    assert rep["samples"] and rep["states"] and rep["image"] and 0 < rep["owned_pixels"] < gc.FUSED_RES[0] * gc.FUSED_RES[1]
    # which way the launches went, from the library's own count at the place that decides it: the variable did what it says
    assert rep["launches_before"] == {"generate_launches": 0, "fused_launches": 0}
    for key in ("launches_samples", "launches_image"):
        made, fused = rep[key]["generate_launches"], rep[key]["fused_launches"]
        assert (made == 0 and fused >= 1) if gc.FUSED_MODES[mode] == "fused" else (fused == 0 and made >= 1), (mode, key, rep[key])
