"""Progressive rendering on the GPU: ssx_render_continue, export / import of the pixel sums, checkpoint files, the noise estimate by batch
means and render_until.  The reference of every image is the CPU oracle at the sample count in question, never another GPU render;
"equals" is np.array_equal on the uint32 view."""
import ctypes as C
import functools
import math
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import glibc_oracle as go
import oracle_lib as ol
from simple_spectral_amd import Options, Renderer, _capi
from simple_spectral_amd.dist import tile_owner_mask
from simple_spectral_amd.renderer import SsxError, load_checkpoint_file, merge_sums

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
TEX = "test-img.png"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def oracle(scene="cornell-srgb", kind=""):
    if kind == "glibc":
        return go.Oracle(scene, texture=TEX)
    return ol.Oracle(scene, texture=TEX, rgb=(kind == "rgb"))


@functools.lru_cache(maxsize=None)
def want(scene, kind, W, H, spp, seed):
    """The oracle's image at `spp` samples per pixel (computed once per count, shared, never written to)."""
    a = oracle(scene, kind).render(W, H, spp, seed=seed)
    a.setflags(write=False)
    return a


def wait(r):
    r.render_wait()
    return r.xyza.copy()


def start(r, spp, **over):
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=spp, **over))))
    return wait(r)


def cont(r, spp):
    r.render_continue(spp)
    return wait(r)


# ---- 1. continuation is exact ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,kind,opts", [
    ("cornell-srgb", "", {}),
    ("plane-srgb", "", {}),                                   # fused sample generation (no generate kernel)
    ("cornell-srgb", "glibc", dict(libm="glibc-2.35")),
    ("cornell-srgb", "rgb", dict(render_mode="rgb")),
    ("cornell-srgb", "", dict(spp_per_launch=1)),
    ("cornell-srgb", "", dict(spp_per_launch=3)),
])
def test_continued_render_equals_the_oracle_at_every_count(scene, kind, opts):
    W, H, seed = 50, 37, 4                                    # ragged: 7 x 5 tiles
    r = Renderer(Options(scene_name=scene, res=(W, H), seed=seed, texture=TEX, **opts))
    total = 0
    for n, call in ((5, start), (7, cont), (1, cont), (20, cont)):
        img = call(r, n)
        total += n
        assert r.done_spp() == total
        assert np.array_equal(bits(img), bits(want(scene, kind, W, H, total, seed))), "after %d samples" % total
    assert r.done_spp() == 33 and not r.is_rendering() and r.progress() == 1.0


def test_continue_after_a_stopped_render():
    W, H, seed, spp = 24, 16, 4, 1 << 20
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=seed, texture=TEX, spp=spp, spp_per_launch=1))
    r.render_start()
    while r.done_spp() < 1 and r.is_rendering():
        pass
    r.render_stop()
    wait(r)
    done = r.done_spp()
    assert 1 <= done < spp
    total = (done // 16 + 1) * 16                             # on to a round total
    img = cont(r, total - done)
    assert r.done_spp() == total
    assert np.array_equal(bits(img), bits(want("cornell-srgb", "", W, H, total, seed)))


def test_continue_after_a_finished_tile_major_render():
    W, H, seed = 50, 37, 4
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=seed, texture=TEX, tile_major=True))
    assert np.array_equal(bits(start(r, 5)), bits(want("cornell-srgb", "", W, H, 5, seed)))
    assert np.array_equal(bits(cont(r, 7)), bits(want("cornell-srgb", "", W, H, 12, seed))) and r.done_spp() == 12


# ---- 2. checkpoint round trip in a fresh process ----------------------------------------------------------------------------------------

CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from simple_spectral_amd import Options, Renderer
r = Renderer(Options(scene_name="cornell-srgb", res=(50, 37), seed=4, texture="test-img.png"))
info = r.load_checkpoint(sys.argv[1])
assert info.done_spp == 12 and r.done_spp() == 12
np.save(sys.argv[2], r.xyza)
r.render_continue(12)
r.render_wait()
assert r.done_spp() == 24
np.save(sys.argv[3], r.xyza)
"""


def test_checkpoint_is_resumed_by_a_fresh_process(tmp_path):
    W, H, seed = 50, 37, 4
    ck, a, b = str(tmp_path / "c.ckpt"), str(tmp_path / "a.npy"), str(tmp_path / "b.npy")
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=seed, texture=TEX))
    start(r, 12)
    r.save_checkpoint(ck)
    r.close()
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT, ck, a, b], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(bits(np.load(a)), bits(want("cornell-srgb", "", W, H, 12, seed)))   # before any rendering
    assert np.array_equal(bits(np.load(b)), bits(want("cornell-srgb", "", W, H, 24, seed)))


# ---- 3. partition independence ----------------------------------------------------------------------------------------------------------

PW, PH, PSEED = 72, 40, 4   # 9 tile columns


@pytest.fixture(scope="module")
def whole_checkpoint(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ckpt") / "whole.ckpt")
    r = Renderer(Options(scene_name="cornell-srgb", res=(PW, PH), seed=PSEED, texture=TEX))
    start(r, 5)
    r.save_checkpoint(path)
    r.close()
    return path


@pytest.mark.parametrize("world,skew", [(2, 0), (3, 1), (8, 1)])
def test_checkpoint_of_one_context_is_resumed_by_many(whole_checkpoint, tmp_path, world, skew):
    at5, at9 = want("cornell-srgb", "", PW, PH, 5, PSEED), want("cornell-srgb", "", PW, PH, 9, PSEED)
    total = np.zeros_like(at9)
    exports = []
    for rank in range(world):
        r = Renderer(Options(scene_name="cornell-srgb", res=(PW, PH), seed=PSEED, texture=TEX, tile_first=rank, tile_stride=world, tile_skew=skew))
        r.load_checkpoint(whole_checkpoint)
        mask = tile_owner_mask(PW, PH, rank, world, skew)
        assert np.array_equal(bits(r.xyza)[mask], bits(at5)[mask]) and not bits(r.xyza)[~mask].any()
        img = cont(r, 4)
        assert r.done_spp() == 9
        assert np.array_equal(bits(img)[mask], bits(at9)[mask]), "rank %d" % rank
        assert not bits(img)[~mask].any()                     # foreign pixels: exactly +0
        total += img
        if (world, skew) == (3, 1):
            exports.append(r.export_sums())
        r.close()
    assert np.array_equal(bits(total), bits(at9))
    if exports:   # ... and back: the three ranks' sums merged by ownership, resumed by one context
        info0 = exports[0][0]
        merged = np.zeros((PH, PW, 4))
        for info, sums, _ in exports:
            assert (info.tile_stride, info.tile_skew, info.done_spp) == (3, 1, 9)
            merge_sums(merged, None, sums, None, info)
        info0.tile_first, info0.tile_stride, info0.tile_skew = 0, 1, 0
        path = str(tmp_path / "merged.ckpt")
        assert _capi.host_lib().ssh_checkpoint_save(path.encode(), C.byref(info0), b"cornell-srgb", b"", merged.ctypes.data, None) == 0
        r = Renderer(Options(scene_name="cornell-srgb", res=(PW, PH), seed=PSEED, texture=TEX))
        r.load_checkpoint(path)
        assert np.array_equal(bits(r.xyza), bits(at9))
        assert np.array_equal(bits(cont(r, 3)), bits(want("cornell-srgb", "", PW, PH, 12, PSEED)))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------

def refused(fn, code, *words):
    with pytest.raises(SsxError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_continue_is_refused_without_continuable_sums():
    W, H = 24, 16
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=1, texture=TEX))
    go_on = lambda: r.render_continue(2)
    refused(go_on, _capi.SSX_ERR_STATE)                                  # nothing rendered yet
    start(r, 2)
    refused(lambda: r.render_continue(0), _capi.SSX_ERR_ARG)
    refused(lambda: r.render_continue(0xFFFFFFFF), _capi.SSX_ERR_ARG)    # 2 + 2^32 - 1
    r.upload_scene_desc(r.scene.desc)
    refused(go_on, _capi.SSX_ERR_STATE)                                  # after ssx_upload_scene
    start(r, 2)
    r.render_device(r._lib.ssx_device_framebuffer(r._ctx), spp=2)         # (into the context's own image buffer: any W*H float4 on the device)
    r.render_device_wait()
    refused(go_on, _capi.SSX_ERR_STATE)                                  # after ssx_render_device
    refused(r.export_sums, _capi.SSX_ERR_STATE)
    # a stopped tile_major render: its tiles hold different counts
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=1 << 17, spp_per_launch=8192, tile_major=1))))   # (five of the six tiles per launch)
    r.render_stop()
    wait(r)
    assert r.done_tiles() < 6
    refused(go_on, _capi.SSX_ERR_STATE)
    # while rendering
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=1 << 20, spp_per_launch=1))))
    assert r.is_rendering()
    refused(go_on, _capi.SSX_ERR_STATE, "render in progress")
    r.render_stop()
    wait(r)
    cont(r, 1)                                                           # (the stopped sample-walking render is continuable)
    r.close()
    # Every entry point that overwrites or reinterprets the sums leaves nothing to continue or to export, and a render brings both back.
    # 16 x 16: two tiles per row.  (An ssx_sums_import refused AFTER its argument checks would belong here: only a failing HIP call gets that far.)
    s = Renderer(Options(scene_name="cornell-srgb", res=(16, 16), seed=1, texture=TEX))

    def render_device():
        s.render_device(s._lib.ssx_device_framebuffer(s._ctx), spp=2)
        s.render_device_wait()

    for overwrite in (lambda: s.upload_scene_desc(s.scene.desc), render_device, lambda: s.debug_samples(spp=2)):
        start(s, 2)
        assert s.export_sums()[0].done_spp == 2                          # continuable sums ...
        overwrite()
        refused(lambda: s.render_continue(2), _capi.SSX_ERR_STATE)       # ... are gone
        refused(s.export_sums, _capi.SSX_ERR_STATE)
    start(s, 2)
    assert np.array_equal(bits(cont(s, 2)), bits(want("cornell-srgb", "", 16, 16, 4, 1))) and s.export_sums()[0].done_spp == 4


def test_import_is_refused_for_other_renders():
    W, H = 24, 16
    base = dict(scene_name="cornell-srgb", res=(W, H), seed=1, texture=TEX)
    r = Renderer(Options(**base))
    start(r, 3)
    info, sums, _ = r.export_sums()
    assert info.scene_digest == r.scene_digest() != 0
    for over, word in ((dict(seed=2), "seed"), (dict(res=(32, 16)), "size"), (dict(libm="glibc-2.35"), "libm"),
                       (dict(indirect_only=True), "indirect_only"), (dict(light_scale=31.0), "scene_digest")):
        other = Renderer(Options(**dict(base, **over)))
        refused(lambda: other.import_sums(info, sums), _capi.SSX_ERR_ARG, word)
        refused(lambda: other.render_continue(1), _capi.SSX_ERR_STATE)
        other.close()
    # one rank's unmerged export holds +0 outside its tiles: only a partition inside them may take it
    half = Renderer(Options(**dict(base, tile_first=1, tile_stride=2)))
    start(half, 3)
    hinfo, hsums, _ = half.export_sums()
    for over in (dict(), dict(tile_first=0, tile_stride=2), dict(tile_first=1, tile_stride=2, tile_skew=1), dict(tile_first=0, tile_stride=4)):
        other = Renderer(Options(**dict(base, **over)))
        refused(lambda: other.import_sums(hinfo, hsums), _capi.SSX_ERR_ARG, "tile ownership")
        other.close()
    for over in (dict(tile_first=1, tile_stride=2), dict(tile_first=3, tile_stride=4)):   # the same tiles, and half of them
        other = Renderer(Options(**dict(base, **over)))
        other.import_sums(hinfo, hsums)
        mask = tile_owner_mask(W, H, over["tile_first"], over["tile_stride"])
        assert np.array_equal(bits(other.xyza)[mask], bits(want("cornell-srgb", "", W, H, 3, 1))[mask]) and not bits(other.xyza)[~mask].any()
        other.close()
    same = Renderer(Options(**base))
    assert same.scene_digest() == info.scene_digest                      # the same description: the same digest in another context
    same.import_sums(info, sums)
    assert np.array_equal(bits(same.xyza), bits(want("cornell-srgb", "", W, H, 3, 1)))


DIGEST_CHILD = """
import sys
sys.path.insert(0, %r)
from simple_spectral_amd import Options, Renderer
kw = dict(jh_coeff_path=sys.argv[2]) if sys.argv[1] == "jh" else dict(meng_grid_path=sys.argv[2])
print(Renderer(Options(scene_name="cornell-srgb", res=(16, 16), texture="test-img.png", uplift=sys.argv[1], **kw)).scene_digest())
"""


@pytest.mark.parametrize("uplift", ["jh", "meng"])
def test_scene_digest_covers_the_uplift_tables_and_is_the_same_in_another_process(uplift, tmp_path):
    base = dict(scene_name="cornell-srgb", res=(16, 16), texture=TEX)
    path = str(tmp_path / "table.bin")
    if uplift == "jh":
        kw = dict(uplift="jh", jh_res=8, jh_coeff_path=path)             # fitted here and written; the child loads the file
    else:
        import ref_lib
        from simple_spectral_amd import meng
        table = ref_lib.meng_table()
        meng.save_table(path, table)
        kw = dict(uplift="meng", meng_grid_path=path)
    r = Renderer(Options(**base, **kw))
    mine = r.scene_digest()
    assert mine not in (0, Renderer(Options(**base)).scene_digest())
    p = subprocess.run([sys.executable, "-c", DIGEST_CHILD % ROOT, uplift, path], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert int(p.stdout.split()[-1]) == mine
    # one value of the table changed: another digest
    if uplift == "jh":
        raw = bytearray(open(path, "rb").read())
        raw[-2] ^= 0x01                                                  # a mantissa bit of the last coefficient
        open(path, "wb").write(bytes(raw))
    else:
        table["points"] = np.array(table["points"], dtype=np.float32, copy=True)
        table["points"].reshape(-1)[-1] += np.float32(1e-3)
        meng.save_table(path, table)
    assert Renderer(Options(**base, **kw)).scene_digest() != mine


# ---- 5. / 6. the noise estimate and render_until ----------------------------------------------------------------------------------------

NW, NH, NSEED, NSTEP, NMAX = 32, 24, 7, 8, 64


@functools.lru_cache(maxsize=None)
def noise_reference():
    """From the oracle's samples, as include/ssx.h defines it: per count n = 16, 24, ... 64 (batches of 8) the per-pixel v, the sums A and the
    image-level noise."""
    xyza, _, _ = oracle().samples(NW, NH, NMAX, seed=NSEED)
    y = (xyza[..., 1] * np.float32(0.001)).astype(np.float32)            # float(sample * 0.001f)
    assert y.dtype == np.float32
    run = np.cumsum(y.astype(np.float64), axis=2)                        # the sequential binary64 running sum
    ends = run[..., NSTEP - 1::NSTEP]                                    # A after each batch
    out = {}
    s2 = np.zeros((NH, NW))
    prev = np.zeros((NH, NW))
    for b in range(NMAX // NSTEP):
        d = ends[..., b] - prev
        s2 = s2 + d * d / float(NSTEP)
        prev = ends[..., b]
        B, N, A = b + 1, float((b + 1) * NSTEP), ends[..., b]
        if B >= 2:
            v = ((s2 - A * A / N) / float(B - 1)) / N
            v = np.where(v > 0.0, v, 0.0)
            n = float(NW * NH)
            out[(b + 1) * NSTEP] = (v, A, math.sqrt(math.fsum(v.ravel()) / n) / (math.fsum((A / N).ravel()) / n))
    return out


def test_noise_estimate_is_the_defined_function_of_the_samples():
    r = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX, spp=NMAX, spp_per_launch=NSTEP))
    refused(r.noise, _capi.SSX_ERR_STATE)                                # off
    r.render_start()
    plain = wait(r)
    # what ssx_scratch_info reported for this configuration before the estimate existed: the sample arrays of the calibration render at upload
    # (64 x 64 x 4 records of 48 bytes; this render's launches of 12 tiles x 8 samples need less) and the level logs of a 256-CU device
    # (16 wave slots per CU x 2 units x 2 cohorts x 128 records x 582 bytes)
    scratch_off = {"sample_bytes": 64 * 64 * 4 * 48, "log_bytes": 256 * 16 * 2 * 2 * 128 * 582}
    assert r.scratch_info() == scratch_off
    refused(r.noise, _capi.SSX_ERR_STATE)
    r.set_noise_estimate(True)
    r.render_start()
    img = wait(r)
    level, v = r.noise()
    ref_v, ref_A, ref_level = noise_reference()[NMAX]
    print("noise %.17g (reference %.17g), summary %r" % (level, ref_level, r.noise_summary))
    assert np.array_equal(v.view(np.uint64), ref_v.view(np.uint64))      # bit for bit
    sv, sa, n, B = r.noise_summary
    assert (n, B) == (NW * NH, NMAX // NSTEP) and B == 8
    fv, fa = math.fsum(ref_v.ravel()), math.fsum((ref_A / float(NMAX)).ravel())
    print("sum v %.17g (fsum %.17g), sum A/N %.17g (fsum %.17g)" % (sv, fv, sa, fa))
    assert abs(sv - fv) <= 1e-11 * fv and abs(sa - fa) <= 1e-11 * fa
    assert abs(level - ref_level) <= 1e-11 * ref_level
    # the estimate does not touch the sums, and costs no scratch of the render
    assert np.array_equal(bits(img), bits(want("cornell-srgb", "", NW, NH, NMAX, NSEED))) and np.array_equal(bits(img), bits(plain))
    assert r.scratch_info() == scratch_off
    info, sums, s2 = r.export_sums()
    assert info.noise_batches == 8 and np.array_equal(sums[..., 1].view(np.uint64), ref_A.view(np.uint64))
    r.set_noise_estimate(False)
    refused(r.noise, _capi.SSX_ERR_STATE)
    assert r.scratch_info() == scratch_off
    # carried through export / import: another context goes on from 40 samples and arrives at the same estimate
    a = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX))
    a.set_noise_estimate(True)
    start(a, 40, spp_per_launch=NSTEP)
    info, sums, s2 = a.export_sums()
    assert info.noise_batches == 5 and s2 is not None
    b = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX, spp_per_launch=NSTEP))
    b.set_noise_estimate(True)
    b.import_sums(info, sums, s2)
    assert np.array_equal(b.noise()[1].view(np.uint64), noise_reference()[40][0].view(np.uint64))
    cont(b, 24)
    assert np.array_equal(b.noise()[1].view(np.uint64), ref_v.view(np.uint64))


def free_device_memory():
    """hipMemGetInfo of the one HIP runtime this process has mapped (the library's own)."""
    rts = _capi.mapped_hip_runtimes()
    assert len(rts) == 1, rts
    hip = C.CDLL(rts[0])
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_estimate_off_allocates_nothing():
    """16 bytes of state per pixel exist only while the estimate is on: 16 MiB at 1024^2, seen in the device's free memory (the slack of
    2 MiB allows for the allocator's granularity; a render that has its buffers allocates nothing)."""
    W = H = 1024
    state, slack = W * H * 16, 2 << 20
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=1, texture=TEX))
    start(r, 1)
    cont(r, 1)
    r.export_sums()                                                      # (the staging buffer of export is there from here on)
    f_off = free_device_memory()
    start(r, 1)
    cont(r, 1)
    assert abs(free_device_memory() - f_off) <= slack                    # off: start and continue allocate nothing
    r.set_noise_estimate(True)
    start(r, 1)
    cont(r, 1)
    f_on = free_device_memory()
    print("free device memory: estimate off %d, on %d (state %d)" % (f_off, f_on, state))
    assert f_off - f_on >= state - slack
    r.set_noise_estimate(False)                                          # ... and it is given back
    assert abs(free_device_memory() - f_off) <= slack
    start(r, 1)
    assert abs(free_device_memory() - f_off) <= slack


def test_noise_estimate_adopts_a_finished_tile_major_render_as_one_batch():
    """A tile_major render takes no batches; finished, it is continuable, and the continue that follows counts its sums as ONE batch:
    start(8), continue(8), continue(8) is the estimate of the batches {8, 8, 8}."""
    r = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX, tile_major=True, spp_per_launch=NSTEP))
    r.set_noise_estimate(True)
    start(r, NSTEP)
    refused(r.noise, _capi.SSX_ERR_STATE)                                # no batch yet
    assert r.export_sums()[0].noise_batches == 0
    cont(r, NSTEP)
    level, v = r.noise()
    assert r.noise_summary[3] == 2 and np.array_equal(v.view(np.uint64), noise_reference()[2 * NSTEP][0].view(np.uint64))
    img = cont(r, NSTEP)
    level, v = r.noise()
    ref_v, _, ref_level = noise_reference()[3 * NSTEP]
    assert r.noise_summary[3] == 3 and np.array_equal(v.view(np.uint64), ref_v.view(np.uint64))
    assert abs(level - ref_level) <= 1e-11 * ref_level
    assert np.array_equal(bits(img), bits(want("cornell-srgb", "", NW, NH, 3 * NSTEP, NSEED)))
    # render_until on a tile_major renderer goes the same way
    t = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX, tile_major=True))
    done, level = t.render_until(0.0, NSTEP, 3 * NSTEP)
    assert done == 3 * NSTEP and abs(level - ref_level) <= 1e-11 * ref_level
    assert np.array_equal(t.noise()[1].view(np.uint64), ref_v.view(np.uint64))


def test_render_until_stops_at_the_first_step_under_the_target():
    ref = noise_reference()
    levels = {n: ref[n][2] for n in sorted(ref)}
    print("noise per count: %r" % (levels,))
    target = 0.5 * (levels[32] + levels[40])
    first = next(n for n in sorted(levels) if levels[n] <= target)
    assert 2 * NSTEP < first < NMAX                                      # the case is one where the target decides, not the limits
    r = Renderer(Options(scene_name="cornell-srgb", res=(NW, NH), seed=NSEED, texture=TEX))
    done, level = r.render_until(target, NSTEP, NMAX)
    print("render_until(%.6g): %d samples, noise %.6g" % (target, done, level))
    assert done == first and r.done_spp() == first
    assert level <= target and abs(level - levels[first]) <= 1e-11 * levels[first]
    assert np.array_equal(bits(r.xyza), bits(want("cornell-srgb", "", NW, NH, first, NSEED)))
    done, level = r.render_until(0.0, NSTEP, NMAX)                       # a target that is never met: the limit decides
    assert done == NMAX and level > 0.0
    assert np.array_equal(bits(r.xyza), bits(want("cornell-srgb", "", NW, NH, NMAX, NSEED)))


# ---- 7. CLI -----------------------------------------------------------------------------------------------------------------------------

def test_cli_checkpoint_and_resume_equal_the_one_shot_render(tmp_path):
    common = ["-s=cornell-srgb", "-w=40", "-h=24", "--texture=data/scenes/test-img.png"]
    run = lambda *a, seed=9: subprocess.run([CLI] + common + ["--seed=%d" % seed] + list(a), cwd=ROOT, capture_output=True, text=True)
    ck, part, res, one = (str(tmp_path / n) for n in ("c.ckpt", "part.png", "resumed.png", "oneshot.png"))
    p = run("-spp=4", "-o=" + part, "--checkpoint=" + ck)
    assert p.returncode == 0, p.stderr
    assert load_checkpoint_file(ck)[0].done_spp == 4
    p = run("-spp=10", "-o=" + res, "--resume=" + ck, "--checkpoint=" + ck)
    assert p.returncode == 0 and "4 samples per pixel done, 10 wanted" in p.stderr, p.stderr
    p = run("-spp=10", "-o=" + one)
    assert p.returncode == 0, p.stderr
    assert open(res, "rb").read() == open(one, "rb").read()
    assert load_checkpoint_file(ck)[0].done_spp == 10
    # a total at or below the checkpoint's count: the image is written as it is
    again = str(tmp_path / "again.png")
    p = run("-spp=6", "-o=" + again, "--resume=" + ck)
    assert p.returncode == 0 and open(again, "rb").read() == open(one, "rb").read()
    # the oracle has the last word
    from PIL import Image
    o = oracle()
    srgba = o.to_srgba(o.render(40, 24, 10, seed=9))
    assert np.array_equal(np.asarray(Image.open(res)), np.floor(np.clip(np.float32(255.0) * srgba, 0, 255) + np.float32(0.5)).astype(np.uint8)[::-1])
    # not this render's checkpoint: the library's reason, the reference's exit code for bad data
    p = run("-spp=10", "-o=" + res, "--resume=" + ck, seed=10)
    assert p.returncode == 255 and "seed differs" in p.stderr
    open(ck, "r+b").write(b"XX")
    p = run("-spp=10", "-o=" + res, "--resume=" + ck)
    assert p.returncode == 255 and "not a checkpoint" in p.stderr
    # --noise-target: stops at a multiple of the step, at the latest at --max-samples
    p = run("-spp=1", "-o=" + res, "--noise-target=0", "--max-samples=24", "--noise-step=8", "--checkpoint=" + ck)
    assert p.returncode == 0 and "after 24 samples per pixel" in p.stderr, p.stderr
    info, _, s2, name, _ = load_checkpoint_file(ck)
    assert (info.done_spp, info.noise_batches, name) == (24, 3, "cornell-srgb") and s2 is not None


def test_cli_checkpoint_of_three_devices_is_resumed_by_two(tmp_path):
    """`--gpus=N` (SSX_TEST_ONE_GPU=1: all contexts on device 0, as in tests/test_cli.py): every context exports its tiles, the host merges by
    ownership; on resume every context imports the whole array and keeps its own tiles -- another number of devices than wrote the file."""
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    common = ["-s=cornell-srgb", "-w=72", "-h=40", "--texture=data/scenes/test-img.png", "--seed=4"]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True, env=env)
    ck, part, res = (str(tmp_path / n) for n in ("c.ckpt", "part.pfm", "resumed.png"))
    p = run("-spp=5", "-o=" + part, "--gpus=3", "--checkpoint=" + ck)
    assert p.returncode == 0, p.stderr
    info, sums, _, _, _ = load_checkpoint_file(ck)
    assert (info.done_spp, info.tile_first, info.tile_stride) == (5, 0, 1) and (sums[..., 3] > 0).any()
    p = run("-spp=9", "-o=" + res, "--gpus=2", "--resume=" + ck)
    assert p.returncode == 0, p.stderr
    from PIL import Image
    o = oracle()
    srgba = o.to_srgba(want("cornell-srgb", "", PW, PH, 9, PSEED))
    assert np.array_equal(np.asarray(Image.open(res)), np.floor(np.clip(np.float32(255.0) * srgba, 0, 255) + np.float32(0.5)).astype(np.uint8)[::-1])


def test_cli_abort_leaves_a_resumable_checkpoint(tmp_path):
    """Ctrl-C (the reference's abort path, as in tests/test_cli.py) with --checkpoint: the partial image is saved and the sums behind it too;
    resuming to the count reached writes that image again."""
    ck, out, again = (str(tmp_path / n) for n in ("c.ckpt", "partial.pfm", "again.pfm"))
    common = ["-s=cornell", "-w=512", "-h=512"]
    p = subprocess.Popen([CLI] + common + ["-spp=1000000", "-o=" + out, "--checkpoint=" + ck], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    seen = b""
    while b"%" not in seen:                                              # the first launch has finished
        chunk = p.stdout.read1(4096)
        assert chunk, "the render ended before it reported progress"
        seen += chunk
    p.send_signal(signal.SIGINT)
    so, se = p.communicate(timeout=120)
    assert p.returncode == 0, se
    assert b"Aborting: saving the partial render" in se
    info = load_checkpoint_file(ck)[0]
    assert 0 < info.done_spp < 1000000
    r = subprocess.run([CLI] + common + ["-spp=%d" % info.done_spp, "-o=" + again, "--resume=" + ck], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(again, "rb").read() == open(out, "rb").read()
