"""Progressive rendering, the parts that need no GPU: the checkpoint file (libssx_host.so), the merge of the ranks' exports by ownership mask,
the shape of the new C ABI and the CLI's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.dist import tile_owner_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
W, H = 21, 13   # ragged: 3 x 2 tiles


def make_info(**kw):
    info = _capi.SsxSumsInfo()
    info.struct_size = C.sizeof(_capi.SsxSumsInfo)
    info.width, info.height, info.done_spp, info.seed = W, H, 12, 0xFEDCBA9876543210
    info.libm, info.tile_stride, info.noise_batches, info.scene_digest = 1, 1, 3, 0x0123456789ABCDEF
    for k, v in kw.items():
        setattr(info, k, v)
    return info


def synthetic(seed=0):
    rs = np.random.RandomState(seed)
    sums = rs.uniform(0.0, 50.0, (H, W, 4))
    sums[3, 5] = [-0.0, 1e-300, 3.5, 1.0]          # signed zero, a denormal-range value
    s2 = rs.uniform(0.0, 9.0, (H, W))
    return sums, s2


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host():
    sbuild.build_host()
    return _capi.host_lib()


def test_capi_exposes_the_new_entry_points_and_the_info_struct_matches_the_header(tmp_path):
    for s in ("ssx_render_continue", "ssx_scene_digest", "ssx_sums_export", "ssx_sums_import", "ssx_set_noise_estimate", "ssx_noise_info"):
        assert s in _capi.HIP_SYMBOLS
    for s in ("ssh_checkpoint_save", "ssh_checkpoint_load", "ssh_sums_merge"):
        assert s in _capi.HOST_SYMBOLS
    src = ('#include "ssx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %d\\n",sizeof(ssx_sums_info_t),'
           'offsetof(ssx_sums_info_t,seed),offsetof(ssx_sums_info_t,noise_batches),offsetof(ssx_sums_info_t,scene_digest),SSX_ABI_VERSION);return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = list(map(int, subprocess.check_output([str(tmp_path / "t")]).split()))
    S = _capi.SsxSumsInfo
    assert got == [C.sizeof(S), S.seed.offset, S.noise_batches.offset, S.scene_digest.offset, 2]


@pytest.mark.parametrize("with_s2", [True, False])
def test_checkpoint_round_trip(host, tmp_path, with_s2):
    from simple_spectral_amd.renderer import load_checkpoint_file
    sums, s2 = synthetic()
    info = make_info(noise_batches=3 if with_s2 else 0, tile_first=0, tile_skew=1)
    path = str(tmp_path / "a.ckpt")
    rc = host.ssh_checkpoint_save(path.encode(), C.byref(info), b"cornell-srgb", b"observer=1931\ntexture=test-img.png\n", sums.ctypes.data,
                                  s2.ctypes.data if with_s2 else None)
    assert rc == 0, host.ssh_last_error()
    raw = open(path, "rb").read()
    assert raw[:8] == b"SSXCKPT1" and len(raw) > sums.nbytes + (s2.nbytes if with_s2 else 0)
    got, gs, g2, name, text = load_checkpoint_file(path)
    assert bytes(got) == bytes(info)
    assert name == "cornell-srgb" and text == "observer=1931\ntexture=test-img.png\n"
    assert np.array_equal(bits64(gs), bits64(sums)) and gs.shape == (H, W, 4)
    assert (g2 is None) == (not with_s2) and (g2 is None or np.array_equal(bits64(g2), bits64(s2)))


def test_damaged_checkpoints_are_refused_as_bad_data(host, tmp_path):
    from simple_spectral_amd.renderer import SsxError, load_checkpoint_file
    sums, s2 = synthetic(1)
    info = make_info()
    path = str(tmp_path / "a.ckpt")
    assert host.ssh_checkpoint_save(path.encode(), C.byref(info), b"cornell", b"", sums.ctypes.data, s2.ctypes.data) == 0
    raw = open(path, "rb").read()
    load_checkpoint_file(path)
    bad = {"truncated": raw[:len(raw) // 2], "cut by one byte": raw[:-1], "no checksum": raw[:-8], "empty": b"", "header only": raw[:40],
           "wrong magic": b"SSXMENG1" + raw[8:], "one more byte": raw + b"\0",
           "payload bit": raw[:len(raw) - 4000] + bytes([raw[len(raw) - 4000] ^ 0x10]) + raw[len(raw) - 3999:],
           "header bit": raw[:20] + bytes([raw[20] ^ 1]) + raw[21:],
           "checksum bit": raw[:-1] + bytes([raw[-1] ^ 0x80])}
    for what, data in bad.items():
        p = str(tmp_path / "bad.ckpt")
        open(p, "wb").write(data)
        with pytest.raises(SsxError) as e:
            load_checkpoint_file(p)
        assert e.value.code == _capi.SSX_ERR_DATA, what
    with pytest.raises(SsxError) as e:
        load_checkpoint_file(str(tmp_path / "missing.ckpt"))
    assert e.value.code == _capi.SSX_ERR_DATA


@pytest.mark.parametrize("world,skew", [(3, 1), (2, 0), (8, 5)])
def test_merge_by_ownership_mask_reproduces_the_whole_array(host, world, skew):
    from simple_spectral_amd.renderer import merge_sums
    full, full2 = synthetic(2)
    assert np.signbit(full[3, 5, 0])
    dst, dst2 = np.full((H, W, 4), 7.0), np.full((H, W), 7.0)   # (every pixel has exactly one owner: nothing of this survives)
    for r in range(world):
        mask = tile_owner_mask(W, H, r, world, skew)
        part = np.where(mask[..., None], full, 0.0)             # a rank's export: +0 where it owns nothing
        part2 = np.where(mask, full2, 0.0)
        merge_sums(dst, dst2, part, part2, make_info(tile_first=r, tile_stride=world, tile_skew=skew))
    assert np.array_equal(bits64(dst), bits64(full)) and np.array_equal(bits64(dst2), bits64(full2))
    added = sum(np.where(tile_owner_mask(W, H, r, world, skew)[..., None], full, 0.0) for r in range(world))
    assert not np.array_equal(bits64(added), bits64(full))      # adding the exports loses the sign of -0.0: why the merge goes by the mask


def test_cli_refuses_progressive_flags_that_cannot_work(tmp_path):
    sbuild.build_host()
    common = ["-s=cornell", "-w=8", "-h=8", "-spp=4", "-o=" + str(tmp_path / "x.png")]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True)
    r = run("--resume=" + str(tmp_path / "a.ckpt"), "--tile-major")
    assert r.returncode == 255 and "--tile-major" in r.stderr and "--resume" in r.stderr and "Simple Spectral" in r.stdout
    r = run("--noise-target=0.01")
    assert r.returncode == 255 and "`--noise-target` needs `--max-samples=<n>`" in r.stderr
    r = run("--noise-target=nope", "--max-samples=64")
    assert r.returncode == 255 and "Invalid value for --noise-target" in r.stderr
    r = run("--checkpoint=" + str(tmp_path / "a.ckpt"), "--tile-major")
    assert r.returncode == 255 and "--checkpoint" in r.stderr
    assert not os.path.exists(str(tmp_path / "x.png"))
