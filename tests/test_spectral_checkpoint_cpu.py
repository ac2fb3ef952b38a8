"""The wavelength bins through checkpoint and resume, the parts that need no GPU: the SSXCKPT2 file (libssx_host.so), the merge of the ranks' bins by ownership
mask, the new entry points and the CLI's argument rules.  "equals" is np.array_equal on the integer views (bit for bit)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.dist import tile_owner_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
W, H = 13, 9    # ragged: 2 x 2 tiles
NAN_PAYLOAD = 0x7FF4000000ABCDEF   # a signalling NaN with a payload: only a copy of the bytes keeps it


def sums_info(**kw):
    info = _capi.SsxSumsInfo()
    info.struct_size = C.sizeof(_capi.SsxSumsInfo)
    info.width, info.height, info.done_spp, info.seed = W, H, 12, 0xFEDCBA9876543210
    info.tile_stride, info.noise_batches, info.scene_digest = 1, 3, 0x0123456789ABCDEF
    for k, v in kw.items():
        setattr(info, k, v)
    return info


def spectral_info(bins, **kw):
    s = _capi.SsxSpectralInfo()
    s.struct_size = C.sizeof(_capi.SsxSpectralInfo)
    s.width, s.height, s.bins, s.done_spp, s.lambda_min, s.bin_width = W, H, bins, 12, 360.0, 117.5 / (bins // 4)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def synthetic(bins, seed=0):
    """(pixel sums [H, W, 4], S2 [H, W], bin sums [H, W, B], counts [H, W, B / 4]) with the values a careless copy loses"""
    rs = np.random.RandomState(seed)
    sums, s2 = rs.uniform(0.0, 50.0, (H, W, 4)), rs.uniform(0.0, 9.0, (H, W))
    S = rs.uniform(0.0, 50.0, (H, W, bins))
    S[3, 5, 0], S[3, 5, 1], S[8, 12, bins - 1] = -0.0, np.inf, -np.inf
    S.view(np.uint64)[0, 0, 2] = NAN_PAYLOAD
    N = rs.randint(0, 2 ** 32, (H, W, bins // 4), dtype=np.uint64).astype(np.uint32)
    return sums, s2, S, N


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def host():
    sbuild.build_host()
    return _capi.host_lib()


def save(host, path, info, sums, s2, sinfo=None, S=None, N=None):
    return host.ssh_checkpoint_save_spectral(os.fsencode(path), C.byref(info), b"cornell-srgb", b"observer=1931\n", sums.ctypes.data, None if s2 is None else s2.ctypes.data,
                                             None if sinfo is None else C.byref(sinfo), None if S is None else S.ctypes.data, None if N is None else N.ctypes.data)


def test_new_entry_points_are_declared_bound_and_exported(host):
    assert "ssx_spectral_import" in _capi.HIP_SYMBOLS
    for s in ("ssh_checkpoint_save_spectral", "ssh_checkpoint_load_spectral", "ssh_spectral_merge"):
        assert s in _capi.HOST_SYMBOLS and hasattr(host, s), s
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "int ssx_spectral_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* sums" in header
    from simple_spectral_amd import Renderer
    from simple_spectral_amd import renderer as rmod
    for m in ("export_spectral", "import_spectral"):
        assert callable(getattr(Renderer, m))
    assert callable(rmod.load_checkpoint_file_spectral) and callable(rmod.merge_spectral)


@pytest.mark.parametrize("with_s2", [True, False])
@pytest.mark.parametrize("bins", [4, 64])
def test_spectral_checkpoint_round_trip(host, tmp_path, bins, with_s2):
    from simple_spectral_amd.renderer import load_checkpoint_file, load_checkpoint_file_spectral
    sums, s2, S, N = synthetic(bins)
    info, sinfo = sums_info(noise_batches=3 if with_s2 else 0), spectral_info(bins)
    path = str(tmp_path / "a.ckpt")
    assert save(host, path, info, sums, s2 if with_s2 else None, sinfo, S, N) == 0, host.ssh_last_error()
    raw = open(path, "rb").read()
    assert raw[:8] == b"SSXCKPT2"
    # the layout: the SSXCKPT1 fields up to s2, then the counted ssx_spectral_info_t, S, N, the checksum
    tail = 4 + C.sizeof(sinfo) + S.nbytes + N.nbytes + 8
    at = len(raw) - tail
    assert raw[at:at + 4] == np.uint32(C.sizeof(sinfo)).tobytes() and raw[at + 4:at + 4 + C.sizeof(sinfo)] == bytes(sinfo)
    assert raw[at + 4 + C.sizeof(sinfo):-8] == S.tobytes() + N.tobytes()
    assert raw[at - (s2.nbytes if with_s2 else 0) - sums.nbytes:at] == sums.tobytes() + (s2.tobytes() if with_s2 else b"")
    got, gs, g2, name, text, gsi, gS, gN = load_checkpoint_file_spectral(path)
    assert bytes(got) == bytes(info) and bytes(gsi) == bytes(sinfo) and name == "cornell-srgb" and text == "observer=1931\n"
    assert np.array_equal(bits64(gs), bits64(sums)) and (g2 is None) == (not with_s2) and (g2 is None or np.array_equal(bits64(g2), bits64(s2)))
    assert gS.shape == (H, W, bins) and gN.shape == (H, W, bins // 4) and gN.dtype == np.uint32
    assert np.array_equal(bits64(gS), bits64(S)) and np.array_equal(gN, N)
    assert bits64(gS)[0, 0, 2] == NAN_PAYLOAD and np.signbit(gS[3, 5, 0]) and gS[3, 5, 1] == np.inf
    # the older entry point reads the same file's pixel sums and passes over the bins
    got, gs, g2, name, text = load_checkpoint_file(path)
    assert bytes(got) == bytes(info) and np.array_equal(bits64(gs), bits64(sums)) and (g2 is None or np.array_equal(bits64(g2), bits64(s2)))


def test_without_spectral_info_the_file_is_todays(host, tmp_path):
    from simple_spectral_amd.renderer import load_checkpoint_file_spectral
    sums, s2, _, _ = synthetic(4)
    info = sums_info()
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    assert host.ssh_checkpoint_save(os.fsencode(a), C.byref(info), b"cornell-srgb", b"observer=1931\n", sums.ctypes.data, s2.ctypes.data) == 0
    assert save(host, b, info, sums, s2) == 0
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read() and raw[:8] == b"SSXCKPT1"
    *_, sinfo, S, N = load_checkpoint_file_spectral(a)
    assert sinfo.bins == 0 and S is None and N is None


def test_save_refuses_bins_that_do_not_belong_to_the_sums(host, tmp_path):
    sums, s2, S, N = synthetic(8)
    path = str(tmp_path / "a.ckpt")
    for bad in (dict(bins=6), dict(bins=0), dict(bins=68), dict(width=W + 1), dict(done_spp=11)):
        si = spectral_info(8)
        for k, v in bad.items():
            setattr(si, k, v)
        assert save(host, path, sums_info(), sums, s2, si, S, N) == _capi.SSX_ERR_ARG, bad
    assert save(host, path, sums_info(), sums, s2, spectral_info(8), S, None) == _capi.SSX_ERR_ARG
    assert not os.path.exists(path)


def test_damaged_spectral_checkpoints_are_refused_as_bad_data(host, tmp_path):
    from simple_spectral_amd.renderer import SsxError, load_checkpoint_file, load_checkpoint_file_spectral
    bins = 8
    sums, s2, S, N = synthetic(bins, 1)
    sinfo = spectral_info(bins)
    path = str(tmp_path / "a.ckpt")
    assert save(host, path, sums_info(), sums, s2, sinfo, S, N) == 0
    raw = open(path, "rb").read()
    section = len(raw) - (4 + C.sizeof(sinfo) + S.nbytes + N.nbytes + 8)   # where the spectral section begins
    flip = lambda at, bit=0x10: raw[:at] + bytes([raw[at] ^ bit]) + raw[at + 1:]
    word = lambda at, v: raw[:at] + np.uint32(v).tobytes() + raw[at + 4:]
    bins_at = section + 4 + _capi.SsxSpectralInfo.bins.offset
    bad = {"a bit in the bin sums": flip(section + 4 + C.sizeof(sinfo) + 1000), "a bit in the counts": flip(len(raw) - 8 - 10),
           "a bit in the spectral description": flip(section + 4 + _capi.SsxSpectralInfo.lambda_min.offset),
           "cut inside the bin sums": raw[:section + 4 + C.sizeof(sinfo) + S.nbytes // 2], "cut inside the counts": raw[:len(raw) - 8 - N.nbytes // 2],
           "cut inside the description": raw[:section + 10], "cut before the section": raw[:section], "cut by one byte": raw[:-1], "one more byte": raw + b"\0",
           "6 bins": word(bins_at, 6), "0 bins": word(bins_at, 0), "68 bins": word(bins_at, 68), "4 bins: arrays of another size": word(bins_at, 4),
           "another description size": word(section, C.sizeof(sinfo) + 4),
           "the older magic on the longer file": b"SSXCKPT1" + raw[8:]}
    for what, data in bad.items():
        p = str(tmp_path / "bad.ckpt")
        open(p, "wb").write(data)
        for load in (load_checkpoint_file_spectral, load_checkpoint_file):
            with pytest.raises(SsxError) as e:
                load(p)
            assert e.value.code == _capi.SSX_ERR_DATA, what


@pytest.mark.parametrize("bins", [4, 64])
def test_spectral_merge_equals_the_ownership_rule(host, bins):
    """tile_stride 3, tile_skew 1: the rule restated with numpy (tile t of the row-major list with tile row ty rotated by ty * skew columns belongs to rank
    t % stride) -- and dist.tile_owner_mask, the restatement the other tests use, agrees with it."""
    from simple_spectral_amd.renderer import merge_spectral
    stride, skew = 3, 1
    _, _, S, N = synthetic(bins, 2)
    tiles_x = (W + 7) // 8
    jj, ii = np.mgrid[0:H, 0:W]
    place = (jj // 8) * tiles_x + (ii // 8 + ((jj // 8) * (skew % tiles_x)) % tiles_x) % tiles_x
    dst_s, dst_n = np.full((H, W, bins), 7.0), np.full((H, W, bins // 4), 7, dtype=np.uint32)   # (every pixel has exactly one owner: nothing of this survives)
    for r in range(stride):
        mask = place % stride == r
        assert np.array_equal(mask, tile_owner_mask(W, H, r, stride, skew))
        part_s, part_n = np.where(mask[..., None], S, 0.0), np.where(mask[..., None], N, 0).astype(np.uint32)   # a rank's export: zeros where it owns nothing
        before = (dst_s.copy(), dst_n.copy())
        merge_spectral(dst_s, dst_n, part_s, part_n, sums_info(tile_first=r, tile_stride=stride, tile_skew=skew))
        assert np.array_equal(bits64(dst_s)[~mask], bits64(before[0])[~mask]) and np.array_equal(dst_n[~mask], before[1][~mask])   # foreign pixels untouched
    assert np.array_equal(bits64(dst_s), bits64(S)) and np.array_equal(dst_n, N)
    with np.errstate(invalid="ignore"):
        added = sum(np.where((place % stride == r)[..., None], S, 0.0) for r in range(stride))
    assert not np.array_equal(bits64(added), bits64(S))      # adding the exports loses -0.0 and the NaN's payload: why the merge goes by the mask
    assert host.ssh_spectral_merge(dst_s.ctypes.data, dst_n.ctypes.data, S.ctypes.data, N.ctypes.data, 6, C.byref(sums_info())) == _capi.SSX_ERR_ARG


def test_cli_argument_rules_of_a_spectral_resume(host, tmp_path):
    """What the CLI decides before it touches a device: a resume with a spectral option needs a checkpoint that holds as many bins as are asked for."""
    sums, s2, S, N = synthetic(8)
    sums1, bins8, missing = str(tmp_path / "sums.ckpt"), str(tmp_path / "bins8.ckpt"), str(tmp_path / "missing.ckpt")
    assert save(host, sums1, sums_info(), sums, s2) == 0 and save(host, bins8, sums_info(), sums, s2, spectral_info(8), S, N) == 0
    common = ["-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "-o=" + str(tmp_path / "x.png")]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True)
    for flags in (["--spectral-output=" + str(tmp_path / "s.npy")], ["--develop-output=" + str(tmp_path / "d.png"), "--spectral-bins=8"],
                  ["--spectral-output=" + str(tmp_path / "s.npy"), "--spectral-denoise"]):
        r = run("--resume=" + sums1, *flags)
        assert r.returncode == 255 and "cannot be combined with `--resume` of a checkpoint without wavelength bins" in r.stderr, r.stderr
        r = run("--resume=" + missing, *flags)
        assert r.returncode == 255 and "cannot be combined with `--resume` of a checkpoint that cannot be read" in r.stderr, r.stderr
    r = run("--resume=" + bins8, "--spectral-output=" + str(tmp_path / "s.npy"), "--spectral-bins=16")
    assert r.returncode == 255 and "cannot be combined with `--resume` of a checkpoint with another bin count" in r.stderr and "holds 8" in r.stderr, r.stderr
    assert "with `--resume` the checkpoint's" in r.stdout       # the usage text says what is now true
    assert not any(os.path.exists(str(tmp_path / n)) for n in ("x.png", "s.npy", "d.png"))
