"""The bins' second moments through checkpoint and resume, the parts that need no GPU: the SSXCKPT3 file (libssx_host.so), the merge of the ranks' Q by
ownership mask, the numpy restatement of ssx_spectral_moments_import's consistency check, the new entry points and the CLI's argument rules.  "equals" is
np.array_equal on the integer views (bit for bit; there are no tolerances)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import moments_import_ref as mref
import oracle_lib as ol
import spectral_stats_ref as sref
import test_spectral_checkpoint_cpu as base
from simple_spectral_amd import Scene, _capi, build as sbuild
from simple_spectral_amd.dist import tile_owner_mask

ROOT, CLI, W, H, NAN_PAYLOAD = base.ROOT, base.CLI, base.W, base.H, base.NAN_PAYLOAD
bits64, sums_info, spectral_info = base.bits64, base.sums_info, base.spectral_info


def synthetic_q(bins, seed=0):
    """Q [H, W, B] with the values a careless copy loses"""
    Q = np.random.RandomState(100 + seed).uniform(0.0, 2500.0, (H, W, bins))
    Q[3, 5, 0], Q[3, 5, 1], Q[H - 1, W - 1, bins - 1] = -0.0, np.inf, np.inf
    Q.view(np.uint64)[0, 0, 2] = NAN_PAYLOAD
    return Q


@pytest.fixture(scope="module")
def host():
    sbuild.build_host()
    return _capi.host_lib()


def save(host, path, info, sums, s2, sinfo=None, S=None, N=None, Q=None):
    ptr = lambda a: None if a is None else a.ctypes.data
    return host.ssh_checkpoint_save_moments(os.fsencode(path), C.byref(info), b"cornell-srgb", b"observer=1931\n", sums.ctypes.data, ptr(s2),
                                            None if sinfo is None else C.byref(sinfo), ptr(S), ptr(N), ptr(Q))


def test_new_entry_points_are_declared_bound_and_exported(host):
    assert "ssx_spectral_moments_import" in _capi.HIP_SYMBOLS
    for s in ("ssh_checkpoint_save_moments", "ssh_checkpoint_load_moments", "ssh_moments_merge"):
        assert s in _capi.HOST_SYMBOLS and hasattr(host, s), s
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "int ssx_spectral_moments_import(ssx_ctx* ctx, const ssx_spectral_info_t* info, const double* q" in header
    host_header = open(os.path.join(ROOT, "include", "ssx_host.h")).read()
    for s in ("int ssh_checkpoint_save_moments(", "int ssh_checkpoint_load_moments(", "int ssh_moments_merge("):
        assert s in host_header, s
    sbuild.build_all()
    exported = subprocess.run(["nm", "-D", "--defined-only", sbuild.HIP_LIB], capture_output=True, text=True, check=True).stdout
    assert " T ssx_spectral_moments_import" in exported
    from simple_spectral_amd import Renderer
    from simple_spectral_amd import renderer as rmod
    for m in ("export_moments", "import_moments", "holds_moments"):
        assert callable(getattr(Renderer, m))
    assert callable(rmod.load_checkpoint_file_moments) and callable(rmod.merge_moments)
    import inspect
    assert inspect.signature(Renderer.render_until_spectral).parameters["resume"].default is False


@pytest.mark.parametrize("with_s2", [True, False])
@pytest.mark.parametrize("bins", [4, 64])
def test_moments_checkpoint_round_trip(host, tmp_path, bins, with_s2):
    from simple_spectral_amd.renderer import load_checkpoint_file, load_checkpoint_file_moments, load_checkpoint_file_spectral
    sums, s2, S, N = base.synthetic(bins)
    Q = synthetic_q(bins)
    info, sinfo = sums_info(noise_batches=3 if with_s2 else 0), spectral_info(bins)
    path, older = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    assert save(host, path, info, sums, s2 if with_s2 else None, sinfo, S, N, Q) == 0, host.ssh_last_error()
    assert base.save(host, older, info, sums, s2 if with_s2 else None, sinfo, S, N) == 0
    raw, raw2 = open(path, "rb").read(), open(older, "rb").read()
    # the layout, byte by byte: the magic, the SSXCKPT2 file's bytes up to and including N, then Q, then the checksum over every byte before it
    assert raw[:8] == b"SSXCKPT3" and raw2[:8] == b"SSXCKPT2"
    assert raw[8:len(raw2) - 8] == raw2[8:-8] and raw[len(raw2) - 8:-8] == Q.tobytes() and len(raw) == len(raw2) + Q.nbytes
    assert raw[-8:] != raw2[-8:]
    got, gs, g2, name, text, gsi, gS, gN, gQ = load_checkpoint_file_moments(path)
    assert bytes(got) == bytes(info) and bytes(gsi) == bytes(sinfo) and name == "cornell-srgb" and text == "observer=1931\n"
    assert np.array_equal(bits64(gs), bits64(sums)) and (g2 is None) == (not with_s2) and (g2 is None or np.array_equal(bits64(g2), bits64(s2)))
    assert np.array_equal(bits64(gS), bits64(S)) and np.array_equal(gN, N)
    assert gQ.shape == (H, W, bins) and gQ.dtype == np.float64 and np.array_equal(bits64(gQ), bits64(Q))
    assert bits64(gQ)[0, 0, 2] == NAN_PAYLOAD and np.signbit(gQ[3, 5, 0]) and gQ[3, 5, 1] == np.inf
    # the older loaders read the same file's sums and bins and pass over what they do not return
    got, gs, g2, name, text, gsi, gS, gN = load_checkpoint_file_spectral(path)
    assert bytes(got) == bytes(info) and bytes(gsi) == bytes(sinfo) and np.array_equal(bits64(gS), bits64(S)) and np.array_equal(gN, N)
    got, gs, g2, name, text = load_checkpoint_file(path)
    assert bytes(got) == bytes(info) and np.array_equal(bits64(gs), bits64(sums)) and (g2 is None or np.array_equal(bits64(g2), bits64(s2)))
    # ... and the new loader reads the older files: no Q
    assert load_checkpoint_file_moments(older)[-1] is None


def test_without_q_the_file_is_todays(host, tmp_path):
    from simple_spectral_amd.renderer import load_checkpoint_file_moments
    sums, s2, S, N = base.synthetic(8)
    info, sinfo = sums_info(), spectral_info(8)
    a, b, c, d = (str(tmp_path / n) for n in ("a.ckpt", "b.ckpt", "c.ckpt", "d.ckpt"))
    assert base.save(host, a, info, sums, s2, sinfo, S, N) == 0 and save(host, b, info, sums, s2, sinfo, S, N) == 0
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read() and raw[:8] == b"SSXCKPT2"
    assert host.ssh_checkpoint_save(os.fsencode(c), C.byref(info), b"cornell-srgb", b"observer=1931\n", sums.ctypes.data, s2.ctypes.data) == 0
    assert save(host, d, info, sums, s2) == 0
    raw = open(c, "rb").read()
    assert raw == open(d, "rb").read() and raw[:8] == b"SSXCKPT1"
    *_, gsi, gS, gN, gQ = load_checkpoint_file_moments(c)
    assert gsi.bins == 0 and gS is None and gN is None and gQ is None


def test_save_refuses_q_without_bins(host, tmp_path):
    sums, s2, S, N = base.synthetic(8)
    path = str(tmp_path / "a.ckpt")
    assert save(host, path, sums_info(), sums, s2, None, None, None, synthetic_q(8)) == _capi.SSX_ERR_ARG
    assert b"q without" in host.ssh_last_error()
    assert save(host, path, sums_info(), sums, s2, spectral_info(8), S, None, synthetic_q(8)) == _capi.SSX_ERR_ARG
    assert not os.path.exists(path)


def test_damaged_moments_checkpoints_are_refused_as_bad_data(host, tmp_path):
    from simple_spectral_amd.renderer import SsxError, load_checkpoint_file, load_checkpoint_file_moments, load_checkpoint_file_spectral
    bins = 8
    sums, s2, S, N = base.synthetic(bins, 1)
    Q, sinfo = synthetic_q(bins, 1), spectral_info(bins)
    path, older = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    assert save(host, path, sums_info(), sums, s2, sinfo, S, N, Q) == 0 and base.save(host, older, sums_info(), sums, s2, sinfo, S, N) == 0
    raw, raw2 = open(path, "rb").read(), open(older, "rb").read()
    q_at = len(raw) - 8 - Q.nbytes                                  # where Q begins
    flip = lambda at, bit=0x10: raw[:at] + bytes([raw[at] ^ bit]) + raw[at + 1:]
    bad = {"a bit in the first byte of Q": flip(q_at, 0x01), "a bit inside Q": flip(q_at + Q.nbytes // 2 + 3), "a bit in the last byte of Q": flip(len(raw) - 9, 0x80),
           "cut at the start of Q": raw[:q_at], "cut inside Q": raw[:q_at + Q.nbytes // 2], "cut inside Q, the checksum kept": raw[:q_at + Q.nbytes // 2] + raw[-8:],
           "cut by one byte": raw[:-1], "one more byte": raw + b"\0",
           "the SSXCKPT2 magic on the longer file": b"SSXCKPT2" + raw[8:], "the SSXCKPT1 magic on the longer file": b"SSXCKPT1" + raw[8:],
           "the SSXCKPT3 magic on a file without Q": b"SSXCKPT3" + raw2[8:]}
    for what, data in bad.items():
        p = str(tmp_path / "bad.ckpt")
        open(p, "wb").write(data)
        for load in (load_checkpoint_file_moments, load_checkpoint_file_spectral, load_checkpoint_file):
            with pytest.raises(SsxError) as e:
                load(p)
            assert e.value.code == _capi.SSX_ERR_DATA, what


@pytest.mark.parametrize("bins", [4, 64])
def test_moments_merge_equals_the_ownership_rule(host, bins):
    """tile_stride 3, tile_skew 1: the rule restated with numpy, as for the bins (test_spectral_checkpoint_cpu.py)."""
    from simple_spectral_amd.renderer import merge_moments
    stride, skew = 3, 1
    Q = synthetic_q(bins, 2)
    tiles_x = (W + 7) // 8
    jj, ii = np.mgrid[0:H, 0:W]
    place = (jj // 8) * tiles_x + (ii // 8 + ((jj // 8) * (skew % tiles_x)) % tiles_x) % tiles_x
    dst = np.full((H, W, bins), 7.0)                                 # (every pixel has exactly one owner: nothing of this survives)
    for r in range(stride):
        mask = place % stride == r
        assert np.array_equal(mask, tile_owner_mask(W, H, r, stride, skew))
        part = np.where(mask[..., None], Q, 0.0)                     # a rank's export: zeros where it owns nothing
        before = dst.copy()
        merge_moments(dst, part, sums_info(tile_first=r, tile_stride=stride, tile_skew=skew))
        assert np.array_equal(bits64(dst)[~mask], bits64(before)[~mask])   # foreign pixels untouched
    assert np.array_equal(bits64(dst), bits64(Q))
    assert host.ssh_moments_merge(dst.ctypes.data, Q.ctypes.data, 6, C.byref(sums_info())) == _capi.SSX_ERR_ARG
    assert host.ssh_moments_merge(None, Q.ctypes.data, bins, C.byref(sums_info())) == _capi.SSX_ERR_ARG


# ---- the consistency check, restated ---------------------------------------------------------------------------------------------------------------------

RW, RH, SEED = 20, 12, 5


@functools.lru_cache(maxsize=None)
def oracle_samples(spp):
    """The CPU oracle's samples of cornell-srgb at 20 x 12: (flux float32 [H, W, spp, 4], lambda_0 float32 [H, W, spp]).  lambda_0 is the oracle's own draw of
    every sample's first hero wavelength (spectral_ref.project_flux restates it the same way), so the sub-bins fill as a render's do.  The oracle hands out no
    hero fluxes, only each sample's projected result: its four binary32 components stand in for the four fluxes -- misses are exact zeros, as a render's are."""
    o = ol.Oracle("cornell-srgb", texture="test-img.png")
    d = Scene("cornell-srgb", texture="test-img.png").desc.contents
    lmin, lstep = np.float32(d.lambda_min), np.float32(d.lambda_step)
    flux, _, _ = o.samples(RW, RH, spp, seed=SEED)
    lam, rng = np.zeros((RH, RW, spp), dtype=np.float32), ol.Rng()
    for j in range(RH):
        for i in range(RW):
            for k in range(spp):
                o.lib.orc_seed_sample(SEED, j * RW + i, k, C.byref(rng))
                o.lib.orc_rand_1d(C.byref(rng)); o.lib.orc_rand_1d(C.byref(rng))
                lam[j, i, k] = lmin + np.float32(o.lib.orc_rand_1f(C.byref(rng))) * lstep
    flux.setflags(write=False); lam.setflags(write=False)
    return flux, lam, lmin, lstep


@pytest.mark.parametrize("bins,spp", [(8, 3), (8, 12), (64, 5), (64, 24)])
def test_the_restated_check_accepts_what_the_moment_kernel_produces(bins, spp):
    flux, lam, lmin, lstep = oracle_samples(spp)
    S, Q, N = sref.restate_sums(flux, lam, lmin, lstep, bins)
    assert (N.sum(axis=2) == spp).all()
    if spp <= 5:                                                    # thin sub-bins: every branch of the check is taken
        n = np.tile(N, (1, 1, 4))
        assert (N == 0).any() and (N == 1).any() and (N >= 2).any() and ((n == 1) & (S != 0.0)).any()
    assert mref.broken_rule(S, Q, N) is None
    assert not any(v.any() for v in mref.violations(S, Q, N))


@pytest.mark.parametrize("bins", [8, 64])
def test_the_restated_check_rejects_each_rule_broken_in_one_element(bins):
    flux, lam, lmin, lstep = oracle_samples(5)
    S, Q, N = sref.restate_sums(flux, lam, lmin, lstep, bins)
    n = np.tile(N, (1, 1, 4))
    at0 = tuple(np.argwhere(n == 0)[-1])
    at1 = tuple(np.argwhere((n == 1) & (S * S != S))[-1])         # (a sum that is not its own square: neither a miss nor the stand-in's alpha of 1)
    at2 = tuple(np.argwhere(n >= 2)[-1])

    def edited(at, value):
        q = Q.copy()
        q[at] = value
        return q

    up = lambda x: np.nextafter(x, np.inf)
    for rule, q in ((0, edited(at0, -0.0)), (0, edited(at0, 5e-324)), (0, edited(at0, np.nan)),
                    (1, edited(at1, up(Q[at1]))), (1, edited(at1, 0.0)), (1, edited(at1, np.nan)), (1, edited(at1, S[at1])),
                    (2, edited(at2, -5e-324)), (2, edited(at2, -np.inf))):
        bad = mref.violations(S, q, N)
        assert mref.broken_rule(S, q, N) == rule and bad[rule][at0 if rule == 0 else at1 if rule == 1 else at2] and sum(int(b.sum()) for b in bad) == 1, (rule, q[at0], q[at1], q[at2])
        mask = np.ones((RH, RW), dtype=bool)
        mask[(at0, at1, at2)[rule][:2]] = False                     # a pixel the importing context does not own is not held to anything
        assert mref.broken_rule(S, q, N, mask) is None
    assert mref.broken_rule(S, edited(at2, np.nan), N) is None and mref.broken_rule(S, edited(at2, 0.0), N) is None    # n >= 2: only the sign is held
    # the mistakes the rules are there for: S handed in as Q; one rank's unmerged export (zeros where n > 0); another render's Q
    assert mref.broken_rule(S, S, N) is not None
    assert mref.broken_rule(S, np.zeros_like(Q), N) == 1
    other = sref.restate_sums(*oracle_samples(3)[:2], lmin, lstep, bins)[1]
    assert mref.broken_rule(S, other, N) is not None


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_cli_argument_rules_of_a_resume_with_the_moments(host, tmp_path):
    """What the CLI decides before it touches a device: a resume with an option that needs the second moments needs a checkpoint that holds them, for as many bins
    as are asked for.  The files are written through libssx_host.so from synthetic arrays."""
    sums, s2, S, N = base.synthetic(8)
    ck1, ck2, ck3 = (str(tmp_path / n) for n in ("sums.ckpt", "bins8.ckpt", "q8.ckpt"))
    assert save(host, ck1, sums_info(), sums, s2) == 0 and save(host, ck2, sums_info(), sums, s2, spectral_info(8), S, N) == 0
    assert save(host, ck3, sums_info(), sums, s2, spectral_info(8), S, N, synthetic_q(8)) == 0
    assert [open(p, "rb").read(8) for p in (ck1, ck2, ck3)] == [b"SSXCKPT1", b"SSXCKPT2", b"SSXCKPT3"]
    common = ["-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=16", "-o=" + str(tmp_path / "x.png")]
    run = lambda *a: subprocess.run([CLI] + common + list(a), cwd=ROOT, capture_output=True, text=True)
    options = {"--spectral-variance-output": ["--spectral-variance-output=" + str(tmp_path / "v.npy")],
               "--probe": ["--probe=0,0,4,4", "--probe-output=" + str(tmp_path / "p.csv")],
               "--spectral-noise-target": ["--spectral-noise-target=0.05", "--max-samples=32", "--spectral-noise-output=" + str(tmp_path / "n.csv")]}
    for flag, args in options.items():
        for ck, reason in ((ck2, "8 wavelength bins without their second moments"), (ck1, "the pixel sums only, no wavelength bins"),
                           (str(tmp_path / "missing.ckpt"), "cannot be read")):
            for given in ([], ["--spectral-bins=8"]):
                r = run("--resume=" + ck, *args, *given)
                assert r.returncode == 255 and "Simple Spectral" in r.stdout, (flag, ck, r.stderr)
                assert "`%s` cannot be combined with `--resume`" % flag in r.stderr and "does not carry the second moments" in r.stderr and reason in r.stderr, (flag, ck, r.stderr)
        r = run("--resume=" + ck3, *args, "--spectral-bins=16")
        assert r.returncode == 255 and "`%s` cannot be combined with `--resume`" % flag in r.stderr and "does not carry the second moments" in r.stderr, r.stderr
        assert "another bin count" in r.stderr and "holds 8" in r.stderr and "`--spectral-bins=16`" in r.stderr, r.stderr
    assert "`--resume` needs a checkpoint that holds them" in r.stdout   # the usage text says what is now true
    assert not any(os.path.exists(str(tmp_path / n)) for n in ("x.png", "v.npy", "p.csv", "n.csv"))
