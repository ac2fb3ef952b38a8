"""Comparing two spectral renders (include/ssx.h "Comparing two spectral renders"), the parts that need no GPU: the numpy restatement (tests/spectral_compare_ref.py)
against its own symmetries and against statistics, the hosts' derivation and CSV writer, the way a checkpoint becomes the call's arguments, the new names and the
CLI's refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spectral_compare_ref as ref
import test_moments_checkpoint_cpu as mbase
import test_spectral_checkpoint_cpu as base
from simple_spectral_amd import _capi, build as sbuild

ROOT, CLI = base.ROOT, base.CLI
W, H, B, SPP = 20, 12, 8, 32          # 20 x 12 x 8 cells, 32 samples per sub-bin
bits64 = base.bits64


@pytest.fixture(scope="module")
def host():
    sbuild.build_host()
    return _capi.host_lib()


def gaussian_render(seed, mean, sigma=2.0, spp=SPP, shape=(H, W, B)):
    """(S, Q float64 [H, W, B], N uint32 [H, W, M]) of spp binary32 Gaussian fluxes per cell, accumulated in ascending k as the kernels do"""
    f = np.random.RandomState(seed).normal(mean, sigma, shape + (spp,)).astype(np.float32).astype(np.float64)
    S, Q = np.zeros(shape), np.zeros(shape)
    for k in range(spp):
        S += f[..., k]; Q += f[..., k] * f[..., k]
    return S, Q, np.full(shape[:2] + (shape[2] // 4,), spp, dtype=np.uint32)


def whole(): return np.zeros((H, W), dtype=np.uint8)


def same_bits(a, b): return a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.itemsize == 8 else np.uint32), b.view(np.uint64 if b.itemsize == 8 else np.uint32))


def test_new_names_exist(host):
    for s in ("ssx_spectral_compare", "ssx_spectral_compare_arrays"):
        assert s in _capi.HIP_SYMBOLS, s
    for s in ("ssh_compare_derive", "ssh_compare_save_csv"):
        assert s in _capi.HOST_SYMBOLS and hasattr(host, s), s
    header = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "Comparing two spectral renders" in header and "int ssx_spectral_compare_arrays(ssx_ctx* ctx, uint32_t width, uint32_t height, uint32_t bins, const double* SA" in header
    assert "int ssx_spectral_compare(ssx_ctx* ctx, const ssx_spectral_info_t* other_info, const double* SB" in header
    host_header = open(os.path.join(ROOT, "include", "ssx_host.h")).read()
    assert "int ssh_compare_derive(" in host_header and "int ssh_compare_save_csv(" in host_header
    sbuild.build_all()
    exported = subprocess.run(["nm", "-D", "--defined-only", sbuild.HIP_LIB], capture_output=True, text=True, check=True).stdout
    assert " T ssx_spectral_compare\n" in exported and " T ssx_spectral_compare_arrays\n" in exported
    kernels = subprocess.check_output(["strings", sbuild.HIP_LIB], text=True)
    for k in ("ssx_compare_rows_kernel", "ssx_compare_rows_wide_kernel", "ssx_ordered_reduce_kernel"):     # (stage 2 is shared with the probes)
        assert k in kernels, k
    cxx = subprocess.check_output(["nm", "-DC", "--defined-only", sbuild.HOST_LIB], text=True)
    assert "ssx::Renderer::compare_spectral(" in cxx and "ssx::compare_derive(" in cxx and "ssx::save_compare_csv(" in cxx
    from simple_spectral_amd import Renderer
    from simple_spectral_amd import renderer as rmod
    for m in ("compare_spectral_raw", "compare_spectral", "compare_arrays"):
        assert callable(getattr(Renderer, m)), m
    assert callable(rmod.compare_derive) and callable(rmod.save_compare_csv)


def test_a_render_against_itself():
    S, Q, N = gaussian_render(1, 10.0)
    N = N.copy(); N[2, 3, 0] = 1; N[4, 5, 1] = 0                      # two thin sub-bins: four cells that are not comparable
    S[0, 0, 0] = Q[0, 0, 0] = 0.0                                     # a black cell: v == 0 and d == 0
    S[1, 1, 1], Q[1, 1, 1] = 4.0 * SPP, 16.0 * SPP                    # a constant cell: v == 0 and d == 0, not black
    DD, VV, X2, CC, NC, EX = ref.compare(S, Q, N, S, Q, N, whole(), 1, 9.0)
    assert not bits64(DD).any() and not bits64(X2).any() and not EX.any()          # +0.0, bit for bit
    want = (np.tile(N, (1, 1, 4)) >= 2).sum(axis=(0, 1), dtype=np.uint64)
    assert np.array_equal(CC[0], want) and np.array_equal(NC[0], np.uint64(W * H) - want) and NC.sum() == 8
    diff, var = ref.maps(S, Q, N, S, Q, N)
    assert not diff.view(np.uint32).any() and np.isposinf(var).sum() == 8 and var[0, 0, 0] == 0 and var[1, 1, 1] == 0


def test_swapping_the_renders_negates_the_difference_only():
    A, Bset = gaussian_render(2, 10.0), gaussian_render(3, 10.5, spp=21)
    NA = A[2].copy(); NA[6, 7, 1] = 1
    A = (A[0], A[1], NA)
    labels = whole().copy(); labels[:, 10:] = 1; labels[0, 0] = 255
    ab, ba = ref.compare(*A, *Bset, labels, 2, 9.0), ref.compare(*Bset, *A, labels, 2, 9.0)
    assert (ab[0] != 0).all() and same_bits(-ab[0], ba[0])                         # DD: every bit but the sign
    for k, name in zip(range(1, 6), ("VV", "X2", "CC", "NC", "EX")):
        assert same_bits(ab[k], ba[k]), name
    (d_ab, v_ab), (d_ba, v_ba) = ref.maps(*A, *Bset), ref.maps(*Bset, *A)
    zero = d_ab == 0
    assert zero.sum() == 4 and not d_ab[zero].view(np.uint32).any() and not d_ba[zero].view(np.uint32).any()      # zeros stay +0.0
    assert same_bits(-d_ab[~zero], d_ba[~zero]) and same_bits(v_ab, v_ba)


def test_chi2_is_calibrated_on_gaussian_fluxes():
    """Equal means, equal sigma and equal n = 32 on both sides: with equal n Welch's statistic is the pooled two-sample t, so z2 = t^2 with nu = 2 n - 2 = 62 degrees of
    freedom EXACTLY (for Gaussian draws; the rounding of the fluxes to binary32 moves nothing visible).  E[t^2] = nu / (nu - 2) = 62 / 60 = 1.0333, E[t^4] = 3 nu^2 /
    ((nu - 2)(nu - 4)) = 3.3138, so Var[t^2] = 3.3138 - 1.0678 = 2.2460.  The cells are independent: the mean of 20 x 12 x 8 = 1920 of them has a standard deviation of
    sqrt(2.2460 / 1920) = 0.0342, the mean of one bin's 240 cells 0.0967.  The bands are five standard deviations: 1.0333 +- 0.171 for all cells, +- 0.484 per bin
    (one run in 1.7 million leaves a 5-sigma band; the seed is fixed)."""
    A, Bset = gaussian_render(10, 10.0), gaussian_render(11, 10.0)
    sums = ref.compare(*A, *Bset, whole(), 1, 9.0)
    DD, VV, X2, CC, NC, EX = sums
    assert (CC == W * H).all() and not NC.any()
    nu = 2.0 * SPP - 2.0
    expect, var_t2 = nu / (nu - 2.0), 3.0 * nu * nu / ((nu - 2.0) * (nu - 4.0)) - (nu / (nu - 2.0)) ** 2
    chi2 = ref.derive(*sums)["chi2"][0]
    pooled = X2.sum() / CC.sum()
    print("chi2 pooled %.4f (expect %.4f +- %.4f), per bin %s" % (pooled, expect, 5 * np.sqrt(var_t2 / CC.sum()), np.round(chi2, 3)))
    assert abs(pooled - expect) <= 5.0 * np.sqrt(var_t2 / CC.sum())
    assert (np.abs(chi2 - expect) <= 5.0 * np.sqrt(var_t2 / (W * H))).all()
    # B's mean shifted by five standard errors of d: z is near 5, and most cells lie beyond Z = 3
    shift = 5.0 * np.sqrt(2.0 * 2.0 ** 2 / SPP)
    shifted = ref.derive(*ref.compare(*A, *gaussian_render(11, 10.0 + shift), whole(), 1, 9.0))
    print("exceed at a shift of 5 standard errors: %s" % np.round(shifted["exceed"][0], 3))
    assert (shifted["exceed"] > 0.5).all() and (shifted["mean_diff"] < 0).all() and (shifted["z"] < -3).all()


def test_the_hosts_derivation_is_the_restatements(host):
    from simple_spectral_amd.renderer import compare_derive
    A, Bset = gaussian_render(4, 10.0), gaussian_render(5, 10.2, spp=21)
    labels = whole().copy(); labels[:, 10:] = 1                                    # region 2 stays empty
    sums = [a.copy() for a in ref.compare(*A, *Bset, labels, 3, 1.0)]
    sums[1][1, 0] = 0.0                                                            # VV == 0 with CC > 0: z has no denominator
    sums[3][1, 1], sums[4][1, 1] = 0, 7                                            # CC == 0 with NC > 0: coverage 0, the rest NaN
    sums[0][0, 2] = np.nan
    got, want = compare_derive(*sums), ref.derive(*sums)
    assert set(got) == set(want) == {"mean_diff", "stderr", "z", "chi2", "exceed", "coverage"}
    for k in want:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(bits64(got[k])[~np.isnan(want[k])], bits64(want[k])[~np.isnan(want[k])]), k
        assert np.isnan(got[k][2]).all(), k                                        # the empty region: every figure NaN
    assert np.isnan(got["z"][1, 0]) and got["stderr"][1, 0] == 0 and np.isfinite(got["mean_diff"][1, 0])
    assert got["coverage"][1, 1] == 0 and all(np.isnan(got[k][1, 1]) for k in ("mean_diff", "stderr", "chi2", "exceed"))
    assert np.isnan(got["mean_diff"][0, 2]) and np.isnan(got["z"][0, 2]) and np.isfinite(got["chi2"][0, 2])
    assert host.ssh_compare_derive(1, 4, None, None, None, None, None, None, None, None, None, None, None, None) == _capi.SSX_ERR_ARG


def test_the_csv_writer(tmp_path):
    from simple_spectral_amd.renderer import compare_derive, save_compare_csv
    A, Bset = gaussian_render(6, 10.0), gaussian_render(7, 10.2)
    labels = whole().copy(); labels[:, 10:] = 1
    sums = [a.copy() for a in ref.compare(*A, *Bset, labels, 3, 9.0)]
    sums[2][0, 1] = np.inf
    path = str(tmp_path / "c.csv")
    save_compare_csv(path, 360.0, 58.75, *sums)
    fig = compare_derive(*sums)
    lines = open(path).read().split("\n")
    assert lines[0] == "region,bin,wavelength,mean_diff,stderr,z,chi2,exceed,comparable,not_comparable" and len(lines) == 2 + 3 * B and lines[-1] == ""
    for k, line in enumerate(lines[1:-1]):
        f = line.split(",")
        r, b = divmod(k, B)
        assert (int(f[0]), int(f[1]), int(f[8]), int(f[9])) == (r, b, int(sums[3][r, b]), int(sums[4][r, b]))
        assert np.float32(f[2]) == np.float32(360.0) + (np.float32(b) + np.float32(0.5)) * np.float32(58.75)
        for col, name in zip(range(3, 8), ("mean_diff", "stderr", "z", "chi2", "exceed")):
            v = fig[name][r, b]
            assert (f[col] == "nan") if np.isnan(v) else (float(f[col]) == v), (name, r, b)
    assert lines[1 + 1].split(",")[6] == "inf" and all(f == "nan" for f in lines[1 + 2 * B].split(",")[3:8])


def test_a_checkpoint_becomes_the_calls_arguments(host, tmp_path):
    from simple_spectral_amd.renderer import compare_other, load_checkpoint_file_moments
    sums, s2, S, N = base.synthetic(8)
    Q = mbase.synthetic_q(8)
    with_q, without = str(tmp_path / "q.ckpt"), str(tmp_path / "bins.ckpt")
    assert mbase.save(host, with_q, base.sums_info(), sums, s2, base.spectral_info(8), S, N, Q) == 0
    assert mbase.save(host, without, base.sums_info(), sums, s2, base.spectral_info(8), S, N) == 0
    info, gS, gQ, gN = compare_other(load_checkpoint_file_moments(with_q))
    assert (info.width, info.height, info.bins) == (base.W, base.H, 8) and info.struct_size == C.sizeof(_capi.SsxSpectralInfo)
    assert np.array_equal(bits64(gS), bits64(S)) and np.array_equal(bits64(gQ), bits64(Q)) and np.array_equal(gN, N) and gN.dtype == np.uint32
    assert all(a.flags.c_contiguous for a in (gS, gQ, gN))
    info2, *_ = compare_other((info, S, N, Q))                                     # the four values are taken as they are
    assert info2 is info
    with pytest.raises(ValueError, match="second moments"):
        compare_other(load_checkpoint_file_moments(without))
    with pytest.raises(ValueError, match="shape"):
        compare_other((info, S[:, :, :4], N, Q))


def test_cli_refusals(host, tmp_path):
    """What the CLI decides when it checks its options, before it touches a device.  (lambda_min and bin_width need the scene and are checked on the GPU.)"""
    assert os.path.exists(CLI)
    sums, s2, S, N = base.synthetic(8)
    Q = mbase.synthetic_q(8)
    ck1, ck2, ck3 = (str(tmp_path / n) for n in ("sums.ckpt", "bins8.ckpt", "q8.ckpt"))
    assert mbase.save(host, ck1, base.sums_info(), sums, s2) == 0 and mbase.save(host, ck2, base.sums_info(), sums, s2, base.spectral_info(8), S, N) == 0
    assert mbase.save(host, ck3, base.sums_info(), sums, s2, base.spectral_info(8), S, N, Q) == 0
    outs = [str(tmp_path / n) for n in ("x.png", "c.csv", "z.npy")]
    size = ["-w=%d" % base.W, "-h=%d" % base.H]
    tail = ["-spp=16", "-o=" + outs[0], "--compare-output=" + outs[1], "--compare-map-output=" + outs[2]]
    run = lambda *a: subprocess.run([CLI, "-s=cornell-srgb"] + tail + list(a), cwd=ROOT, capture_output=True, text=True)
    cases = [(size + ["--compare-to=" + ck2, "--spectral-bins=8"], ["cannot compare with", "8 wavelength bins without their second moments Q"]),
             (size + ["--compare-to=" + ck1, "--spectral-bins=8"], ["cannot compare with", "no wavelength bins and no second moments Q"]),
             (size + ["--compare-to=" + str(tmp_path / "missing.ckpt"), "--spectral-bins=8"], ["cannot compare with", "cannot be read"]),
             (["-w=%d" % (base.W + 1), "-h=%d" % base.H, "--compare-to=" + ck3, "--spectral-bins=8"], ["the size differs", "%u x %u" % (base.W, base.H)]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=16"], ["the bin count differs", "holds 8", "`--spectral-bins=16`"]),
             (size + ["--compare-to=" + ck3], ["`--compare-to` needs `--spectral-bins=<n>`"]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=8", "--tile-major"], ["`--compare-to` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`"]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=8", "--rgb"], ["`--compare-to` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`"]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=8", "--libm=glibc-2.35"], ["`--compare-to` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`"]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=8", "--compare-threshold=-1"], ["Invalid value for --compare-threshold"]),
             (size + ["--compare-to=" + ck3, "--spectral-bins=8", "--compare-threshold=inf"], ["Invalid value for --compare-threshold"]),
             (size + ["--spectral-bins=8"], ["`--compare-output` and `--compare-map-output` need `--compare-to=<file.ckpt>`"])]
    for args, reasons in cases:
        r = run(*args)
        assert r.returncode == 255 and "Simple Spectral" in r.stdout, (args, r.stderr)
        for reason in reasons:
            assert reason in r.stderr, (args, reason, r.stderr)
        assert "same seed" not in r.stderr
    assert "`--compare-to=<file.ckpt>`" in r.stdout and "`--compare-threshold=<z>`" in r.stdout       # the usage names the options
    # --probe-output without --probe is still refused; --probe alone is --compare-to's regions and passes the option check (here: on to the same-seed warning)
    r = run(*size, "--compare-to=" + ck3, "--spectral-bins=8", "--probe-output=" + str(tmp_path / "p.csv"))
    assert r.returncode == 255 and "need each other" in r.stderr
    assert not any(os.path.exists(p) for p in outs)
