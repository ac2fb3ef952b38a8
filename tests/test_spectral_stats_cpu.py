"""Spectral moments and region probes without a GPU (include/ssx.h "Spectral moments and region probes"): the symbols, the numpy restatement of the definitions
held against statistics and against np.var, the +inf and NaN rules, the CLI's refusals and the CSV writer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spectral_stats_ref as ref
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd import renderer as rmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
LMIN, LSTEP = np.float32(380.0), np.float32(100.0)


def ulps32(a, b):
    """distance in binary32 ulps between two arrays of positive finite floats"""
    return np.abs(np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64))


def synthetic(rng, H, W, spp, mean=1.0, sigma=0.5):
    """Gaussian hero fluxes float32 [H, W, spp, 4] and uniform lambda_0 float32 [H, W, spp] in [LMIN, LMIN + LSTEP)"""
    flux = rng.normal(mean, sigma, size=(H, W, spp, 4)).astype(np.float32)
    lam = (LMIN + np.float32(0.999) * LSTEP * rng.random(size=(H, W, spp), dtype=np.float32)).astype(np.float32)
    return flux, lam


def test_new_symbols_exist_in_both_libraries(tmp_path):
    sbuild.build_all()
    hip, host = C.CDLL(sbuild.HIP_LIB), C.CDLL(sbuild.HOST_LIB)   # load without a GPU; no compute call is made
    for s in ("ssx_set_spectral_moments", "ssx_spectral_variance", "ssx_spectral_probe", "ssx_probe_arrays"):
        assert s in _capi.HIP_SYMBOLS
        getattr(hip, s)
    for s in ("ssh_probe_derive", "ssh_probe_save_csv"):
        assert s in _capi.HOST_SYMBOLS
        getattr(host, s)
    src = ('#include "ssx_host.h"\n'
           'int (*a)(ssx_ctx*, int) = ssx_set_spectral_moments;\n'
           'int (*b)(ssx_ctx*, ssx_spectral_info_t*, float*, double*) = ssx_spectral_variance;\n'
           'int (*c)(ssx_ctx*, const uint8_t*, uint32_t, double*, uint64_t*, double*, uint64_t*) = ssx_spectral_probe;\n'
           'int (*d)(ssx_ctx*, uint32_t, uint32_t, uint32_t, const double*, const double*, const uint32_t*, const uint8_t*, uint32_t, double*, uint64_t*, double*, uint64_t*) = ssx_probe_arrays;\n'
           'int (*e)(const char*, uint32_t, uint32_t, float, float, const double*, const uint64_t*, const double*, const uint64_t*) = ssh_probe_save_csv;\n')
    open(tmp_path / "t.c", "w").write(src)
    subprocess.check_call(["gcc", "-c", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t.o")])   # the declarations are C
    from simple_spectral_amd import Renderer
    for m in ("set_spectral_moments", "spectral_variance", "probe", "probe_raw", "probe_arrays"):
        assert callable(getattr(Renderer, m))
    names = subprocess.check_output(["nm", "-D", "--defined-only", sbuild.HOST_LIB], text=True)   # the C++ host's methods
    for sym in ("_ZN3ssx8Renderer20set_spectral_momentsEb", "_ZN3ssx8Renderer17spectral_varianceEv", "_ZN3ssx8Renderer5probeE"):
        assert sym in names, sym
    text = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "Q[p][i*M + m] += (double)f[i] * (double)f[i]" in text and "stderr = sqrt(VV * NN / (NN - UU)) / NN" in text


def test_the_pooled_standard_error_predicts_the_spread_of_the_pooled_mean():
    """R independent replicates of a 4 x 3 region at M = 2 and 64 spp (about 32 samples per sub-bin: none holds fewer than 2, which the test asserts).  The mean
    over the replicates of VV / NN^2 estimates the variance of the pooled mean SS / NN; the empirical variance of the pooled mean over the replicates measures it.
    For Gaussian data the empirical variance of R values has relative standard deviation sqrt(2 / (R - 1)), and the numerator -- an average of R * 12 * 32 squared
    deviations -- adds a few percent of that, so sd(ratio) ~ sqrt(2 / (R - 1)).  R = 1601 is chosen for sd = 0.0354: the ratio must be 1 within 4 sd = 0.1414,
    which a factor-of-n or ddof mistake (ratios of 1/32, 32, or 1 +- 1/32 ... the last one is not resolved, and test 3 holds it) cannot meet."""
    R, h, w, spp, bins = 1601, 3, 4, 64, 8
    rng = np.random.default_rng(20240607)
    flux, lam = synthetic(rng, R * h, w, spp)
    S, Q, N = ref.restate_sums(flux, lam, LMIN, LSTEP, bins)
    assert (N >= 2).all()
    labels = np.zeros((h, w), dtype=np.uint8)
    pooled, predicted = np.zeros((R, bins)), np.zeros((R, bins))
    for k in range(R):
        rows = slice(k * h, (k + 1) * h)
        SS, NN, VV, UU = ref.probe(S[rows], Q[rows], N[rows], labels, 1)
        assert not UU.any() and (NN[0, :2] == np.uint64(0) + N[rows].sum(axis=(0, 1))).all()
        mean, err = ref.derive(SS, NN, VV, UU)
        pooled[k], predicted[k] = mean[0], VV[0] / NN[0].astype(np.float64) ** 2
        assert np.allclose(err[0] ** 2, predicted[k], rtol=1e-12)   # with UU = 0 the standard error is sqrt(VV) / NN
    ratio = predicted.mean(axis=0) / pooled.var(axis=0, ddof=1)
    bound = 4.0 * np.sqrt(2.0 / (R - 1))
    print("ratio per bin", ratio, "bound", bound)
    assert (np.abs(ratio - 1.0) <= bound).all(), (ratio, bound)


def test_the_variance_is_the_sample_variance_of_the_sub_bin_over_n():
    """var[p][b] against np.var(ddof=1) / n of the samples that fell into the sub-bin.  With mean 1 and sigma 0.5, Q / q is about 5: the cancellation in
    Q - S*S/n loses three bits of binary64, far below the rounding to binary32 -- so the two agree to 1 ulp of binary32 (2 allowed: each side rounds once)."""
    bins, spp = 8, 40
    M = bins // 4
    rng = np.random.default_rng(7)
    flux, lam = synthetic(rng, 5, 6, spp)
    S, Q, N = ref.restate_sums(flux, lam, LMIN, LSTEP, bins)
    var = ref.variance(S, Q, N)
    m = rmod.spectral_bin_index(lam, LMIN, LSTEP, bins)
    assert (N >= 2).all()
    for j, i in np.ndindex(5, 6):
        for b in range(bins):
            x = flux[j, i, m[j, i] == b % M, b // M].astype(np.float64)
            assert x.size == N[j, i, b % M]
            want = np.float32(np.var(x, ddof=1) / x.size)
            assert ulps32(var[j, i, b], want) <= 2, (j, i, b, var[j, i, b], want)


def test_thin_sub_bins_are_unknown_and_a_nan_stays_a_nan():
    bins, M = 8, 2
    flux = np.ones((1, 3, 5, 4), dtype=np.float32) * np.arange(1, 6, dtype=np.float32)[None, None, :, None]
    lam = np.full((1, 3, 5), LMIN, dtype=np.float32)                                  # pixel 0: all five samples in m = 0, none in m = 1
    lam[0, 1, 4] = LMIN + np.float32(0.75) * LSTEP                                    # pixel 1: four in m = 0, ONE in m = 1
    flux[0, 2, 2, 1] = np.nan                                                         # pixel 2: a NaN flux in hero slot 1
    S, Q, N = ref.restate_sums(flux, lam, LMIN, LSTEP, bins)
    var = ref.variance(S, Q, N)
    inf = np.float32(np.inf)
    assert (var[0, 0, 1::M] == inf).all() and (var[0, 1, 1::M] == inf).all()          # n = 0 and n = 1: unknown, not zero
    assert np.array_equal(var[0, 0, 0::M], np.full(4, np.float32(2.5 / 5.0)))         # 1..5: sample variance 2.5, over n = 5
    assert np.isnan(var[0, 2, 1 * M]) and np.isnan(Q[0, 2, 1 * M]) and np.isfinite(np.delete(var[0, 2, 0::M], 1)).all()
    labels = np.array([[0, 0, 1]], dtype=np.uint8)
    SS, NN, VV, UU = ref.probe(S, Q, N, labels, 3)                                    # region 2 is empty
    assert NN[0].tolist() == [9, 1] * 4 and UU[0].tolist() == [0, 1] * 4 and UU[1].tolist() == [0, 0] * 4
    assert np.isnan(VV[1, M]) and np.isnan(SS[1, M]) and not np.isnan(VV[0]).any()
    assert not NN[2].any() and not SS[2].any() and not np.signbit(SS[2]).any()
    mean, err = ref.derive(SS, NN, VV, UU)
    assert (mean[2] == 0).all() and np.isnan(err[2]).all()                            # an empty region: mean 0, no error bar
    assert np.isnan(err[0, 1]) and err[0, 0] > 0                                      # one sample, unestimated: NN - UU == 0
    host_mean, host_err = rmod.probe_derive(SS, NN, VV, UU)                            # the hosts' derivation is the restatement's, bit for bit
    assert np.array_equal(host_mean.view(np.uint64)[~np.isnan(mean)], mean.view(np.uint64)[~np.isnan(mean)]) and np.array_equal(np.isnan(host_mean), np.isnan(mean))
    assert np.array_equal(host_err.view(np.uint64)[~np.isnan(err)], err.view(np.uint64)[~np.isnan(err)]) and np.array_equal(np.isnan(host_err), np.isnan(err))


@pytest.fixture(scope="module")
def cli():
    sbuild.build_host()
    assert os.path.exists(CLI)
    return CLI


def test_cli_refusals(cli, tmp_path):
    base = [cli, "-s=cornell-srgb", "-w=20", "-h=12", "-spp=4", "-o=" + str(tmp_path / "o.png"), "--texture=data/scenes/test-img.png"]
    var, csv = "--spectral-variance-output=" + str(tmp_path / "v.npy"), "--probe-output=" + str(tmp_path / "p.csv")

    def refused(args, *words):
        p = subprocess.run(base + args, cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 255 and "Simple Spectral" in p.stdout, (args, p.stderr)
        for w in words:
            assert w in p.stderr, (args, p.stderr)

    refused([var], "`--spectral-variance-output` needs `--spectral-bins=<n>`")
    refused(["--probe=0,0,4,4", csv], "`--probe` needs `--spectral-bins=<n>`")
    refused(["--spectral-bins=8", "--probe=0,0,4,4"], "need each other")
    refused(["--spectral-bins=8", csv], "need each other")
    refused(["--spectral-bins=8", csv] + ["--probe=0,0,1,1"] * 33, "32 times at most")
    refused(["--spectral-bins=8", csv, "--probe=4,0,4,4"], "`--probe=4,0,4,4` is empty or leaves the image")
    refused(["--spectral-bins=8", csv, "--probe=0,5,4,3"], "is empty or leaves the image")
    refused(["--spectral-bins=8", csv, "--probe=0,0,21,4"], "is empty or leaves the image")
    refused(["--spectral-bins=8", csv, "--probe=0,0,4,13"], "is empty or leaves the image")
    refused(["--spectral-bins=8", csv, "--probe=0,0,4"], "Invalid value for --probe")
    refused(["--spectral-bins=8", csv, "--probe=0,0,4,x"], "Invalid value for --probe")
    refused(["--spectral-bins=8", csv, "--probe=-1,0,4,4"], "Invalid value for --probe")
    for args in ([var], ["--probe=0,0,4,4", csv]):
        refused(["--spectral-bins=8", "--resume=" + str(tmp_path / "c.ckpt")] + args, "cannot be combined with `--resume`", "does not carry the second moments")
        refused(["--spectral-bins=8", "--tile-major"] + args, "cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`")
        refused(["--spectral-bins=8", "--rgb"] + args, "cannot be combined with")
        refused(["--spectral-bins=8", "--libm=glibc-2.35"] + args, "cannot be combined with")


def test_the_csv_writer(tmp_path):
    SS = np.array([[1.5, 0.1, -3.0, 7.0], [0.0, 0.0, 0.0, 0.0]])
    NN = np.array([[3, 4, 3, 4], [0, 1, 0, 1]], dtype=np.uint64)
    VV = np.array([[0.75, 1.0 / 3.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    UU = np.array([[0, 1, 0, 1], [0, 1, 0, 1]], dtype=np.uint64)
    path = str(tmp_path / "p.csv")
    lmin, width = np.float32(380.0), np.float32(100.0 / 3.0)
    rmod.save_probe_csv(path, lmin, width, SS, NN, VV, UU)
    lines = open(path).read().split("\n")
    assert lines[0] == "region,bin,wavelength,mean,stderr,samples,unestimated" and lines[-1] == "" and len(lines) == 2 + 2 * 4
    mean, err = ref.derive(SS, NN, VV, UU)
    for r in range(2):
        for b in range(4):
            f = lines[1 + r * 4 + b].split(",")
            assert len(f) == 7 and (int(f[0]), int(f[1]), int(f[5]), int(f[6])) == (r, b, int(NN[r, b]), int(UU[r, b]))
            assert np.float32(f[2]) == lmin + (np.float32(b) + np.float32(0.5)) * width                 # %.9g reads back to the same binary32
            for text, want in ((f[3], mean[r, b]), (f[4], err[r, b])):
                assert (text == "nan") if np.isnan(want) else (float(text) == want), (text, want)       # %.17g reads back to the same binary64
    assert lines[1 + 4 + 0].split(",")[3:5] == ["0", "nan"] and lines[1 + 4 + 1].split(",")[4] == "nan"   # nothing counted; one sample, unestimated
    with pytest.raises(rmod.SsxError):
        rmod.save_probe_csv(str(tmp_path / "no" / "dir.csv"), lmin, width, SS, NN, VV, UU)
