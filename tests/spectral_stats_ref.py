"""include/ssx.h "Spectral moments and region probes" restated in numpy: binary64, IEEE + - * / only, every operation in the order the header writes it, so that
the device's results are compared with these bit for bit.  TEST INFRASTRUCTURE, shared by tests/test_spectral_stats_cpu.py and tests/test_spectral_stats_gpu.py."""
import numpy as np

from simple_spectral_amd.renderer import spectral_bin_index

NO_REGION = 255


def restate_sums(flux, lam, lambda_min, lambda_step, bins):
    """(S float64 [H, W, B], Q float64 [H, W, B], N uint32 [H, W, M]) from the per-sample flux [H, W, spp, 4] (float32) and lambda_0 [H, W, spp], sequentially:
    in ascending k, S[i*M + m] += (double)f[i] and Q[i*M + m] += (double)f[i] * (double)f[i]."""
    H, W, spp = lam.shape
    M = bins // 4
    m = spectral_bin_index(lam, lambda_min, lambda_step, bins)
    S, Q, N = np.zeros((H, W, bins)), np.zeros((H, W, bins)), np.zeros((H, W, M), dtype=np.uint32)
    J, I = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(spp):                       # ascending k; every pixel appears once per statement
            for i in range(4):
                f = flux[:, :, k, i].astype(np.float64)
                S[J, I, i * M + m[:, :, k]] += f
                Q[J, I, i * M + m[:, :, k]] += f * f
            N[J, I, m[:, :, k]] += np.uint32(1)
    return S, Q, N


def deviations(S, Q, n):
    """q of the header where n >= 2 (elsewhere the value is not used): q = Q - (S*S) / (double)n; q = (q < 0.0) ? 0.0 : q -- a NaN stays a NaN."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = Q - (S * S) / n.astype(np.float64)
        return np.where(q < 0.0, 0.0, q)


def variance(S, Q, N):
    """var float32 [H, W, B]: n = N[b % M]; n < 2: +inf; else (float)((q / (double)(n-1)) / (double)n)."""
    n = np.tile(N, (1, 1, 4))
    q = deviations(S, Q, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = ((q / (n.astype(np.float64) - 1.0)) / n.astype(np.float64)).astype(np.float32)
    return np.where(n < 2, np.float32(np.inf), v).astype(np.float32)


def probe(S, Q, N, labels, regions):
    """(SS float64, NN uint64, VV float64, UU uint64), each [R, B]: within a row the pixels are added in ascending i starting from +0.0, the row partials in
    ascending j starting from +0.0; a row without a pixel of the region contributes its +0.0."""
    H, W, B = S.shape
    n_all = np.tile(N, (1, 1, 4))
    q_all = deviations(S, Q, n_all)
    SS, VV = np.zeros((regions, B)), np.zeros((regions, B))
    NN, UU = np.zeros((regions, B), dtype=np.uint64), np.zeros((regions, B), dtype=np.uint64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(H):
            ss, vv = np.zeros((regions, B)), np.zeros((regions, B))
            nn, uu = np.zeros((regions, B), dtype=np.uint64), np.zeros((regions, B), dtype=np.uint64)
            for i in range(W):
                r = int(labels[j, i])
                if r == NO_REGION:
                    continue
                assert r < regions
                n = n_all[j, i]
                est = n >= 2
                nf = n.astype(np.float64)
                ss[r] += S[j, i]
                nn[r] += n.astype(np.uint64)
                vv[r, est] += ((q_all[j, i] / (nf - 1.0)) * nf)[est]
                uu[r, ~est] += n.astype(np.uint64)[~est]
            SS += ss; VV += vv; NN += nn; UU += uu
    return SS, NN, VV, UU


def derive(SS, NN, VV, UU):
    """(mean, stderr) float64: mean = NN ? SS / NN : 0; stderr = sqrt(VV * NN / (NN - UU)) / NN, NaN when NN - UU == 0."""
    n = NN.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = np.where(NN > 0, SS / n, 0.0)
        err = np.sqrt(VV * n / (NN - UU).astype(np.float64)) / n
    return mean, err
