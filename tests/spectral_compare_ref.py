"""include/ssx.h "Comparing two spectral renders" restated in numpy: binary64, IEEE + - * / only, every operation in the order the header writes it, so that the
device's results are compared with these bit for bit.  TEST INFRASTRUCTURE, shared by tests/test_spectral_compare_cpu.py and tests/test_spectral_compare_gpu.py."""
import numpy as np

from spectral_stats_ref import deviations

NO_REGION = 255


def cells(SA, QA, NA, SB, QB, NB):
    """(comparable bool, d, v, z2 float64), each [H, W, B]; d, v and z2 are +0.0 where the cell is not comparable.
    eX = (qX / (double)(nX-1)) / (double)nX;  muX = S_X / (double)nX;  d = muA - muB;  v = eA + eB;  z2 = (v == 0.0 && d == 0.0) ? 0.0 : (d * d) / v."""
    nA, nB = np.tile(NA, (1, 1, 4)), np.tile(NB, (1, 1, 4))
    comparable = (nA >= 2) & (nB >= 2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        fA, fB = nA.astype(np.float64), nB.astype(np.float64)
        eA, muA = (deviations(SA, QA, nA) / (fA - 1.0)) / fA, SA / fA
        eB, muB = (deviations(SB, QB, nB) / (fB - 1.0)) / fB, SB / fB
        d = muA - muB
        v = eA + eB
        z2 = np.where((v == 0.0) & (d == 0.0), 0.0, (d * d) / v)
    return comparable, np.where(comparable, d, 0.0), np.where(comparable, v, 0.0), np.where(comparable, z2, 0.0)


def maps(SA, QA, NA, SB, QB, NB):
    """(diff, var) float32 [H, W, B]: (float)d and (float)v of a comparable cell, 0.0f and +inf otherwise."""
    comparable, d, v, _ = cells(SA, QA, NA, SB, QB, NB)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (np.where(comparable, d.astype(np.float32), np.float32(0.0)).astype(np.float32),
                np.where(comparable, v.astype(np.float32), np.float32(np.inf)).astype(np.float32))


def compare(SA, QA, NA, SB, QB, NB, labels, regions, t2):
    """(DD, VV, X2 float64, CC, NC, EX uint64), each [R, B]: the sums over the comparable cells of every region; within a row the pixels are added in ascending i
    starting from +0.0, the row partials in ascending j starting from +0.0; a row without a pixel of the region contributes its +0.0.  EX counts z2 > t2, strictly."""
    H, W, B = SA.shape
    comparable, d, v, z2 = cells(SA, QA, NA, SB, QB, NB)
    with np.errstate(invalid="ignore"):
        beyond = comparable & (z2 > t2)
    DD, VV, X2 = np.zeros((regions, B)), np.zeros((regions, B)), np.zeros((regions, B))
    CC, NC, EX = (np.zeros((regions, B), dtype=np.uint64) for _ in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(H):
            dd, vv, x2 = np.zeros((regions, B)), np.zeros((regions, B)), np.zeros((regions, B))
            for i in range(W):
                r = int(labels[j, i])
                if r == NO_REGION:
                    continue
                assert r < regions
                c = comparable[j, i]
                dd[r, c] += d[j, i][c]; vv[r, c] += v[j, i][c]; x2[r, c] += z2[j, i][c]
                CC[r] += c.astype(np.uint64); NC[r] += (~c).astype(np.uint64); EX[r] += beyond[j, i].astype(np.uint64)
            DD += dd; VV += vv; X2 += x2
    return DD, VV, X2, CC, NC, EX


def derive(DD, VV, X2, CC, NC, EX):
    """mean_diff = DD / CC, stderr = sqrt(VV) / CC, z = DD / sqrt(VV), chi2 = X2 / CC, exceed = EX / CC, coverage = CC / (CC + NC): float64, NaN where the
    denominator is 0."""
    c, root = CC.astype(np.float64), np.sqrt(VV)
    none = CC == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return {"mean_diff": np.where(none, np.nan, DD / c), "stderr": np.where(none, np.nan, root / c), "z": np.where(root == 0.0, np.nan, DD / root),
                "chi2": np.where(none, np.nan, X2 / c), "exceed": np.where(none, np.nan, EX.astype(np.float64) / c),
                "coverage": np.where(CC + NC == 0, np.nan, c / (CC + NC).astype(np.float64))}


def zmap(diff, var):
    """float32: diff / sqrt(var), 0 where var is +inf"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isposinf(var), np.float32(0.0), diff / np.sqrt(var)).astype(np.float32)
