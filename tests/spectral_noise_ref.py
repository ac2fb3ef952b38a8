"""include/ssx.h "Spectral noise figure" restated in numpy: binary64, IEEE + - * / only, every operation in the order the header writes it, so that the device's
results are compared with these bit for bit.  TEST INFRASTRUCTURE, shared by tests/test_spectral_noise_cpu.py and tests/test_spectral_noise_gpu.py."""
import numpy as np

from simple_spectral_amd.dist import tile_owner_mask
from spectral_stats_ref import deviations


def per_pixel(S, Q, N):
    """(e, mu float64 [H, W, B], estimable bool [H, W, B]): n = N[b % M]; n >= 2: e = (q / (double)(n-1)) / (double)n, mu = S / (double)n (elsewhere unused)."""
    n = np.tile(N, (1, 1, 4))
    q = deviations(S, Q, n)
    nf = n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = (q / (nf - 1.0)) / nf
        mu = S / nf
    return e, mu, n >= 2


def tile_partials(S, Q, N, mask=None, owner=None):
    """(tEV, tEM float64, tPP, tPU uint32), each [tiles, B]: per 8x8 tile t = ty * tiles_x + tx the in-image, in-mask pixels in ascending row, then ascending
    column, every partial from +0.0 / 0.  owner = (tile_first, tile_stride, tile_skew): the tiles that context does not own keep +0.0 and 0."""
    H, W, B = S.shape
    e, mu, est = per_pixel(S, Q, N)
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    inside = np.ones((H, W), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    owned = np.ones((H, W), dtype=bool) if owner is None else tile_owner_mask(W, H, *owner)
    tEV, tEM = np.zeros((tiles_x * tiles_y, B)), np.zeros((tiles_x * tiles_y, B))
    tPP, tPU = np.zeros((tiles_x * tiles_y, B), dtype=np.uint32), np.zeros((tiles_x * tiles_y, B), dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                if not owned[ty * 8, tx * 8]:
                    continue
                t = ty * tiles_x + tx
                for j in range(ty * 8, min(ty * 8 + 8, H)):
                    for i in range(tx * 8, min(tx * 8 + 8, W)):
                        if not inside[j, i]:
                            continue
                        k = est[j, i]
                        tEV[t, k] += e[j, i, k]
                        tEM[t, k] += mu[j, i, k]
                        tPP[t, k] += np.uint32(1)
                        tPU[t, ~k] += np.uint32(1)
    return tEV, tEM, tPP, tPU


def totals(tEV, tEM, tPP, tPU):
    """(EV, EM float64, PP, PU uint64), each [B]: the tile partials added in ascending t, from +0.0 / 0."""
    B = tEV.shape[1]
    EV, EM, PP, PU = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(tEV.shape[0]):
            EV += tEV[t]; EM += tEM[t]
            PP += tPP[t].astype(np.uint64); PU += tPU[t].astype(np.uint64)
    return EV, EM, PP, PU


def merge_owned(parts, W, H, owners):
    """Several contexts' tile partials merged by ownership: tile t from the context that owns it."""
    tiles_x = (W + 7) // 8
    out = [np.zeros_like(a) for a in parts[0]]
    for part, owner in zip(parts, owners):
        owned = tile_owner_mask(W, H, *owner)
        for t in range(out[0].shape[0]):
            if owned[(t // tiles_x) * 8, (t % tiles_x) * 8]:
                for o, a in zip(out, part):
                    o[t] = a[t]
    return tuple(out)


def derive(EV, EM, PP, PU):
    """(noise, coverage, rel [B]): sums over ascending b from +0.0 / 0; noise = sqrt(EVs / P) / (EMs / P), NaN when P == 0 or the mean is 0; coverage = P / (P + U),
    NaN when P + U == 0; rel[b] = sqrt(EV[b] / PP[b]) / (EM[b] / PP[b]), NaN when PP[b] == 0 or the bin's mean is 0."""
    evs, ems, P, U = np.float64(0.0), np.float64(0.0), 0, 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for b in range(EV.shape[0]):
            evs = evs + EV[b]; ems = ems + EM[b]; P += int(PP[b]); U += int(PU[b])
        n = PP.astype(np.float64)
        mean_b = EM / n
        rel = np.where((PP == 0) | (mean_b == 0.0), np.nan, np.sqrt(EV / n) / mean_b)
        mean = ems / np.float64(P)
        noise = np.float64(np.nan) if (P == 0 or mean == 0.0) else np.sqrt(evs / np.float64(P)) / mean
        coverage = np.float64(np.nan) if P + U == 0 else np.float64(P) / np.float64(P + U)
    return float(noise), float(coverage), rel


def figure(S, Q, N, mask=None):
    """(noise, coverage) of a whole image: the restatement end to end."""
    noise, coverage, _ = derive(*totals(*tile_partials(S, Q, N, mask)))
    return noise, coverage
