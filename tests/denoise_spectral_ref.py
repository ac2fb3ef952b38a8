"""The extra channels of the a-trous filter and the spectral channels built on them (include/ssx.h "Denoising the spectral bins") restated on the CPU in
numpy float32, tap by tap in the stated order -- a restatement of its own, c' and var' included (tests/test_denoise_spectral_cpu.py holds those against
tests/denoise_ref.py bit for bit).  The GPU results are compared with these bit for bit.  TEST INFRASTRUCTURE."""
import numpy as np

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _valid(c, var):
    return np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2]) & np.isfinite(var)


def _shift(H, W, dy, dx):
    """(inside, qy, qx): whether the pixel at offset (dx, dy) is in the image, and its coordinates clipped into it"""
    qy, qx = np.mgrid[0:H, 0:W]
    qy, qx = qy + dy, qx + dx
    return (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W), np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)


def channels_level(c, var, prim, albedo, e, step, sigma_l, sigma_a):
    """One level: (c', var', e') from float32 c [H, W, 4], var [H, W], uint32 prim [H, W], float32 albedo [H, W, 4] and e [H, W, E]."""
    H, W = var.shape
    valid = _valid(c, var)
    sigma_l, sigma_a = F(sigma_l), F(sigma_a)
    inv_sa2 = F(1) / (sigma_a * sigma_a)
    with np.errstate(all="ignore"):
        gs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, qy, qx = _shift(H, W, dy, dx)
                m = inside & valid[qy, qx]
                k3 = F(2 if dy == 0 else 1) * F(2 if dx == 0 else 1)
                gs = np.where(m, gs + k3 * var[qy, qx], gs)
                ks = np.where(m, ks + k3, ks)
        den = sigma_l * np.sqrt(gs / ks) + F(1e-6)
        sw, sv = np.zeros((H, W), F), np.zeros((H, W), F)
        sc, se = np.zeros((H, W, 3), F), np.zeros(e.shape, F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inside, qy, qx = _shift(H, W, step * dy, step * dx)
                m = inside & valid[qy, qx] & (prim[qy, qx] == prim)      # a tap that is not counted is skipped, not added with weight 0
                k = H5[dy + 2] * H5[dx + 2]
                x = np.abs(c[qy, qx, 1] - c[..., 1]) / den
                wl = F(1) / (F(1) + x * x)
                d = albedo[qy, qx] - albedo
                da2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
                wa = F(1) / (F(1) + da2 * inv_sa2)
                w = (k * wl) * wa
                sw = np.where(m, sw + w, sw)
                sc = np.where(m[..., None], sc + w[..., None] * c[qy, qx, :3], sc)
                sv = np.where(m, sv + (w * w) * var[qy, qx], sv)
                se = np.where(m[..., None], se + w[..., None] * e[qy, qx], se)
        c2 = np.concatenate([sc / sw[..., None], c[..., 3:]], axis=-1)
        v2 = sv / (sw * sw)
        e2 = se / sw[..., None]
    assert c2.dtype == F and v2.dtype == F and e2.dtype == F
    return np.where(valid[..., None], c2, c), np.where(valid, v2, var), np.where(valid[..., None], e2, e)


def atrous_channels(c, var, prim, albedo, e, levels=5, sigma_l=1.0, sigma_a=0.1):
    """(c, var, e) after `levels` levels, steps 1, 2, 4, ..."""
    c = np.ascontiguousarray(c, dtype=F); var = np.ascontiguousarray(var, dtype=F); e = np.ascontiguousarray(e, dtype=F)
    prim = np.ascontiguousarray(prim, dtype=np.uint32); albedo = np.ascontiguousarray(albedo, dtype=F)
    for l in range(levels):
        c, var, e = channels_level(c, var, prim, albedo, e, 1 << l, sigma_l, sigma_a)
    return c, var, e


def spectral_channels(S, N, n):
    """e0 [H, W, B + M] from the sums S float64 [H, W, B], the counts N uint32 [H, W, M] and n = done_spp: both divisions binary64, then rounded."""
    n = np.float64(n)
    return np.concatenate([(np.asarray(S, dtype=np.float64) / n).astype(F), (np.asarray(N).astype(np.float64) / n).astype(F)], axis=-1)


def spectral_ratio(eL, B):
    """out [H, W, B] = eL[b] / eL[B + b % M] where that count channel is positive, else 0"""
    M = B // 4
    den = eL[..., B + np.arange(B) % M]
    with np.errstate(all="ignore"):
        out = np.where(den > 0, eL[..., :B] / den, F(0))
    assert out.dtype == F
    return out


def denoise_spectral(S, N, n, c, var, prim, albedo, **params):
    """(out [H, W, B], c', var'): the whole definition"""
    c2, v2, eL = atrous_channels(c, var, prim, albedo, spectral_channels(S, N, n), **params)
    return spectral_ratio(eL, S.shape[-1]), c2, v2
