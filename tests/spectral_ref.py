"""include/ssx.h "Spectral radiance output" restated: the bins as a sequential sum over the per-sample hero fluxes, and the projection of those fluxes onto the
oracle's per-sample XYZ.  TEST INFRASTRUCTURE, shared by tests/test_spectral_gpu.py and tests/test_pipeline_matrix_gpu.py."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from simple_spectral_amd.renderer import spectral_bin_index


def restate_bins(flux, lam, lambda_min, lambda_step, bins):
    """The definition, sequentially: (sums float64 [H, W, B], counts uint32 [H, W, M], mean float32 [H, W, B]) from the per-sample flux [H, W, spp, 4] and
    lambda_0 [H, W, spp], with the scene's lambda_min and lambda_step."""
    H, W, spp = lam.shape
    M = bins // 4
    m = spectral_bin_index(lam, lambda_min, lambda_step, bins)
    S, N = np.zeros((H, W, bins), dtype=np.float64), np.zeros((H, W, M), dtype=np.uint32)
    J, I = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for k in range(spp):                       # ascending k; every pixel appears once per statement
        for i in range(4):
            S[J, I, i * M + m[:, :, k]] += flux[:, :, k, i].astype(np.float64)
        N[J, I, m[:, :, k]] += np.uint32(1)
    n = np.tile(N, (1, 1, 4)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n > 0, S / n, 0.0).astype(np.float32)
    return S, N, mean


def restate_moments(flux, lam, lambda_min, lambda_step, bins):
    """include/ssx.h "Spectral moments", sequentially: Q float64 [H, W, B], Q[i * M + m] += (double)f[i] * (double)f[i] in ascending k from +0.0 -- the product
    of the two converted binary32 values, taken in binary64 (where it is exact)."""
    H, W, spp = lam.shape
    M = bins // 4
    m = spectral_bin_index(lam, lambda_min, lambda_step, bins)
    Q = np.zeros((H, W, bins), dtype=np.float64)
    J, I = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(spp):                   # ascending k; every pixel appears once per statement
            for i in range(4):
                d = flux[:, :, k, i].astype(np.float64)
                Q[J, I, i * M + m[:, :, k]] += d * d
    return Q


def project_flux(o, flux, lam, seed, lambda_min, lambda_step):
    """(proj float32 [H, W, spp, 3], lambda_0 restated [H, W, spp]): every sample's flux through orc_specradflux_to_ciexyz_hero of the oracle `o`, and the draw of
    its first hero wavelength restated (renderer.cpp:113,138: two doubles of sub-pixel offset, then the wavelength)."""
    H, W, spp = lam.shape
    rng, out = ol.Rng(), (C.c_float * 3)()
    proj, lam_ref = np.zeros((H, W, spp, 3), dtype=np.float32), np.zeros((H, W, spp), dtype=np.float32)
    for j in range(H):
        for i in range(W):
            for k in range(spp):
                f = (C.c_float * 4)(*[float(x) for x in flux[j, i, k]])
                o.lib.orc_specradflux_to_ciexyz_hero(o.color, f, C.c_float(float(lam[j, i, k])), out)
                proj[j, i, k] = out[:]
                o.lib.orc_seed_sample(seed, j * W + i, k, C.byref(rng))
                o.lib.orc_rand_1d(C.byref(rng)); o.lib.orc_rand_1d(C.byref(rng))
                lam_ref[j, i, k] = lambda_min + np.float32(o.lib.orc_rand_1f(C.byref(rng))) * lambda_step
    return proj, lam_ref
