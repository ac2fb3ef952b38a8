"""include/ssx.h "Demodulated denoising" restated on the CPU: the albedo bins traced with the oracle (camera_dir restated in float64, as tests/denoise_ref.py
does for the guide buffers), the channel albedo through the develop's restatement, the divide and the multiply in numpy float32, and the filter between them
through tests/denoise_spectral_ref.py with an all-zero albedo guide.  The GPU results are compared with these bit for bit.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import denoise_ref as dr
import denoise_spectral_ref as sr
import develop_ref
import oracle_lib as ol

F = np.float32
bits = sr.bits
DEFAULT_FLOOR, DEFAULT_SIGMA_L, DEFAULT_SUPERSAMPLE = F(1.0 / 16.0), 1.0, 2     # include/ssx.h SSX_DEMOD_DEFAULT_*; chosen in DESIGN.md section 15


def sub_pixel_rays(orc, W, H, ox, oy):
    """Ray directions float32 [H, W, 3] through (i + ox, j + oy) of every pixel, and the camera position: denoise_ref.camera_rays with another offset."""
    pv = np.array(orc.lib.orc_scene_pv_inv(orc.scene)[:16], dtype=np.float64)
    cam = np.array(orc.lib.orc_scene_cam_pos(orc.scene)[:3], dtype=np.float32).astype(np.float64)
    x = (np.arange(W, dtype=np.float64) + np.float64(ox))[None, :] + np.zeros((H, 1))
    y = (np.arange(H, dtype=np.float64) + np.float64(oy))[:, None] + np.zeros((1, W))
    ndc_x = (x / np.float64(W)) * 2.0 - 1.0
    ndc_y = (y / np.float64(H)) * 2.0 - 1.0
    q = [(pv[0 * 4 + r] * ndc_x + pv[1 * 4 + r] * ndc_y) + (pv[2 * 4 + r] * 0.0 + pv[3 * 4 + r] * 1.0) for r in range(4)]
    d = [q[k] / q[3] - cam[k] for k in range(3)]
    inv = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return np.stack([(d[k] * inv).astype(F) for k in range(3)], axis=-1), cam.astype(F)


def albedo_bins(orc, W, H, B, K):
    """rho float32 [H, W, B] as ALBEDO BINS defines it, from orc_scene_intersect and orc_material_albedo (spectral mode)."""
    assert B % 4 == 0 and 4 <= B <= 64 and K in (1, 2, 4)
    lib = orc.lib
    lib.orc_material_albedo.restype = None
    lib.orc_material_albedo.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(dr._OrcMaterial), ol.V2, C.c_float, C.POINTER(C.c_float), C.c_void_p]
    head = C.cast(orc.scene, C.POINTER(dr._OrcSceneHead)).contents
    col = C.cast(orc.color, C.POINTER(dr._OrcColorHead)).contents
    M = B // 4
    sub_step = F(col.lambda_step) / F(M)
    lambdas = [float(F(col.lambda_min) + (F(m) + F(0.5)) * sub_step) for m in range(M)]
    acc = np.zeros((H, W, B), dtype=F)
    hit, out = ol.Hit(), (C.c_float * 4)()
    for c in range(K):                                                          # rows outer, columns inner
        for a in range(K):
            dirs, cam = sub_pixel_rays(orc, W, H, (a + 0.5) / K, (c + 0.5) / K)
            origin = ol.V3(*[float(v) for v in cam])
            add = np.zeros((H, W, B), dtype=F)                                  # a miss adds +0
            for j in range(H):
                for i in range(W):
                    ray = ol.Ray(origin, ol.V3(*[float(v) for v in dirs[j, i]]))
                    if not lib.orc_scene_intersect(orc.scene, C.byref(ray), C.byref(hit), -1, None):
                        continue
                    mat = C.byref(head.materials[lib.orc_scene_quad_material(orc.scene, hit.prim)])
                    for m in range(M):
                        lib.orc_material_albedo(orc.color, orc.scene, mat, hit.st, C.c_float(lambdas[m]), out, None)
                        add[j, i, m::M] = out[:]                                # bins i * M + m, i = 0..3
            acc = (acc + add).astype(F)
    rho = acc / F(K * K)
    assert rho.dtype == F
    return rho


def channel_albedo(rho, weights_xyz):
    """rho_c float32 [H, W, 3] = DEVELOP(rho, Wc) / DEVELOP(ones, Wc)"""
    w = np.ascontiguousarray(weights_xyz, dtype=F)
    den = develop_ref.develop(np.ones((1, w.shape[1]), dtype=F), w)[0]
    assert (den > 0).all()
    out = develop_ref.develop(rho, w) / den
    assert out.dtype == F
    return out


def floored(r, floor):
    return np.where(r > F(floor), r, F(floor)).astype(F)


def demodulate(e0, c, var, rho, rho_c, floor):
    """(e0', c', var', valid): the B sum channels of e0 [H, W, B + M] by r~, X, Y, Z by r~_c, var by r~_c[1]^2; invalid pixels keep everything."""
    B = rho.shape[-1]
    r, rc = floored(rho, floor), floored(rho_c, floor)
    valid = dr.valid_mask(c, var)
    with np.errstate(all="ignore"):
        e2 = np.concatenate([e0[..., :B] / r, e0[..., B:]], axis=-1)
        c2 = np.concatenate([c[..., :3] / rc, c[..., 3:]], axis=-1)
        v2 = var / (rc[..., 1] * rc[..., 1])
    assert e2.dtype == F and c2.dtype == F and v2.dtype == F
    return np.where(valid[..., None], e2, e0), np.where(valid[..., None], c2, c), np.where(valid, v2, var), valid


def remodulate(eL, cL, varL, rho, rho_c, floor, valid):
    """(out [H, W, B], c_out, var_out): the ratio times r~, X, Y, Z times r~_c, var times r~_c[1]^2; pixels that were invalid on input are not multiplied."""
    B = rho.shape[-1]
    r, rc = floored(rho, floor), floored(rho_c, floor)
    ratio = sr.spectral_ratio(eL, B)
    with np.errstate(all="ignore"):
        out = np.where(eL[..., B + np.arange(B) % (B // 4)] > 0, ratio * np.where(valid[..., None], r, F(1)), F(0))
        c2 = np.concatenate([cL[..., :3] * rc, cL[..., 3:]], axis=-1)
        v2 = varL * (rc[..., 1] * rc[..., 1])
    assert out.dtype == F and c2.dtype == F and v2.dtype == F
    return out, np.where(valid[..., None], c2, cL), np.where(valid, v2, varL)


def denoise_spectral_demod(e0, c, var, prim, rho, weights_xyz, floor=DEFAULT_FLOOR, levels=5, sigma_l=DEFAULT_SIGMA_L, channels=None):
    """(out [H, W, B], c_out, var_out): the whole definition from the spectral channels e0 [H, W, B + M].  `channels` replaces the numpy filter by another
    implementation of FILTER with EXTRA CHANNELS (the GPU's pure function): channels(c, var, prim, albedo, e, levels, sigma_l) -> (e', c', var')."""
    c = np.ascontiguousarray(c, dtype=F); var = np.ascontiguousarray(var, dtype=F)
    rho_c = channel_albedo(rho, weights_xyz)
    e1, c1, v1, valid = demodulate(e0, c, var, rho, rho_c, floor)
    zero = np.zeros(c.shape, dtype=F)                                           # wa = 1 / (1 + 0) = 1: sigma_a does not matter
    if channels is None:
        cL, vL, eL = sr.atrous_channels(c1, v1, prim, zero, e1, levels=levels, sigma_l=sigma_l, sigma_a=1.0)
    else:
        eL, cL, vL = channels(c1, v1, prim, zero, e1, levels, sigma_l)
    return remodulate(eL, cL, vL, rho, rho_c, floor, valid)
