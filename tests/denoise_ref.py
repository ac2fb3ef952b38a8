"""The denoising definitions of include/ssx.h restated on the CPU: `atrous` is the filter in numpy float32, tap by tap in the stated order; `guides_ref`
traces the pixel-centre rays with the oracle (camera_dir restated in float64).  The GPU results are compared with these bit for bit.  TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import oracle_lib as ol

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
H5 = (F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16))
DEFAULTS = dict(levels=5, sigma_l=1.0, sigma_a=0.1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def valid_mask(c, var):
    return np.isfinite(c[..., 0]) & np.isfinite(c[..., 1]) & np.isfinite(c[..., 2]) & np.isfinite(var)


def _tap(H, W, dy, dx):
    """(inside [H, W], qy, qx clipped) of the neighbour at offset (dx, dy)"""
    qy = np.arange(H)[:, None] + dy + np.zeros((1, W), dtype=np.int64)
    qx = np.arange(W)[None, :] + dx + np.zeros((H, 1), dtype=np.int64)
    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
    return inside, np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)


def atrous_level(c, var, prim, albedo, step, sigma_l, sigma_a):
    """One level: (c', var') from float32 c [H, W, 4], var [H, W], uint32 prim [H, W], float32 albedo [H, W, 4]."""
    H, W = var.shape
    valid = valid_mask(c, var)
    sigma_l, sigma_a = F(sigma_l), F(sigma_a)
    inv_sa2 = F(1) / (sigma_a * sigma_a)
    with np.errstate(all="ignore"):
        gs, ks = np.zeros((H, W), F), np.zeros((H, W), F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, qy, qx = _tap(H, W, dy, dx)
                m = inside & valid[qy, qx]
                k3 = F((2 if dy == 0 else 1) * (2 if dx == 0 else 1))
                gs = np.where(m, gs + k3 * var[qy, qx], gs)
                ks = np.where(m, ks + k3, ks)
        g = gs / ks
        den = sigma_l * np.sqrt(g) + F(1e-6)
        sw, sv = np.zeros((H, W), F), np.zeros((H, W), F)
        sc = np.zeros((H, W, 3), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                inside, qy, qx = _tap(H, W, step * dy, step * dx)
                m = inside & valid[qy, qx] & (prim[qy, qx] == prim)
                k = H5[dy + 2] * H5[dx + 2]
                cq, vq = c[qy, qx], var[qy, qx]
                x = np.abs(cq[..., 1] - c[..., 1]) / den
                wl = F(1) / (F(1) + x * x)
                d = albedo[qy, qx] - albedo
                da2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) + d[..., 3] * d[..., 3]
                wa = F(1) / (F(1) + da2 * inv_sa2)
                w = (k * wl) * wa
                sw = np.where(m, sw + w, sw)
                sc = np.where(m[..., None], sc + w[..., None] * cq[..., :3], sc)
                sv = np.where(m, sv + (w * w) * vq, sv)
        c2 = np.concatenate([sc / sw[..., None], c[..., 3:]], axis=-1)
        v2 = sv / (sw * sw)
    assert c2.dtype == F and v2.dtype == F
    return np.where(valid[..., None], c2, c), np.where(valid, v2, var)


def atrous(c, var, prim, albedo, levels=5, sigma_l=1.0, sigma_a=0.1):
    c = np.ascontiguousarray(c, dtype=F); var = np.ascontiguousarray(var, dtype=F)
    prim = np.ascontiguousarray(prim, dtype=np.uint32); albedo = np.ascontiguousarray(albedo, dtype=F)
    for l in range(levels):
        c, var = atrous_level(c, var, prim, albedo, 1 << l, sigma_l, sigma_a)
    return c, var


def variance_in_image_units(v, rgb=False):
    """var = (float)(v * (s * s)) in binary64; s = 1000, or 1 in RGB mode"""
    s = 1.0 if rgb else 1000.0
    return (np.asarray(v, dtype=np.float64) * (s * s)).astype(F)


# ---- the guide buffers from the oracle ----------------------------------------------------------------------------------------------------------------

class _OrcSpectrum(C.Structure):  # oracle/oracle.h orc_spectrum
    _fields_ = [("data", C.c_void_p), ("n", C.c_int), ("low", C.c_float), ("high", C.c_float), ("delta_lambda", C.c_float), ("delta_lambda_recip", C.c_float)]


class _OrcMaterial(C.Structure):  # orc_material
    _fields_ = [("kind", C.c_int), ("albedo_mode", C.c_int), ("emission", _OrcSpectrum), ("albedo", _OrcSpectrum), ("texture", C.c_void_p),
                ("rgb_emission", C.c_float * 3), ("rgb_albedo", C.c_float * 3)]


class _OrcCamera(C.Structure):  # orc_camera
    _fields_ = [("pos", ol.V3), ("dir", ol.V3), ("up", ol.V3), ("res", C.c_size_t * 2), ("near_", C.c_float), ("far_", C.c_float), ("vfov_deg", C.c_float),
                ("matr_P", C.c_double * 16), ("matr_V", C.c_double * 16), ("matr_PV_inv", C.c_double * 16)]


class _OrcSceneHead(C.Structure):  # the first members of orc_scene
    _fields_ = [("camera", _OrcCamera), ("materials", C.POINTER(_OrcMaterial)), ("n_materials", C.c_int)]


class _OrcColorHead(C.Structure):  # the first members of orc_color
    _fields_ = [("observer", C.c_int), ("lambda_min", C.c_float), ("lambda_max", C.c_float), ("lambda_step", C.c_float)]


def camera_rays(orc, W, H):
    """Pixel-centre ray directions float32 [H, W, 3]: camera_dir (csrc/ssx_kernels.hip; reference renderer.cpp:114-131) and the normalisation of
    generate_sample, in float64 operation by operation."""
    pv = np.array(orc.lib.orc_scene_pv_inv(orc.scene)[:16], dtype=np.float64)      # column-major m[col * 4 + row]
    cam = np.array(orc.lib.orc_scene_cam_pos(orc.scene)[:3], dtype=np.float32).astype(np.float64)
    x = (np.arange(W, dtype=np.float64) + 0.5)[None, :] + np.zeros((H, 1))
    y = (np.arange(H, dtype=np.float64) + 0.5)[:, None] + np.zeros((1, W))
    ndc_x = (x / np.float64(W)) * 2.0 - 1.0
    ndc_y = (y / np.float64(H)) * 2.0 - 1.0
    q = [(pv[0 * 4 + r] * ndc_x + pv[1 * 4 + r] * ndc_y) + (pv[2 * 4 + r] * 0.0 + pv[3 * 4 + r] * 1.0) for r in range(4)]
    d = [q[k] / q[3] - cam[k] for k in range(3)]
    inv = 1.0 / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return np.stack([(d[k] * inv).astype(F) for k in range(3)], axis=-1), cam.astype(F)


def guides_ref(orc, W, H, rgb=False):
    """{"prim", "depth", "normal", "albedo"} as ssx_guides defines them, from orc_scene_intersect and orc_material_albedo."""
    lib = orc.lib
    lib.orc_material_albedo.restype = None
    lib.orc_material_albedo.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_OrcMaterial), ol.V2, C.c_float, C.POINTER(C.c_float), C.c_void_p]
    head = C.cast(orc.scene, C.POINTER(_OrcSceneHead)).contents
    col = C.cast(orc.color, C.POINTER(_OrcColorHead)).contents
    lambda_g = F(0) if rgb else F(col.lambda_min) + F(0.5) * F(col.lambda_step)
    dirs, cam = camera_rays(orc, W, H)
    g = {"prim": np.full((H, W), MISS, dtype=np.uint32), "depth": np.zeros((H, W), F), "normal": np.zeros((H, W, 3), F), "albedo": np.zeros((H, W, 4), F)}
    hit, out = ol.Hit(), (C.c_float * 4)()
    for j in range(H):
        for i in range(W):
            ray = ol.Ray(ol.V3(*[float(v) for v in cam]), ol.V3(*[float(v) for v in dirs[j, i]]))
            if not lib.orc_scene_intersect(orc.scene, C.byref(ray), C.byref(hit), -1, None):
                continue
            m = lib.orc_scene_quad_material(orc.scene, hit.prim)
            assert 0 <= m < head.n_materials
            lib.orc_material_albedo(orc.color, orc.scene, C.byref(head.materials[m]), hit.st, C.c_float(float(lambda_g)), out, None)
            g["prim"][j, i] = hit.prim
            g["depth"][j, i] = hit.dist
            g["normal"][j, i] = (hit.normal.x, hit.normal.y, hit.normal.z)
            g["albedo"][j, i] = out[:]
    return g


def synthetic(W, H, seed):
    """Inputs that reach every branch of the filter: blobs of three primitive ids plus misses, random colour and albedo, variances including 0, a
    denormal and inf, one NaN colour pixel.  Returns (c, var, prim, albedo)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    prim = np.full((H, W), MISS, dtype=np.uint32)
    for k, (cx, cy, r) in enumerate(((0.25, 0.3, 0.35), (0.7, 0.6, 0.4), (0.5, 0.95, 0.3))):
        prim[(xx - cx * W) ** 2 + (yy - cy * H) ** 2 <= (r * max(W, H)) ** 2] = k * 5 + 1
    c = g.uniform(0, 4, size=(H, W, 4)).astype(F)
    c[..., 3] = g.integers(0, 2, size=(H, W)).astype(F)
    albedo = (g.uniform(0, 1, size=(H, W, 4)) * (0.2 + 0.8 * (prim[..., None] % 3 == 1))).astype(F)
    var = (g.uniform(0, 0.5, size=(H, W)) ** 2).astype(F)
    flat = g.permutation(W * H)
    var.flat[flat[0]] = F(0)
    var.flat[flat[1]] = np.uint32(0x00000123).view(F)     # a denormal
    var.flat[flat[2]] = F(np.inf)
    c.reshape(-1, 4)[flat[3], g.integers(0, 3)] = F(np.nan)
    if W * H > 8:
        var.flat[flat[4:6]] = F(0)
    return c, var, prim, albedo
