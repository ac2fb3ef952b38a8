"""The numpy restatement of DEFOCUS (include/ssx.h "Depth of field after the render"): explicit binary32 operations in the header's order, the (dy, dx) walk as
the outer loops and all destinations at once inside them -- every destination still meets its sources in ascending dy, then ascending dx.  tests/
test_defocus_gpu.py holds ssx_defocus_images to it bit for bit; tests/test_defocus_cpu.py checks it against what the definition implies.

MUTANTS are the definition's near misses, for showing that the shared cases (tests/defocus_cases.py) can tell them apart."""
import numpy as np

F = np.float32
PI, THIRD = F(3.14159274), F(0.333333343)
MUTANTS = ("contract", "dx_outer", "cover_aq", "no_occlusion", "replicate")


def prepare(depth, R, K, focus):
    """inv [H, W], c and a [H, W, B]"""
    depth = np.ascontiguousarray(depth, dtype=F)
    focus = np.ascontiguousarray(focus, dtype=F)
    with np.errstate(all="ignore"):
        inv = np.where(depth > F(0), F(1) / depth, F(0)).astype(F)
        x = np.abs(inv[:, :, None] - focus[None, None, :]) * F(K)
        c = np.where(x < F(R), x, F(R)).astype(F)                                      # min(x, (float)R)
        a = F(1) / (PI * ((c * c + c) + THIRD))
    return inv, c, a.astype(F)


def defocus(q, depth, R, K, focus, mutant=None):
    q = np.ascontiguousarray(q, dtype=F)
    H, W, B = q.shape
    R = int(R)
    if R == 0 or F(K) == F(0):
        return q.copy()
    inv, c, a = prepare(depth, R, K, focus)
    edge = mutant == "replicate"
    pad = lambda x, fill: np.pad(x, [(R, R), (R, R)] + [(0, 0)] * (x.ndim - 2), mode="edge") if edge else np.pad(x, [(R, R), (R, R)] + [(0, 0)] * (x.ndim - 2), constant_values=fill)
    inv_p, c_p, a_p, q_p = pad(inv, 0), pad(c, 0), pad(a, 0), pad(q, 0)
    inside = np.pad(np.ones((H, W), dtype=bool), R, constant_values=edge)
    sw, sq = np.zeros((H, W, B), F), np.zeros((H, W, B), F)
    steps = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    if mutant == "dx_outer":
        steps = [(dy, dx) for dx in range(-R, R + 1) for dy in range(-R, R + 1)]
    with np.errstate(all="ignore"):
        for dy, dx in steps:
            win = (slice(R + dy, R + dy + H), slice(R + dx, R + dx + W))
            ok = inside[win]
            if not ok.any():
                continue
            cs, invs = c_p[win], inv_p[win][:, :, None]
            ce = cs if mutant == "no_occlusion" else np.where(invs < inv[:, :, None], np.where(cs < c, cs, c), cs)
            dist = np.sqrt(F(dx * dx + dy * dy), dtype=F)
            cover = (ce + F(1)) - dist
            cover = np.where(cover > F(0), cover, F(0))
            cover = np.where(cover < F(1), cover, F(1)).astype(F)
            taken = (cover > F(0)) & ok[:, :, None]
            w = cover * a_p[win]
            if mutant == "contract":
                term = (sq.astype(np.float64) + w.astype(np.float64) * q_p[win].astype(np.float64)).astype(F)
            elif mutant == "cover_aq":
                term = sq + cover * (a_p[win] * q_p[win])
            else:
                term = sq + w * q_p[win]
            sw = np.where(taken, sw + w, sw)
            sq = np.where(taken, term, sq)
        return (sq / sw).astype(F)


def scalar_defocus(q, depth, R, K, focus):
    """the header's loops as they stand, one destination at a time (small inputs only)"""
    q = np.ascontiguousarray(q, dtype=F)
    H, W, B = q.shape
    if R == 0 or F(K) == F(0):
        return q.copy()
    inv, c, a = prepare(depth, R, K, focus)
    out = np.zeros_like(q)
    with np.errstate(all="ignore"):
        for j in range(H):
            for i in range(W):
                for b in range(B):
                    sw, sq = F(0), F(0)
                    for dy in range(-R, R + 1):
                        for dx in range(-R, R + 1):
                            y, x = j + dy, i + dx
                            if not (0 <= x < W and 0 <= y < H):
                                continue
                            cs = c[y, x, b]
                            ce = (cs if cs < c[j, i, b] else c[j, i, b]) if inv[y, x] < inv[j, i] else cs
                            cover = F(ce + F(1)) - np.sqrt(F(dx * dx + dy * dy), dtype=F)
                            cover = cover if cover > F(0) else F(0)
                            cover = cover if cover < F(1) else F(1)
                            if cover > F(0):
                                w = F(cover * a[y, x, b])
                                sw = F(sw + w)
                                sq = F(sq + F(w * q[y, x, b]))
                    out[j, i, b] = F(sq) / F(sw)
    return out


def thin_lens(vfov_deg, height, bins, lambda_min, lambda_step, aperture, focus_distance, axial, lambda_ref):
    """ssh_defocus_thin_lens (include/ssx_host.h) in binary64, rounded once"""
    import math
    vfov = float(F(vfov_deg)) * (3.14159265358979323846 / 180.0)
    v_px = (float(height) / 2.0) / math.tan(vfov / 2.0)
    gain = F(0.5 * aperture * v_px)
    width = float(F(lambda_step)) / (bins // 4)
    focus = np.zeros(bins, F)
    for b in range(bins):
        lc = float(F(lambda_min)) + (b + 0.5) * width
        u = (lc - lambda_ref) / lambda_ref
        f = 1.0 / focus_distance + axial * u
        focus[b] = F(f if f > 0.0 else 0.0)
    return gain, focus
