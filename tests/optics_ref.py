"""The lens of include/ssx.h ("Developing through a lens") restated in numpy: WARP, then BLUR, in binary32, operation by operation in the order the header
writes them.  The device output is compared with this bit for bit.

`mutant` names one of the near misses the tests must be able to tell from the definition (tests/test_optics_cpu.py checks that every one of them differs in
bits on the shared case list); None is the definition."""
import numpy as np

F = np.float32
MUTANTS = ("contracted", "descending", "vertical_first", "blur_first", "zero_border", "no_half", "r0_multiplied")


def _mul_add(acc, a, b, contracted):
    """acc + (a * b): the product rounded before the add; contracted: one rounding (binary32 products are exact in binary64; the sum is then rounded once more
    on the way back, which is as close to a fused multiply-add as a mutant needs to be)."""
    if contracted:
        with np.errstate(all="ignore"):
            return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F)
    return acc + a * b


def _axis(n, c, s, extent, no_half):
    """WARP along one axis for destination indices 0 .. n-1: (ka, kb, f)"""
    k = np.arange(n, dtype=np.int64).astype(F)
    c, s = F(c), F(s)
    with np.errstate(all="ignore"):
        if no_half:
            x = c + (k - c) * s
        else:
            d = (k + F(0.5)) - c
            x = (c + d * s) - F(0.5)
        x = np.where(x > F(-1.0), x, F(-1.0)).astype(F)
        x = np.where(x < F(extent), x, F(extent)).astype(F)
        x0 = np.floor(x)
        f = (x - x0).astype(F)
    k0 = x0.astype(np.int64)
    return np.clip(k0, 0, extent - 1), np.clip(k0 + 1, 0, extent - 1), f


def _take(q, jj, ii, zero, valid_j=None, valid_i=None):
    v = q[np.ix_(jj, ii)]
    if zero:
        v = np.where(np.logical_and.outer(valid_j, valid_i), v, F(0.0)).astype(F)
    return v


def warp(q, cx, cy, scale, mutant=None):
    H, W, B = q.shape
    out = np.empty_like(q)
    contracted, zero, no_half = mutant == "contracted", mutant == "zero_border", mutant == "no_half"
    for b in range(B):
        s = F(scale[b])
        if s == F(1.0):
            out[:, :, b] = q[:, :, b]
            continue
        ia, ib, fx = _axis(W, cx, s, W, no_half)
        ja, jb, fy = _axis(H, cy, s, H, no_half)
        plane = q[:, :, b]
        if zero:  # the neighbours outside the image read 0 instead of the border pixel
            ia0, ja0 = _axis_raw(W, cx, s, W, no_half), _axis_raw(H, cy, s, H, no_half)
            vi = [(ia0 >= 0) & (ia0 < W), (ia0 + 1 >= 0) & (ia0 + 1 < W)]
            vj = [(ja0 >= 0) & (ja0 < H), (ja0 + 1 >= 0) & (ja0 + 1 < H)]
        else:
            vi = vj = [None, None]
        gx, gy = (F(1.0) - fx)[None, :], (F(1.0) - fy)[:, None]
        fxr, fyc = fx[None, :], fy[:, None]
        with np.errstate(all="ignore"):
            rows = []
            for jj, vjj in ((ja, vj[0]), (jb, vj[1])):
                a = _take(plane, jj, ia, zero, vjj, vi[0])
                c = _take(plane, jj, ib, zero, vjj, vi[1])
                rows.append(_mul_add(a * gx, c, np.broadcast_to(fxr, c.shape), contracted))
            out[:, :, b] = _mul_add(rows[0] * gy, rows[1], np.broadcast_to(fyc, rows[1].shape), contracted)
    return out


def _axis_raw(n, c, s, extent, no_half):
    """the unclamped floor index of _axis (for the zero-border mutant)"""
    k = np.arange(n, dtype=np.int64).astype(F)
    c, s = F(c), F(s)
    with np.errstate(all="ignore"):
        x = c + (k - c) * s if no_half else (c + ((k + F(0.5)) - c) * s) - F(0.5)
        x = np.where(x > F(-1.0), x, F(-1.0)).astype(F)
        x = np.where(x < F(extent), x, F(extent)).astype(F)
    return np.floor(x).astype(np.int64)


def blur_pass(w, axis, R, radius, taps, mutant=None):
    """One pass of BLUR along axis 1 (i) or 0 (j)."""
    out = np.empty_like(w)
    n = w.shape[axis]
    idx = np.arange(n)
    contracted, zero = mutant == "contracted", mutant == "zero_border"
    for b in range(w.shape[2]):
        r = int(radius[b])
        plane = w[:, :, b]
        if r == 0 and mutant != "r0_multiplied":
            out[:, :, b] = plane
            continue
        acc = np.zeros(plane.shape, dtype=F)
        ds = range(-r, r + 1)
        for d in (reversed(ds) if mutant == "descending" else ds):
            src = idx + d
            v = np.take(plane, np.clip(src, 0, n - 1), axis=axis)
            if zero:
                ok = (src >= 0) & (src < n)
                v = np.where(ok[None, :] if axis == 1 else ok[:, None], v, F(0.0)).astype(F)
            k = np.full(plane.shape, F(taps[b, d + R]), dtype=F)
            with np.errstate(all="ignore"):
                acc = _mul_add(acc, v, k, contracted)
        out[:, :, b] = acc
    return out


def blur(w, R, radius, taps, mutant=None):
    first, second = (0, 1) if mutant == "vertical_first" else (1, 0)
    return blur_pass(blur_pass(w, first, R, radius, taps, mutant), second, R, radius, taps, mutant)


def optics(q, cx, cy, R, scale, radius, taps, mutant=None):
    """q float32 [H, W, B]; scale float32 [B]; radius [B] <= R; taps float32 [B, 2 R + 1] -> float32 [H, W, B]"""
    q = np.ascontiguousarray(q, dtype=F)
    scale = np.asarray(scale, dtype=F)
    taps = np.asarray(taps, dtype=F).reshape(q.shape[2], 2 * R + 1)
    assert mutant is None or mutant in MUTANTS
    if mutant == "blur_first":
        return warp(blur(q, R, radius, taps), cx, cy, scale)
    return blur(warp(q, cx, cy, scale, mutant), R, radius, taps, mutant)


def lens(bins, lambda_min, lambda_step, lambda_ref, lateral, sigma_ref, axial, max_radius):
    """ssh_optics_lens (include/ssx_host.h) restated: (scale float32 [B], radius uint32 [B], taps float32 [B, 2 R + 1]), binary64 rounded once at the end."""
    R = int(max_radius)
    M = bins // 4
    width = np.float64(F(lambda_step)) / M
    scale, radius, taps = np.zeros(bins, F), np.zeros(bins, np.uint32), np.zeros((bins, 2 * R + 1), F)
    for b in range(bins):
        lc = np.float64(F(lambda_min)) + (b + 0.5) * width
        u = (lc - np.float64(lambda_ref)) / np.float64(lambda_ref)
        scale[b] = F(1.0 + np.float64(lateral) * u)
        sd, ax = np.float64(sigma_ref) * lc / np.float64(lambda_ref), np.float64(axial) * u
        sigma = np.sqrt(sd * sd + ax * ax)
        if sigma * sigma == 0.0:
            continue
        r = int(min(float(R), np.ceil(3.0 * sigma)))
        radius[b] = r
        k = [np.exp(-np.float64(d * d) / (2.0 * (sigma * sigma))) for d in range(-r, r + 1)]
        total = np.float64(0.0)
        for v in k:
            total = total + v
        for d in range(-r, r + 1):
            taps[b, d + R] = F(k[d + r] / total)
    return scale, radius, taps
