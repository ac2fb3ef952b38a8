"""include/ssx.h "Glare: per-bin convolution by FFT", restated in numpy: binary32 throughout, one rounded operation per numpy call, each butterfly stage
vectorised over its blocks and lines.  The tables are arguments, as they are the library's.  `variant` swaps in one of the near misses the CPU test holds the
definition against; None is the definition."""
import numpy as np

F = np.float32
VARIANTS = ("correlation", "inverse_rows_first", "twiddles_not_conjugated", "zero_border", "px_halved")


def bitrev(P):
    n = P.bit_length() - 1
    k = np.arange(P)
    r = np.zeros(P, dtype=np.int64)
    for bit in range(n):
        r |= ((k >> bit) & 1) << (n - 1 - bit)
    return r


def fft_lines(re, im, T, inverse):
    """FFT of the header along the last axis of re, im [..., P] with the table T [P / 2, 2]."""
    P = re.shape[-1]
    n = P.bit_length() - 1
    assert 1 << n == P and T.shape == (max(P // 2, 1), 2) and T.dtype == F
    perm = bitrev(P)
    yr, yi = np.ascontiguousarray(re[..., perm], dtype=F), np.ascontiguousarray(im[..., perm], dtype=F)
    lead = yr.shape[:-1]
    for s in range(1, n + 1):
        h = 1 << (s - 1)
        step = P // (2 * h)
        wr, wi = T[np.arange(h) * step, 0], T[np.arange(h) * step, 1]
        if inverse:
            wi = -wi
        vr, vi = yr.reshape(lead + (P // (2 * h), 2, h)), yi.reshape(lead + (P // (2 * h), 2, h))
        ar, ai, br, bi = vr[..., 0, :], vi[..., 0, :], vr[..., 1, :], vi[..., 1, :]
        tr = (wr * br) - (wi * bi)
        ti = (wr * bi) + (wi * br)
        nr, ni = np.empty_like(vr), np.empty_like(vi)
        nr[..., 0, :], ni[..., 0, :] = ar + tr, ai + ti
        nr[..., 1, :], ni[..., 1, :] = ar - tr, ai - ti
        yr, yi = nr.reshape(lead + (P,)), ni.reshape(lead + (P,))
    return yr, yi


def _fft2(re, im, tx, ty, inverse, rows_first):
    def rows(re, im):
        return fft_lines(re, im, tx, inverse)

    def cols(re, im):
        r, i = fft_lines(np.ascontiguousarray(re.T), np.ascontiguousarray(im.T), ty, inverse)
        return np.ascontiguousarray(r.T), np.ascontiguousarray(i.T)
    for f in ((rows, cols) if rows_first else (cols, rows)):
        re, im = f(re, im)
    return re, im


def pad(qb, R, px, py, zero_border=False):
    """PAD: X [py, px] (the real part) of one bin qb [H, W]."""
    H, W = qb.shape
    X = np.zeros((py, px), dtype=F)
    ii, jj = np.arange(px), np.arange(py)
    i1, j1 = np.where(ii < W + R, ii, ii - px), np.where(jj < H + R, jj, jj - py)
    vi, vj = (i1 >= -R) & (i1 < W + R), (j1 >= -R) & (j1 < H + R)
    src = qb[np.clip(j1, 0, H - 1)[:, None], np.clip(i1, 0, W - 1)[None, :]]
    inside = vj[:, None] & vi[None, :]
    if zero_border:
        inside = inside & ((j1 >= 0) & (j1 < H))[:, None] & ((i1 >= 0) & (i1 < W))[None, :]
    X[inside] = src[inside]
    return X


def kernel(psf_b, R, px, py, correlation=False):
    """KERNEL: Kp [py, px] (the real part) of one bin's psf [K, K]."""
    Kp = np.zeros((py, px), dtype=F)
    d = np.arange(-R, R + 1)
    src = psf_b[::-1, ::-1] if correlation else psf_b
    Kp[(d % py)[:, None], (d % px)[None, :]] = src
    return Kp


def glare(q, R, px, py, on, psf, tx, ty, variant=None):
    """GLARE: q [H, W, B] float32 -> out [H, W, B] float32."""
    assert variant is None or variant in VARIANTS
    q = np.asarray(q, dtype=F)
    H, W, B = q.shape
    if variant == "px_halved":
        px = px // 2
        assert px >= W   # (the rules applied literally at the halved extent: the aprons and the psf's halves then overlap; where taps collide the last one written stays)
        tx = np.ascontiguousarray(tx[::2])
    out = q.copy()
    inv = F(1.0) / (F(px) * F(py))
    conj = variant != "twiddles_not_conjugated"
    for b in range(B):
        if not on[b]:
            continue
        X = pad(q[:, :, b], R, px, py, zero_border=variant == "zero_border")
        Kp = kernel(np.asarray(psf[b], dtype=F).reshape(2 * R + 1, 2 * R + 1), R, px, py, correlation=variant == "correlation")
        xr, xi = _fft2(X, np.zeros_like(X), tx, ty, False, True)
        kr, ki = _fft2(Kp, np.zeros_like(Kp), tx, ty, False, True)
        yr = (xr * kr) - (xi * ki)
        yi = (xr * ki) + (xi * kr)
        yr, yi = _fft2(yr, yi, tx, ty, conj, variant == "inverse_rows_first")
        out[:, :, b] = yr[:H, :W] * inv
    return out


def direct(q, R, on, psf):
    """The convolution with the replicated border, tap by tap in binary64: out(j, i) = sum psf(dy, dx) q(clamp(j - dy), clamp(i - dx)); `off` bins copied."""
    q64 = np.asarray(q, dtype=np.float64)
    H, W, B = q64.shape
    K = 2 * R + 1
    p = np.asarray(psf, dtype=np.float64).reshape(B, K, K) * (np.asarray(on) != 0)[:, None, None]
    e = np.pad(q64, ((R, R), (R, R), (0, 0)), mode="edge")
    out = np.zeros_like(q64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            out += e[R - dy:R - dy + H, R - dx:R - dx + W, :] * p[:, dy + R, dx + R]
    off = np.asarray(on) == 0
    out[:, :, off] = q64[:, :, off]
    return out
