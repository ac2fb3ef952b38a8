"""include/ssx.h "Finishing a development for a display" restated in numpy, to the same bits: METER (integer histograms of sixteen keys per octave), LOCAL (the
integer log-luminance, a self-guided filter of box sums in a fixed order, the compression, the integer exponential) and TONE (gains, matrix, table).  TEST
INFRASTRUCTURE: nothing here calls the libraries.  Every line on float32 arrays is one rounded binary32 operation (numpy does not contract); keys, L and E go
through integer views of the bit patterns."""
import numpy as np

F = np.float32
U = np.uint32
I = np.int32
KEYS = 4096


def fmax(a, b):
    """max(a, b) = a > b ? a : b (a NaN a gives b)"""
    return np.where(a > b, a, b).astype(F)


def fmin(a, b):
    return np.where(a < b, a, b).astype(F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def frombits(u):
    return np.ascontiguousarray(u, dtype=U).view(F)


def luminance(img, luma):
    img, luma = np.asarray(img, dtype=F), np.asarray(luma, dtype=F)
    with np.errstate(all="ignore"):
        y = (F(0.0) + (img[..., 0] * luma[0]).astype(F)).astype(F)
        y = (y + (img[..., 1] * luma[1]).astype(F)).astype(F)
        return (y + (img[..., 2] * luma[2]).astype(F)).astype(F)


def meter(img, luma, mask=None):
    """METER: img [H, W, 3] -> (hist uint32 [4, 4096], special uint32 [4, 4])"""
    img = np.asarray(img, dtype=F)
    q = [img[..., 0], img[..., 1], img[..., 2], luminance(img, luma)]
    keep = np.ones(img.shape[:2], dtype=bool) if mask is None else np.asarray(mask) != 0
    hist, special = np.zeros((4, KEYS), dtype=U), np.zeros((4, 4), dtype=U)
    for k in range(4):
        u = bits(q[k])[keep]
        m = u & U(0x7FFFFFFF)
        zero, nan = m == 0, m > U(0x7F800000)
        neg = ~zero & ~nan & ((u >> U(31)) != 0)
        inf = u == U(0x7F800000)
        rest = ~(zero | nan | neg | inf)
        special[k] = [zero.sum(), neg.sum(), inf.sum(), nan.sum()]
        np.add.at(hist[k], (u[rest] >> U(19)).astype(np.int64), U(1))
    return hist, special


def log_l(img, luma, exposure, y_lo, y_hi):
    """L of the header: [H, W]"""
    with np.errstate(all="ignore"):
        yc = (luminance(img, luma) * F(exposure)).astype(F)
    yc = fmin(fmax(yc, F(y_lo)), F(y_hi))
    return (((bits(yc) >> U(7)).astype(I) - I(8323072)).astype(F) * F(2.0 ** -16)).astype(F)


def exp_e(d):
    """E(d) of the header"""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(d, dtype=F) * F(65536.0)).astype(F)).astype(F)
    f = fmin(fmax(f, F(-16777216.0)), F(16777216.0))
    key = f.astype(I) + I(8323072)
    key = np.minimum(np.maximum(key, I(0x10000)), I(0xFEFFFF))
    return frombits(key.astype(U) << U(7))


def box(P, r):
    """box(P) of the header: rows from 0.0f in ascending dx, then columns in ascending dy, the coordinates clamped"""
    P = np.asarray(P, dtype=F)
    H, W = P.shape
    ii, jj = np.arange(W), np.arange(H)
    h = np.zeros((H, W), dtype=F)
    for dx in range(-r, r + 1):
        h = (h + P[:, np.clip(ii + dx, 0, W - 1)]).astype(F)
    s = np.zeros((H, W), dtype=F)
    for dy in range(-r, r + 1):
        s = (s + h[np.clip(jj + dy, 0, H - 1), :]).astype(F)
    return s


def local(img, luma, radius, exposure=1.0, y_lo=2.0 ** -20, y_hi=2.0 ** 20, eps=0.25, pivot=0.0, compress=1.0, boost=1.0):
    """LOCAL: img [H, W, 3] -> (gain [H, W], base [H, W])"""
    r = int(radius)
    n = F((2 * r + 1) * (2 * r + 1))
    L = log_l(img, luma, exposure, y_lo, y_hi)
    with np.errstate(all="ignore"):
        S1, S2 = box(L, r), box((L * L).astype(F), r)
        m = (S1 / n).astype(F)
        v = fmax(((S2 / n).astype(F) - (m * m).astype(F)).astype(F), F(0.0))
        a = (v / (v + F(eps)).astype(F)).astype(F)
        b = (m - (a * m).astype(F)).astype(F)
        A, Bm = (box(a, r) / n).astype(F), (box(b, r) / n).astype(F)
        base = ((A * L).astype(F) + Bm).astype(F)
        t = (((base - F(pivot)).astype(F) * F(compress)).astype(F) + F(pivot)).astype(F)
        Lo = (t + ((L - base).astype(F) * F(boost)).astype(F)).astype(F)
        gain = exp_e((Lo - L).astype(F))
    return gain, base


def curve_len(lo, hi, shift):
    b = bits(np.array([lo, hi], dtype=F))
    return ((int(b[1]) - int(b[0])) >> int(shift)) + 2


def nodes(lo, hi, shift):
    """the table's nodes as float32 (the last may lie beyond hi)"""
    n = curve_len(lo, hi, shift)
    return frombits((int(bits(F(lo)).reshape(-1)[0]) + (np.arange(n, dtype=np.int64) << int(shift))).astype(U))


def tone(img, curve, lo, hi, shift, gains=(1.0, 1.0, 1.0), matrix=None, local=None):
    """TONE: img [H, W, 3] -> out [H, W, 3]"""
    img = np.asarray(img, dtype=F)
    curve = np.asarray(curve, dtype=F)
    M = np.eye(3, dtype=F) if matrix is None else np.asarray(matrix, dtype=F)
    g = np.asarray(gains, dtype=F)
    shift = int(shift)
    out = np.zeros(img.shape, dtype=F)
    with np.errstate(all="ignore"):
        v = [(img[..., c] * g[c]).astype(F) for c in range(3)]
        if local is not None:
            v = [(v[c] * np.asarray(local, dtype=F)).astype(F) for c in range(3)]
        for c in range(3):
            x = (F(0.0) + (v[0] * M[c, 0]).astype(F)).astype(F)
            x = (x + (v[1] * M[c, 1]).astype(F)).astype(F)
            x = (x + (v[2] * M[c, 2]).astype(F)).astype(F)
            xc = fmin(fmax(x, F(lo)), F(hi))
            k = bits(xc) - bits(F(lo)).reshape(-1)[0]
            idx = (k >> U(shift)).astype(np.int64)
            f = ((k & U((1 << shift) - 1)).astype(F) * F(2.0 ** -shift)).astype(F)
            c0, c1 = curve[idx], curve[idx + 1]
            out[..., c] = (c0 + ((c1 - c0).astype(F) * f).astype(F)).astype(F)
    return out


def same_bits(a, b):
    """the same bits, or a zero of the other sign; NaN exactly where the other has NaN"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))))
