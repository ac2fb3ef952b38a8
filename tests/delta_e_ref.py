"""The colour difference of two developments (include/ssx.h, "Colour difference of two developments") restated in numpy binary64: Lab, dE*ab, CIEDE2000, the
ordered region walk, the hosts' derived figures and the development of a white.  The per-pixel part is the header's formula statement by statement (the device is
held to it within a bound); the region walk gives the device's bits when it is fed the device's own map."""
import numpy as np

NO_REGION = 255
KNEE = 216.0 / 24389.0
RAD = 0.017453292519943295
DEG = 57.29577951308232
K25_7 = 6103515625.0
GUARD_DEG = 1.0          # the guard around the branch points of CIEDE2000 (hue_guard)
FIGURES = ("mean", "rms", "max", "exceed", "coverage")


def _f(u):
    with np.errstate(invalid="ignore"):
        return np.where(u > KNEE, np.cbrt(u), u / (108.0 / 841.0) + 4.0 / 29.0)


def lab(xyz, white):
    """xyz float32 [..., 3], white float64 [3] -> (L, a, b) float64 [...]"""
    xyz = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    w = np.asarray(white, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy, fz = _f(xyz[..., 0] / w[0]), _f(xyz[..., 1] / w[1]), _f(xyz[..., 2] / w[2])
        return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def delta_e_ab(lab_a, lab_b):
    with np.errstate(invalid="ignore", over="ignore"):
        dL, da, db = lab_a[0] - lab_b[0], lab_a[1] - lab_b[1], lab_a[2] - lab_b[2]
        return np.sqrt((dL * dL + da * da) + db * db)


def _p7(c):
    c2 = c * c
    return ((c2 * c2) * c2) * c


def _hue(b, ap):
    h = np.arctan2(b, ap) * DEG
    h = np.where(h < 0.0, h + 360.0, h)
    return np.where((ap == 0.0) & (b == 0.0), 0.0, h)


def _primes(lab_a, lab_b):
    (L1, a1, b1), (L2, a2, b2) = lab_a, lab_b
    C1, C2 = np.sqrt(a1 * a1 + b1 * b1), np.sqrt(a2 * a2 + b2 * b2)
    m7 = _p7(0.5 * (C1 + C2))
    G = 0.5 * (1.0 - np.sqrt(m7 / (m7 + K25_7)))
    ap1, ap2 = (1.0 + G) * a1, (1.0 + G) * a2
    Cp1, Cp2 = np.sqrt(ap1 * ap1 + b1 * b1), np.sqrt(ap2 * ap2 + b2 * b2)
    return Cp1, Cp2, _hue(b1, ap1), _hue(b2, ap2)


def delta_e_00(lab_a, lab_b, parts=False):
    """CIEDE2000, kL = kC = kH = 1.  parts: also a dict of the intermediate terms (for the closed-form tests)."""
    (L1, a1, b1), (L2, a2, b2) = [tuple(np.asarray(v, dtype=np.float64) for v in s) for s in (lab_a, lab_b)]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Cp1, Cp2, h1, h2 = _primes((L1, a1, b1), (L2, a2, b2))
        dL, dC, P, d, s = L2 - L1, Cp2 - Cp1, Cp1 * Cp2, h2 - h1, h1 + h2
        grey, far = P == 0.0, np.abs(h1 - h2) > 180.0
        dh = np.where(grey, 0.0, np.where(~far, d, np.where(d > 180.0, d - 360.0, d + 360.0)))
        dH = (2.0 * np.sqrt(P)) * np.sin((0.5 * dh) * RAD)
        Lm, Cm = 0.5 * (L1 + L2), 0.5 * (Cp1 + Cp2)
        hm = np.where(grey, s, np.where(~far, 0.5 * s, np.where(s < 360.0, 0.5 * (s + 360.0), 0.5 * (s - 360.0))))
        T = (((1.0 - 0.17 * np.cos((hm - 30.0) * RAD)) + 0.24 * np.cos((2.0 * hm) * RAD)) + 0.32 * np.cos((3.0 * hm + 6.0) * RAD)) - 0.20 * np.cos((4.0 * hm - 63.0) * RAD)
        u = (hm - 275.0) / 25.0
        dtheta = 30.0 * np.exp(-(u * u))
        c7 = _p7(Cm)
        RC = 2.0 * np.sqrt(c7 / (c7 + K25_7))
        l50 = (Lm - 50.0) * (Lm - 50.0)
        SL, SC, SH = 1.0 + (0.015 * l50) / np.sqrt(20.0 + l50), 1.0 + 0.045 * Cm, 1.0 + (0.015 * Cm) * T
        RT = -np.sin((2.0 * dtheta) * RAD) * RC
        tl, tc, th = dL / SL, dC / SC, dH / SH
        out = np.sqrt(((tl * tl + tc * tc) + th * th) + (RT * tc) * th)
    if parts:
        return out, dict(Cp1=Cp1, Cp2=Cp2, h1=h1, h2=h2, dh=dh, hm=hm, SL=SL, SC=SC, SH=SH, RT=RT, T=T, dH=dH)
    return out


def hue_guard(lab_a, lab_b, guard=GUARD_DEG):
    """bool [...]: the pair lies within `guard` degrees of a branch point of CIEDE2000 -- C'1 C'2 == 0, ||h'1 - h'2| - 180| < guard, or |h'1 + h'2 - 360| < guard
    where |h'1 - h'2| > 180 -- where the formula jumps and a last-place difference in atan2 moves the result visibly.  Pairs with a non-finite term are not
    guarded: their pattern is compared exactly."""
    lab_a, lab_b = [tuple(np.asarray(v, dtype=np.float64) for v in s) for s in (lab_a, lab_b)]
    with np.errstate(invalid="ignore", over="ignore"):
        Cp1, Cp2, h1, h2 = _primes(lab_a, lab_b)
        gap = np.abs(h1 - h2)
        return (Cp1 * Cp2 == 0.0) | (np.abs(gap - 180.0) < guard) | ((gap > 180.0) & (np.abs(h1 + h2 - 360.0) < guard))


def maps(xyz_a, xyz_b, white_a, white_b):
    """-> (de float64 [H, W, 2] BEFORE the rounding to float, lab float64 [H, W, 6] before the rounding)"""
    la, lb = lab(xyz_a, white_a), lab(xyz_b, white_b)
    de = np.stack([delta_e_ab(la, lb), delta_e_00(la, lb)], axis=-1)
    return de, np.stack(la + lb, axis=-1)


def regions_walk(de, labels, R, t, order="rows", strict=True, square="double", finite_only=True):
    """The six region arrays of the float32 map de [H, W, 2]: (SUM f8, SSQ f8, MAX f4, NF u8, NX u8, EX u8), each [R, 2], in the header's order of additions.
    labels None: the whole image is region 0.  The keyword arguments select deliberately WRONG variants for the tests that show the inputs discriminate:
    order "columns" walks columns first, strict False counts v >= t, square "float" rounds the square to binary32, finite_only False lets every v into SUM."""
    de = np.asarray(de)
    assert de.dtype == np.float32 and de.ndim == 3 and de.shape[2] == 2
    H, W, _ = de.shape
    labels = np.zeros((H, W), dtype=np.uint8) if labels is None else np.asarray(labels, dtype=np.uint8)
    SUM, SSQ = np.zeros((R, 2)), np.zeros((R, 2))
    MAX = np.zeros((R, 2), dtype=np.float32)
    NF, NX, EX = (np.zeros((R, 2), dtype=np.uint64) for _ in range(3))
    if order == "columns":
        de, labels, H, W = de.transpose(1, 0, 2), labels.T, W, H
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            for k in range(2):
                for j in range(H):
                    s = q = 0.0
                    for i in np.nonzero(labels[j] == r)[0]:
                        v = de[j, i, k]
                        x = float(v)
                        fin = bool(np.isfinite(v))
                        if fin or not finite_only:
                            s += x
                            q += float(np.float32(v * v)) if square == "float" else x * x
                        if fin:
                            NF[r, k] += np.uint64(1)
                            if v > MAX[r, k]:
                                MAX[r, k] = v
                        else:
                            NX[r, k] += np.uint64(1)
                        if (x > t[k]) if strict else (x >= t[k]):
                            EX[r, k] += np.uint64(1)
                    SUM[r, k] += s
                    SSQ[r, k] += q
    return SUM, SSQ, MAX, NF, NX, EX


def derive(SUM, SSQ, MAX, NF, NX, EX):
    """The hosts' figures: a dict of float64 [R, 2] arrays mean, rms, max, exceed, coverage; NaN where the denominator is 0."""
    nf, nx = NF.astype(np.float64), NX.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nan = np.full(nf.shape, np.nan)
        some = nf > 0
        return dict(mean=np.where(some, SUM / nf, nan), rms=np.where(some, np.sqrt(SSQ / nf), nan), max=MAX.astype(np.float64),
                    exceed=np.where(some, EX.astype(np.float64) / nf, nan), coverage=np.where(nf + nx > 0, nf / (nf + nx), nan))


def develop_white(weights, bin_means):
    """out[c] = sum over b (ascending) of (double)W[c][b] * bin_means[b], bin_means the illuminant's mean over each bin (1.0: equal energy)"""
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    e = np.broadcast_to(np.asarray(bin_means, dtype=np.float64), (w.shape[1],))
    out = np.zeros(w.shape[0])
    for b in range(w.shape[1]):
        out = out + w[:, b] * e[b]
    return out


# ---- the bound: forward error propagation through the formula ---------------------------------------------------------------------------------------------

U = 2.0 ** -52     # one binary64 ulp, relative


class Err:
    """A binary64 value with a bound on |device - numpy| of it, propagated to first order through every operation of the formula: the partial derivatives
    times the operands' bounds, plus what the operation itself may differ by.  + - * / and sqrt are correctly rounded on both sides (half an ulp each: U
    together); a library function differs by `T` ulp: the device's documented (or assumed) error plus numpy's own 1 ulp."""
    T = 5.0

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _r(self, v, e, ulps=1.0):
        return Err(v, e + ulps * U * np.abs(v))

    def __add__(self, o):
        o = Err.of(o); return self._r(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o); return self._r(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Err.of(o) - self

    def __mul__(self, o):
        o = Err.of(o); return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.of(o); return self._r(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def __neg__(self):
        return Err(-self.v, self.e)

    def sqrt(self):
        """|sqrt(a + d) - sqrt(a)| <= min(|d| / sqrt(a), sqrt(|d|)): twice the first-order term away from 0, and finite at 0"""
        root = np.sqrt(self.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(self.e == 0.0, 0.0, np.minimum(self.e / root, np.sqrt(self.e)))
        return self._r(root, e)

    def fn(self, f, dabs):
        v = f(self.v)
        return self._r(v, dabs(self.v, v) * self.e, Err.T)


def _where(c, a, b):
    a, b = Err.of(a), Err.of(b)
    return Err(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def _err_f(u):
    with np.errstate(divide="ignore", invalid="ignore"):
        return _where(u.v > KNEE, u.fn(np.cbrt, lambda a, v: np.abs(v) / (3.0 * np.abs(a))), u / (108.0 / 841.0) + 4.0 / 29.0)


def _err_lab(xyz, w):
    x = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    fx, fy, fz = (_err_f(Err(x[..., c]) / float(w[c])) for c in range(3))
    return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def _err_atan2(y, x):
    v = np.arctan2(y.v, x.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r2 = x.v * x.v + y.v * y.v
        e = np.where(r2 > 0.0, (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / r2, 0.0)
    return Err(v, e + Err.T * U * np.abs(v))


def bounds(xyz_a, xyz_b, white_a, white_b):
    """(de_bound [H, W, 2], lab_bound [H, W, 6]): |device's float - this file's binary64 value| may reach this much -- twice the first-order propagated bound
    (the factor covers the second-order terms) plus one binary32 ulp of the value for the final rounding.  Meaningless inside hue_guard and for non-finite
    values, which the caller leaves out."""
    cos = lambda t: t.fn(np.cos, lambda a, v: 1.0)
    sin = lambda t: t.fn(np.sin, lambda a, v: 1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        A, B = _err_lab(xyz_a, white_a), _err_lab(xyz_b, white_b)
        (L1, a1, b1), (L2, a2, b2) = A, B
        dL, da, db = L1 - L2, a1 - a2, b1 - b2
        ab = ((dL * dL + da * da) + db * db).sqrt()

        def p7(c):
            c2 = c * c
            return ((c2 * c2) * c2) * c

        def hue(b, ap):
            h = _err_atan2(b, ap) * DEG
            h = _where(h.v < 0.0, h + 360.0, h)
            return _where((ap.v == 0.0) & (b.v == 0.0), 0.0, h)
        C1, C2 = (a1 * a1 + b1 * b1).sqrt(), (a2 * a2 + b2 * b2).sqrt()
        m7 = p7(0.5 * (C1 + C2))
        G = 0.5 * (1.0 - (m7 / (m7 + K25_7)).sqrt())
        ap1, ap2 = (1.0 + G) * a1, (1.0 + G) * a2
        Cp1, Cp2 = (ap1 * ap1 + b1 * b1).sqrt(), (ap2 * ap2 + b2 * b2).sqrt()
        h1, h2 = hue(b1, ap1), hue(b2, ap2)
        dLp, dC, P, d, s = L2 - L1, Cp2 - Cp1, Cp1 * Cp2, h2 - h1, h1 + h2
        grey, far = P.v == 0.0, np.abs(h1.v - h2.v) > 180.0
        dh = _where(grey, 0.0, _where(~far, d, _where(d.v > 180.0, d - 360.0, d + 360.0)))
        dH = (2.0 * P.sqrt()) * sin((0.5 * dh) * RAD)
        Lm, Cm = 0.5 * (L1 + L2), 0.5 * (Cp1 + Cp2)
        hm = _where(grey, s, _where(~far, 0.5 * s, _where(s.v < 360.0, 0.5 * (s + 360.0), 0.5 * (s - 360.0))))
        T = (((1.0 - 0.17 * cos((hm - 30.0) * RAD)) + 0.24 * cos((2.0 * hm) * RAD)) + 0.32 * cos((3.0 * hm + 6.0) * RAD)) - 0.20 * cos((4.0 * hm - 63.0) * RAD)
        u = (hm - 275.0) / 25.0
        dtheta = 30.0 * (-(u * u)).fn(np.exp, lambda a, v: np.abs(v))
        c7 = p7(Cm)
        RC = 2.0 * (c7 / (c7 + K25_7)).sqrt()
        l50 = (Lm - 50.0) * (Lm - 50.0)
        SL, SC, SH = 1.0 + (0.015 * l50) / (20.0 + l50).sqrt(), 1.0 + 0.045 * Cm, 1.0 + (0.015 * Cm) * T
        RT = -sin((2.0 * dtheta) * RAD) * RC
        tl, tc, th = dLp / SL, dC / SC, dH / SH
        e00 = (((tl * tl + tc * tc) + th * th) + (RT * tc) * th).sqrt()
        ulp32 = lambda v: np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
        de = np.stack([2.0 * ab.e + ulp32(ab.v), 2.0 * e00.e + ulp32(e00.v)], axis=-1)
        six = np.stack([2.0 * t.e + ulp32(t.v) for t in A + B], axis=-1)
    return de, six
