"""include/ssx.h "Developing onto a sensor" restated in numpy, to the same bits: SENSOR (mosaic, electrons, noise, ADC) and DEMOSAIC (5 x 5 tables per phase
and channel, mirrored border, 3 x 3 matrix), and include/ssx_host.h's Bayer tables.  TEST INFRASTRUCTURE: nothing here calls the libraries.  Every line on
float32 arrays is one rounded binary32 operation (numpy does not contract); the hash is uint32 arithmetic, which wraps."""
import numpy as np

F = np.float32
U = np.uint32


def hash32(x):
    """h(x) of the header on uint32 arrays"""
    x = np.asarray(x, dtype=U).copy()
    x ^= x >> U(16)
    x *= U(0x7feb352d)
    x ^= x >> U(15)
    x *= U(0x846ca68b)
    x ^= x >> U(16)
    return x


def normal(p, seed, frame):
    """z(p) for an array of pixel indices: the sum of the twelve 16-bit halves of u_0 .. u_5, centred and scaled -- both float operations are exact"""
    with np.errstate(over="ignore"):
        base = hash32(hash32(U(seed)) + U(frame))
        hp = hash32(base + np.asarray(p, dtype=U))
        S = np.zeros(hp.shape, dtype=U)
        for k in range(6):
            u = hash32(hp + U(k))
            S += (u & U(0xFFFF)) + (u >> U(16))
    return ((S.astype(F) - F(393210.0)) * F(1.52587890625e-05)).astype(F)


def fmax(a, b):
    """max(a, b) = a > b ? a : b (a NaN a gives b)"""
    return np.where(a > b, a, b).astype(F)


def fmin(a, b):
    return np.where(a < b, a, b).astype(F)


def cfa_map(cfa, H, W):
    j, i = np.mgrid[0:H, 0:W]
    return np.asarray(cfa, dtype=np.int64)[(j & 1) * 2 + (i & 1)]


def sensor(q, weights, cfa, exposure=1.0, inv_exposure=1.0, noise=0, seed=0, frame=0, read_var=0.0, dn_per_e=1.0, e_per_dn=1.0, black=0.0, white=0.0, **_):
    """SENSOR: q [H, W, B], weights [3, B] -> (raw [H, W], dn [H, W] or None without an ADC)"""
    q = np.asarray(q, dtype=F)
    w = np.asarray(weights, dtype=F)
    H, W, B = q.shape
    c = cfa_map(cfa, H, W)
    wc = w[c]                                                                     # [H, W, B]: each photosite's own filter
    with np.errstate(all="ignore"):
        v = np.zeros((H, W), dtype=F)
        for b in range(B):
            v = (v + (q[..., b] * wc[..., b]).astype(F)).astype(F)
        e = (v * F(exposure)).astype(F)
        if noise:
            p = (np.arange(H, dtype=U)[:, None] * U(W) + np.arange(W, dtype=U)[None, :]).astype(U)
            sd = np.sqrt((fmax(e, F(0.0)) + F(read_var)).astype(F)).astype(F)
            e = (e + (sd * normal(p, seed, frame)).astype(F)).astype(F)
        dn = None
        if white > 0:
            d = np.floor((((e * F(dn_per_e)).astype(F) + F(black)).astype(F) + F(0.5)).astype(F)).astype(F)
            d = fmin(fmax(d, F(0.0)), F(white))
            dn = d
            e = ((d - F(black)).astype(F) * F(e_per_dn)).astype(F)
        raw = (e * F(inv_exposure)).astype(F)
    return raw, dn


def mirror(k, n):
    """m(k, n) on integer arrays"""
    k = np.asarray(k)
    return np.where(k < 0, -k, np.where(k >= n, 2 * (n - 1) - k, k))


def demosaic(raw, taps, ccm, mutant=None):
    """DEMOSAIC: raw [H, W], taps [4, 3, 25], ccm [3, 3] -> [H, W, 3].  mutant "clamp": the border clamped instead of mirrored (a near miss for the tests)."""
    raw = np.asarray(raw, dtype=F)
    taps = np.asarray(taps, dtype=F).reshape(4, 3, 25)
    ccm = np.asarray(ccm, dtype=F).reshape(3, 3)
    H, W = raw.shape
    j, i = np.mgrid[0:H, 0:W]
    phase = (j & 1) * 2 + (i & 1)
    at = (lambda k, n: np.clip(k, 0, n - 1)) if mutant == "clamp" else mirror
    rgb = np.zeros((3, H, W), dtype=F)
    with np.errstate(all="ignore"):
        for c in range(3):
            acc = np.zeros((H, W), dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    src = raw[at(j + dy, H), at(i + dx, W)]
                    acc = (acc + (src * taps[phase, c, (dy + 2) * 5 + (dx + 2)]).astype(F)).astype(F)
            rgb[c] = acc
        out = np.zeros((H, W, 3), dtype=F)
        for c in range(3):
            acc = (F(0.0) + (rgb[0] * ccm[c, 0]).astype(F)).astype(F)
            acc = (acc + (rgb[1] * ccm[c, 1]).astype(F)).astype(F)
            out[..., c] = (acc + (rgb[2] * ccm[c, 2]).astype(F)).astype(F)
    return out


# ---- include/ssx_host.h's tables, from the published description ------------------------------------------------------------------------------------------

PATTERNS = ("RGGB", "BGGR", "GRBG", "GBRG")


def bayer(pattern, method):
    """(cfa uint32 [4], taps float32 [4, 3, 25]) as ssh_sensor_bayer defines them; method "mhc" or "bilinear".  Built here from 5 x 5 stencils written out in
    full, not from the library's rules."""
    cfa = np.array(["RGB".index(ch) for ch in pattern], dtype=U)
    e = lambda rows: np.array(rows, dtype=np.float64) / 8.0                       # [dy + 2][dx + 2]
    own = e([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 8, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    if method == "mhc":
        g_at_rb = e([[0, 0, -1, 0, 0], [0, 0, 2, 0, 0], [-1, 2, 4, 2, -1], [0, 0, 2, 0, 0], [0, 0, -1, 0, 0]])
        rb_at_g_row = e([[0, 0, 0.5, 0, 0], [0, -1, 0, -1, 0], [-1, 4, 5, 4, -1], [0, -1, 0, -1, 0], [0, 0, 0.5, 0, 0]])
        rb_at_br = e([[0, 0, -1.5, 0, 0], [0, 2, 0, 2, 0], [-1.5, 0, 6, 0, -1.5], [0, 2, 0, 2, 0], [0, 0, -1.5, 0, 0]])
    else:
        g_at_rb = e([[0, 0, 0, 0, 0], [0, 0, 2, 0, 0], [0, 2, 0, 2, 0], [0, 0, 2, 0, 0], [0, 0, 0, 0, 0]])
        rb_at_g_row = e([[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 4, 0, 4, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
        rb_at_br = e([[0, 0, 0, 0, 0], [0, 2, 0, 2, 0], [0, 0, 0, 0, 0], [0, 2, 0, 2, 0], [0, 0, 0, 0, 0]])
    taps = np.zeros((4, 3, 25), dtype=F)
    for phase in range(4):
        s = int(cfa[phase])
        for c in range(3):
            if c == s:
                k = own
            elif c == 1:
                k = g_at_rb
            elif s == 1:
                k = rb_at_g_row if int(cfa[phase ^ 1]) == c else rb_at_g_row.T
            else:
                k = rb_at_br
            taps[phase, c] = k.reshape(25).astype(F)
    return cfa, taps


IDENTITY_TAPS = np.zeros((4, 3, 25), dtype=F)
IDENTITY_TAPS[:, :, 12] = 1.0
IDENTITY_CCM = np.eye(3, dtype=F)
