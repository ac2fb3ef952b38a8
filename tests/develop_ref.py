"""include/ssx.h "Developing the spectral bins" restated: the develop as a float32 loop over the bins (vectorised over pixels), the raw q from the sums, and
the weights in float64 with exact piecewise Simpson.  TEST INFRASTRUCTURE: nothing here calls the libraries, except `observer_tables` / `xyz_to_lrgb`, which only
fetch the tables the host loaded.  Python floats and numpy float64 are binary64 with IEEE + - * / and no contraction, so every line is one rounded operation."""
import math

import numpy as np


def develop(q, weights):
    """out[p][c] = sum_b q[p][b] * W[c][b]: acc = 0.0f; acc = acc + (q * W) for b ascending, the product rounded to binary32 before the add."""
    q = np.asarray(q, dtype=np.float32)
    w = np.asarray(weights, dtype=np.float32)
    C, B = w.shape
    assert q.shape[-1] == B
    out = np.zeros(q.shape[:-1] + (C,), dtype=np.float32)
    with np.errstate(all="ignore"):
        for c in range(C):
            acc = np.zeros(q.shape[:-1], dtype=np.float32)
            for b in range(B):
                prod = (q[..., b] * w[c, b]).astype(np.float32)
                acc = (acc + prod).astype(np.float32)
            out[..., c] = acc
    return out


def raw_q(sums, done_spp):
    """q[b] = (float)((S[b] * (double)M) / (double)n), M = B / 4: the multiply, then the divide, both binary64."""
    S = np.asarray(sums, dtype=np.float64)
    M = np.float64(S.shape[-1] // 4)
    with np.errstate(all="ignore"):
        return ((S * M) / np.float64(done_spp)).astype(np.float32)


# ---- the weights --------------------------------------------------------------------------------------------------------------------------------------------
# a table is (samples float32 [n], low, high), low and high binary32 values

def _delta(t):
    s, low, high = t
    return (float(np.float32(high)) - float(np.float32(low))) / float(len(s) - 1)


def table_at(t, lam):
    """T(lambda): pos = (lambda - low) / delta; i = floor(pos); f = pos - i; s(i) * (1 - f) + s(i + 1) * f, s = 0 outside the table."""
    s, low, _ = t
    pos = (lam - float(np.float32(low))) / _delta(t)
    base = math.floor(pos)
    if not (-1 <= base < len(s)):
        return 0.0
    f = pos - float(base)
    at = lambda k: float(s[k]) if 0 <= k < len(s) else 0.0
    return at(base) * (1.0 - f) + at(base + 1) * f


def _knots_inside(t, a, z):
    s, low, _ = t
    x = float(np.float32(low)) + np.arange(-1, len(s) + 1, dtype=np.float64) * _delta(t)
    return [float(v) for v in x[(x > a) & (x < z)]]


def table_integral(r, g, a, z):
    """Simpson on every piece between a, z and the knots of r (and g) strictly inside, pieces added in ascending order from 0.0."""
    x = sorted(set([a, z] + _knots_inside(r, a, z) + (_knots_inside(g, a, z) if g is not None else [])))
    F = (lambda lam: table_at(r, lam) * table_at(g, lam)) if g is not None else (lambda lam: table_at(r, lam))
    total = 0.0
    for p, q in zip(x[:-1], x[1:]):
        total += ((q - p) / 6.0) * ((F(p) + 4.0 * F(0.5 * (p + q))) + F(q))
    return total


def bin_edge(b, bins, lambda_min, lambda_step):
    return float(np.float32(lambda_min)) + float(b) * (float(np.float32(lambda_step)) / float(bins // 4))


def weights64(responses, bins, lambda_min, lambda_step, filter=None, gain=None, xyz_to_lrgb=None):
    """[C][B] float64 before the final rounding.  xyz_to_lrgb: the 9 floats of ssh_color_values("xyz_to_lrgb"), column-major."""
    C = len(responses)
    w = np.zeros((C, bins), dtype=np.float64)
    for b in range(bins):
        a, z = bin_edge(b, bins, lambda_min, lambda_step), bin_edge(b + 1, bins, lambda_min, lambda_step)
        for c in range(C):
            integral = table_integral(responses[c], filter, a, z)
            w[c, b] = float(gain[b]) * integral if gain is not None else integral
        if xyz_to_lrgb is not None:
            m = [float(v) for v in xyz_to_lrgb]
            X, Y, Z = float(w[0, b]), float(w[1, b]), float(w[2, b])
            for r in range(3):
                w[r, b] = (m[r] * X + m[3 + r] * Y) + m[6 + r] * Z
    return w


def weights(*args, **kw):
    return weights64(*args, **kw).astype(np.float32)


def relight_gain(old, new, bins, lambda_min, lambda_step):
    g = np.zeros(bins, dtype=np.float64)
    for b in range(bins):
        a, z = bin_edge(b, bins, lambda_min, lambda_step), bin_edge(b + 1, bins, lambda_min, lambda_step)
        den = table_integral(old, None, a, z)
        g[b] = 0.0 if den == 0.0 else table_integral(new, None, a, z) / den
    return g


def observer_tables(scene):
    """[(samples, low, high)] x 3: the x-bar, y-bar, z-bar tables of a simple_spectral_amd Scene (what the host loaded from data/)."""
    d = scene.desc.contents
    out = []
    for idx in (d.spec_xbar, d.spec_ybar, d.spec_zbar):
        sp = d.spectra[idx]
        out.append((np.array(d.samples[sp.offset:sp.offset + sp.n], dtype=np.float32), float(sp.low), float(sp.high)))
    return out


def table_extrema_over(t, a, z):
    """(min, max) of the piecewise-linear T over [a, z]: taken at a, z or a knot inside."""
    v = [table_at(t, x) for x in [a, z] + _knots_inside(t, a, z)]
    return min(v), max(v)


# ---- inputs at the edges of binary32, and the bound of the develop against the image -------------------------------------------------------------------------

def extreme_inputs(W, H, bins, channels, seed):
    """(q [H, W, bins], weights [channels, bins]) whose products and sums are denormal or overflow.  Rows of the image in four groups: q denormal, q about
    1e-20, q about +-1e30, q in [-4, 9]; weights: channel 0 ordinary, 1 denormal, 2 about 1e-20, 3 about 1e30, the rest ordinary (channels >= 4; fewer
    channels take the first of them)."""
    g = np.random.default_rng(seed)
    F = np.float32
    q = g.uniform(-4, 9, size=(H, W, bins)).astype(F)
    sign = lambda shape: np.where(g.integers(0, 2, size=shape) == 1, F(1), F(-1))
    rows = np.arange(H) % 4
    n = int((rows == 0).sum())
    q[rows == 0] = g.integers(1, 0x007FFFFF, size=(n, W, bins)).astype(np.uint32).view(F) * sign((n, W, bins))
    n = int((rows == 1).sum())
    q[rows == 1] = (g.uniform(0.5, 2, size=(n, W, bins)) * 1e-20).astype(F) * sign((n, W, bins))
    n = int((rows == 2).sum())
    big = (g.uniform(0.5, 2, size=(n, W, bins)) * 1e30).astype(F) * sign((n, W, 1))      # one sign per pixel: the sum is +inf or -inf ...
    big[0, 0, 0] = -big[0, 0, 0]                                                          # ... and in one pixel inf - inf
    q[rows == 2] = big
    w = g.uniform(-2, 3, size=(channels, bins)).astype(F)
    if channels > 1:
        w[1] = g.integers(1, 0x007FFFFF, size=bins).astype(np.uint32).view(F) * sign(bins)
    if channels > 2:
        w[2] = (g.uniform(0.5, 2, size=bins) * 1e-20).astype(F)
    if channels > 3:
        w[3] = (g.uniform(0.5, 2, size=bins) * 1e30).astype(F)
    return q, w


def bin_average_bound(flux, lam, q, w, w64, tables, bins, lambda_min, lambda_step, spp):
    """The bound of tests/test_develop_gpu.py test_raw_develop_under_the_renders_observer_is_the_image_up_to_the_bin_average, [H, W, 3]:
    (1/n) sum_k sum_i |f_ki| max over the bin of |bar_c - avg_b(bar_c)| lambda_step, plus the rounding slack (B + 4) 2^-23 sum_b |q_b W_cb|.  The
    derivation holds for any observer: `tables` are the render's own x-bar, y-bar, z-bar (observer_tables), w / w64 its develop weights."""
    from simple_spectral_amd.renderer import spectral_bin_index
    M = bins // 4
    dev = np.zeros((3, bins))
    for b in range(bins):
        a, z = bin_edge(b, bins, lambda_min, lambda_step), bin_edge(b + 1, bins, lambda_min, lambda_step)
        for c in range(3):
            avg = w64[c, b] / (z - a)
            lo, hi = table_extrema_over(tables[c], a, z)
            dev[c, b] = max(abs(hi - avg), abs(lo - avg))
    m = spectral_bin_index(lam, np.float32(lambda_min), np.float32(lambda_step), bins).astype(np.int64)
    bound = np.zeros(lam.shape[:2] + (3,))
    for i in range(4):
        f = np.abs(flux[..., i].astype(np.float64))
        for c in range(3):
            bound[..., c] += (f * dev[c][i * M + m]).sum(axis=2)
    bound *= lambda_step / spp
    slack = (bins + 4) * 2.0 ** -23 * np.einsum("hwb,cb->hwc", np.abs(q.astype(np.float64)), np.abs(w.astype(np.float64)))
    return bound + slack
