"""The shared case list of the display tests (tests/test_display_cpu.py, tests/test_display_gpu.py).  Seeded: every process builds the same list.
METER: 1 x 1; 67 x 5 (odd, under one workgroup of 2048 pixels); 300 x 9 (two workgroups per quantity: the flush adds onto another's counts); 256 x 64 of one
value (16 384 in one key: the wave's aggregation, eight workgroups); every special class, subnormals, the patterns k << 19 and (k << 19) - 1, the largest finite
value; masks with zeros and of nothing but zeros.
LOCAL: 3 x 3 with r = 1; 5 x 4 with r = 8 (the window wider than the image); 65 x 17 and 130 x 35 (one and three tiles across with a ragged one; two and three
column tiles of 16 rows, five and nine row tiles of 4) with r in {1, 4, 32}; NaN, +-inf, negative, zero, values below y_lo and above y_hi; compress = boost = 1;
the constant image y * exposure = 4.
TONE: 1 x 1, 67 x 5, 300 x 9; shift 12, 19, 23; lo, hi, beyond both, NaN, -0, negatives, nodes (f = 0), f at its maximum, the last segment; with and without a
local gain; a matrix that is not the identity; a table with negative and non-monotone entries."""
import numpy as np

import display_ref as ref

F = np.float32
U = np.uint32
LUMA = np.array([0.2126, 0.7152, 0.0722], dtype=F)
SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xBF800000, 0x80000001, 0x00000001, 0x007FFFFF,
                    0x00080000, 0x0007FFFF, 0x7F7FFFFF, 0x7F780000, 0x7F77FFFF], dtype=U)


def log_uniform(g, shape, lo=-14.0, hi=10.0):
    return np.exp2(g.uniform(lo, hi, size=shape)).astype(F)


def edge_values():
    """the special patterns, and for several keys k the patterns k << 19 and (k << 19) - 1"""
    keys = np.array([1, 15, 16, 17, 1000, 2031, 2032, 2033, 2047, 2048, 4079], dtype=U)
    return np.concatenate([SPECIAL, keys << U(19), (keys << U(19)) - U(1)]).view(F)


def meter_cases():
    out = []
    g = np.random.default_rng(2601)
    out.append(dict(name="1x1", img=np.array([[[0.25, 1.5, 3.0e-3]]], dtype=F), luma=LUMA, mask=None))
    img = log_uniform(g, (5, 67, 3))
    ev = edge_values()
    flat = img.reshape(-1)
    flat[g.choice(flat.size, size=2 * ev.size, replace=False)] = np.tile(ev, 2)
    img[2, :, :] = g.integers(1, 0x007FFFFF, size=(67, 3)).astype(U).view(F)                  # a row of subnormals
    mask = (g.uniform(size=(5, 67)) < 0.7).astype(np.uint8) * np.uint8(3)
    out.append(dict(name="67x5-edges", img=img, luma=LUMA, mask=None))
    out.append(dict(name="67x5-edges-mask", img=img, luma=LUMA, mask=mask))
    out.append(dict(name="67x5-mask-of-zeros", img=img, luma=LUMA, mask=np.zeros((5, 67), dtype=np.uint8)))
    img = log_uniform(g, (9, 300, 3))
    img[g.uniform(size=(9, 300)) < 0.05] = -img[0, 0]
    out.append(dict(name="300x9", img=img, luma=LUMA, mask=None))
    out.append(dict(name="300x9-mask", img=img, luma=np.array([0.0, 1.0, 0.0], dtype=F), mask=(g.uniform(size=(9, 300)) < 0.5).astype(np.uint8)))
    out.append(dict(name="256x64-one-value", img=np.full((64, 256, 3), 0.7315, dtype=F), luma=LUMA, mask=None))
    return out


def local_cases():
    out = []
    g = np.random.default_rng(2602)

    def case(name, W, H, r, edges=False, **kw):
        img = log_uniform(g, (H, W, 3), -8.0, 8.0)
        if edges:
            flat = img.reshape(-1)
            vals = np.concatenate([SPECIAL.view(F), np.array([1.0e-9, 3.0e-8, 5.0e7, 3.0e9, -2.0, 0.0], dtype=F)])
            flat[g.choice(flat.size, size=min(vals.size, flat.size // 2), replace=False)] = vals[:min(vals.size, flat.size // 2)]
        p = dict(exposure=0.75, y_lo=2.0 ** -20, y_hi=2.0 ** 20, eps=0.25, pivot=-2.5, compress=0.5, boost=1.25)
        p.update(kw)
        return dict(name=name, img=img, luma=LUMA, radius=r, **p)

    out.append(case("3x3-r1", 3, 3, 1, edges=True))
    out.append(case("5x4-r8", 5, 4, 8, edges=True))
    for (W, H) in ((65, 17), (130, 35)):
        for r in (1, 4, 32):
            out.append(case("%dx%d-r%d" % (W, H, r), W, H, r, edges=(r != 4), eps=(0.25, 0.01, 1.0)[r % 3]))
    out.append(case("65x17-r4-identity", 65, 17, 4, compress=1.0, boost=1.0))
    c = constant_case()
    out.append(c)
    return out


def constant_case():
    """y * exposure = 4 everywhere: L = 2, every sum is exact, base = 2 and the gain is E((2 - pivot) * compress + pivot - 2)"""
    return dict(name="130x35-r32-constant", img=np.full((35, 130, 3), 8.0, dtype=F), luma=np.array([0.25, 0.5, 0.25], dtype=F), radius=32, exposure=0.5,
                y_lo=2.0 ** -20, y_hi=2.0 ** 20, eps=0.25, pivot=-2.5, compress=0.5, boost=1.25)


def local_params(case):
    """what display_ref.local and Renderer.local_images take besides the image and luma"""
    return {k: case[k] for k in ("radius", "exposure", "y_lo", "y_hi", "eps", "pivot", "compress", "boost")}


def wild_curve(g, n):
    """finite, with negative and non-monotone entries"""
    return (g.uniform(-1.0, 2.0, size=n) * np.where(np.arange(n) % 7 == 3, -3.0, 1.0)).astype(F)


def tone_cases():
    out = []
    g = np.random.default_rng(2603)
    ranges = {12: (2.0 ** -4, 8.0), 19: (2.0 ** -12, 10.0), 23: (2.0 ** -12, 16.0)}          # (lo, hi): 14338, 246 and 18 entries; 10.0 is on no node
    k = 0
    for (W, H) in ((1, 1), (67, 5), (300, 9)):
        for shift in (12, 19, 23):
            lo, hi = ranges[shift]
            n = ref.curve_len(lo, hi, shift)
            nd = ref.nodes(lo, hi, shift)
            ub = nd.view(U)
            lh = np.array([lo, hi], dtype=F)
            crafted = np.concatenate([
                lh, (lh.view(U) + np.array([-1, 1]).astype(U)).view(F), np.array([hi * 4.0, lo / 4.0, -0.0, -1.5], dtype=F), SPECIAL.view(F),
                nd[:8], nd[n // 2:n // 2 + 4], nd[-3:-1],                                          # nodes: f = 0
                (ub[1:6] - U(1)).view(F), (ub[-2:-1] - U(1)).view(F),                              # f at its maximum
                (lh.view(U)[1:] - U(1)).view(F), ((ub[-2:-1] + lh.view(U)[1:]) // U(2)).view(F)])  # the last segment, where idx + 1 is the table's last entry
            img = log_uniform(g, (H, W, 3), np.log2(lo) - 2.0, np.log2(hi) + 2.0)
            plain = k % 3 == 0 or (W, H) == (67, 5) and shift == 19
            if W * H > 1:
                flat = img.reshape(-1)
                m = min(crafted.size, flat.size // 2)
                if plain:                                                                      # identity matrix, unit gains: put the crafted values on finite pixels
                    img[0, :, :] = 1.0
                    img[0, :m if m < W else W, 0] = crafted[:m if m < W else W]
                    if H > 1 and m > W:
                        img[1, :, :] = 1.0
                        img[1, :min(m - W, W), 0] = crafted[W:W + min(m - W, W)]
                else:
                    flat[g.choice(flat.size, size=m, replace=False)] = crafted[:m]
            else:
                img[0, 0] = np.array([nd[1], hi, lo / 2], dtype=F) if shift == 12 else np.array([(ub[3:4] - U(1)).view(F)[0], np.nan, hi * 2], dtype=F)
            c = dict(name="%dx%d-s%d-%s" % (W, H, shift, "plain" if plain else "full"), img=img, lo=lo, hi=hi, shift=shift, curve=wild_curve(g, n),
                     gains=np.ones(3, dtype=F) if plain else g.uniform(0.5, 2.0, size=3).astype(F),
                     matrix=np.eye(3, dtype=F) if plain else (np.eye(3) + g.uniform(-0.4, 0.4, size=(3, 3))).astype(F),
                     local=None if k % 2 == 0 else log_uniform(g, (H, W), -2.0, 2.0))
            if plain and W * H > 1:
                c["matrix"] = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0]], dtype=F)                 # every output channel sees channel 0
                c["local"] = None
            out.append(c)
            k += 1
    return out


def tone_params(case):
    return {k: case[k] for k in ("lo", "hi", "shift", "gains", "matrix", "local")}
