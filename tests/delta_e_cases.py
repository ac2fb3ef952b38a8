"""The fixed-seed inputs of the colour-difference tests (tests/test_delta_e_cpu.py shows on the reference alone that they discriminate and that few of them lie
near a branch point; tests/test_delta_e_gpu.py runs the device on them)."""
import functools

import numpy as np

import delta_e_ref as ref

SEED = 20
CHUNK = 256                                           # pixels per chunk of ssx_delta_e_rows_kernel
WHITE_A = np.array([0.95047, 1.0, 1.08883])           # D65, Y = 1
WHITE_B = np.array([0.96422, 1.0, 0.82521])           # D50
THRESHOLDS = (2.3, 1.0)
SHAPES = ((1, 1), (42, 23), (CHUNK + 1, 1), (2 * CHUNK, 2))       # (W, H): one pixel; ragged tiles; the carry across a chunk; two full chunks and a second row


def lab_to_xyz(L, a, b, white):
    """the inverse of the header's Lab, rounded to float32: where the planted pairs come from"""
    fy = (L + 16.0) / 116.0
    fx, fz = fy + a / 500.0, fy - b / 200.0
    inv = lambda f: f ** 3 if f ** 3 > ref.KNEE else (f - 4.0 / 29.0) * (108.0 / 841.0)
    return (np.array([inv(fx), inv(fy), inv(fz)]) * white).astype(np.float32)


def polar(L, C, h, white):
    return lab_to_xyz(L, C * np.cos(np.radians(h)), C * np.sin(np.radians(h)), white)


def planted(white_a, white_b):
    """pairs (A, B) on both sides of every rule of the formula, and the special values"""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    p = lambda L1, C1, h1, L2, C2, h2: (polar(L1, C1, h1, white_a), polar(L2, C2, h2, white_b))
    f3 = lambda *v: np.array(v, dtype=np.float32)
    return [
        (f3(0, 0, 0), f3(0, 0, 0)),                                                     # exact zeros
        (f3(0.3, 0.4, 0.2), f3(0.3, 0.4, 0.2)),                                         # an equal pair (equal colours only under equal whites)
        (f3(-0.1, 0.2, 0.3), f3(0.2, -0.05, 0.1)),                                      # negative components
        (f3(inf, 0.2, 0.3), f3(0.2, 0.3, 0.1)), (f3(0.2, 0.3, 0.1), f3(0.1, inf, 0.3)), # +inf
        (f3(nan, 0.2, 0.3), f3(0.2, 0.3, 0.1)), (f3(0.2, 0.3, 0.1), f3(0.1, 0.2, nan)), # NaN
        p(50, 30, 10, 55, 35, 100),                                                     # |dh| < 180
        p(50, 30, 10, 55, 35, 200),                                                     # |dh| > 180, h1 + h2 < 360, d > 180
        p(50, 30, 200, 55, 35, 10),                                                     # the same with d < -180
        p(50, 30, 300, 55, 35, 100),                                                    # |dh| > 180, h1 + h2 >= 360
        p(50, 30, 200, 55, 35, 300),                                                    # |dh| < 180, h1 + h2 > 360
        (lab_to_xyz(50, 0, 0, white_a), polar(55, 30, 40, white_b)),                    # near C'1 C'2 = 0 (the rounding to float leaves a tiny chroma)
        (f3(*(0.004 * white_a)), f3(*(0.02 * white_b))),                                # f's knee: A below, B above
        (f3(*(0.004 * white_a)), f3(*(0.006 * white_b))),                               # both below
        p(20, 5, 275, 80, 90, 285),                                                     # the rotation term's peak, large chroma
    ]


@functools.lru_cache(maxsize=None)
def images(shape, equal_whites=False):
    """(xyz_a, xyz_b float32 [H, W, 3], white_a, white_b): three quarters of the pixels are a colour and a perturbation of it (what two developments of one render
    look like), a quarter are independent; in an image of 64 pixels or more the planted pairs stand at a stride through it.  Read-only."""
    W, H = shape
    rng = np.random.default_rng(SEED + 1000 * W + H)
    wa, wb = WHITE_A, (WHITE_A if equal_whites else WHITE_B)
    Y = rng.uniform(0.01, 1.2, (H, W, 1))
    a = (Y * rng.uniform(0.6, 1.4, (H, W, 3)) * wa).astype(np.float32)
    b = (a * rng.uniform(0.93, 1.07, (H, W, 3)) * (wb / wa)).astype(np.float32)
    free = rng.random((H, W)) < 0.25
    b[free] = (rng.uniform(0.01, 1.2, (int(free.sum()), 1)) * rng.uniform(0.6, 1.4, (int(free.sum()), 3)) * wb).astype(np.float32)
    if W * H >= 64:
        pairs = planted(wa, wb)
        at = (np.arange(len(pairs)) * (W * H // len(pairs)) + 3) % (W * H)
        for n, (pa, pb) in zip(at, pairs):
            a.reshape(-1, 3)[n], b.reshape(-1, 3)[n] = pa, pb
    for arr in (a, b):
        arr.setflags(write=False)
    return a, b, wa, wb


@functools.lru_cache(maxsize=None)
def labels(shape, R, full=False):
    """uint8 [H, W]: regions 0..R-2 and 255 at random, region R - 1 without a pixel (R > 1; R = 1: region 0 and 255); full: every region 0..R-1 and 255.  In an
    image of several rows one row belongs to no region and another to region 0 alone, so that rows without a pixel of a region exist at every R."""
    W, H = shape
    rng = np.random.default_rng(SEED + 7 * R + W + full)
    pool = np.array(list(range(R if full else max(R - 1, 1))) + [255], dtype=np.uint8)
    lab = pool[rng.integers(0, pool.size, (H, W))]
    if H > 2:
        lab[H // 2] = 255
        lab[H // 3] = 0
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def reference(shape, equal_whites=False):
    """(de float64 [H, W, 2], lab float64 [H, W, 6], guard bool [H, W], de_bound, lab_bound) of images(shape): computed once, read-only"""
    a, b, wa, wb = images(shape, equal_whites)
    de, six = ref.maps(a, b, wa, wb)
    guard = ref.hue_guard(ref.lab(a, wa), ref.lab(b, wb))
    db, lb = ref.bounds(a, b, wa, wb)
    for arr in (de, six, guard, db, lb):
        arr.setflags(write=False)
    return de, six, guard, db, lb
