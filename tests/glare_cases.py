"""The shared case list of the glare tests (include/ssx.h "Glare: per-bin convolution by FFT"): what tests/test_glare_gpu.py feeds ssx_glare_images and compares
with tests/glare_ref.py bit for bit, and what tests/test_glare_cpu.py holds against a direct binary64 convolution and against the definition's near misses.

The smallest shapes at which the kernels can still go wrong: 1 x 1; the aprons adjacent (W + 2 R = px); lines shorter and longer than a wave, non-square plans;
R larger than the image; an image that fits its plan exactly; the largest line (4096); every bin off.  Inputs are finite, uniform in 0.05 .. 4; the psf is
random, positive and NOT symmetric (a correlation differs); `on` is mixed per bin, and an `off` bin's psf is NaN: nobody may read it.  The twiddles are
ssh_glare_twiddles', except in one case whose tables are arbitrary, asymmetric and finite: an index or conjugation slip cannot hide behind a symmetry of the
cosine.  Each case's restatement is computed once (want) and shared."""
import functools

import numpy as np

import glare_ref as ref
from simple_spectral_amd.renderer import glare_plan, glare_twiddles

F = np.float32

#          name                 W     H   R   B   px    py   on         twiddles
SHAPES = (("1x1-r1-b4",         1,    1,  1,   4,    4,   4, "mixed", "host"),
          ("5x3-r1-b8",         5,    3,  1,   8,    8,   8, "mixed", "host"),
          ("6x5-r5-b4",         6,    5,  5,   4,   16,  16, "mixed", "host"),    # W + 2 R = px exactly: the aprons are adjacent
          ("7x5-r4-b20",        7,    5,  4,  20,   16,  16, "mixed", "host"),
          ("67x9-r12-b20",     67,    9, 12,  20,  128,  64, "mixed", "host"),    # non-square, lines longer than a wave
          ("300x3-r2-b8",     300,    3,  2,   8,  512,   8, "mixed", "host"),
          ("40x24-r100-b4",    40,   24, 100,  4,  256, 256, "mixed", "host"),    # R larger than the image
          ("1000x2-r12-b4",  1000,    2, 12,   4, 1024,  32, "mixed", "host"),    # fits exactly
          ("4000x1-r48-b4",  4000,    1, 48,   4, 4096, 128, "mixed", "host"),    # the largest line
          ("16x16-r3-b64-off", 16,   16,  3,  64,   32,  32, "off", "host"),      # every on[b] = 0
          ("7x5-r4-b20-any-tables", 7, 5, 4,  20,   16,  16, "mixed", "arbitrary"))


def _case(k, name, W, H, R, B, px, py, on_kind, tw_kind):
    g = np.random.default_rng(700 + k)
    assert glare_plan(W, H, R) == (px, py), name
    q = g.uniform(0.05, 4.0, size=(H, W, B)).astype(F)
    K = 2 * R + 1
    psf = g.uniform(0.1, 1.0, size=(B, K, K))
    psf = (psf / psf.sum(axis=(1, 2), keepdims=True)).astype(F)
    on = np.array([0 if on_kind == "off" else int(b % 3 != 1) for b in range(B)], dtype=np.uint8)
    psf[on == 0] = np.nan
    if tw_kind == "host":
        tx, ty = glare_twiddles(px), glare_twiddles(py)
    else:
        tx, ty = g.uniform(-1.0, 1.0, size=(px // 2, 2)).astype(F), g.uniform(-1.0, 1.0, size=(py // 2, 2)).astype(F)
    return {"name": name, "q": q, "R": R, "px": px, "py": py, "on": on, "psf": psf, "tx": tx, "ty": ty, "arbitrary": tw_kind != "host"}


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_case(k, *s) for k, s in enumerate(SHAPES))


def params_of(case):
    """the glare dict Renderer.glare_images takes (simple_spectral_amd.renderer.glare_aperture)"""
    return {"radius": case["R"], "px": case["px"], "py": case["py"], "on": case["on"], "psf": case["psf"], "twiddle_x": case["tx"], "twiddle_y": case["ty"]}


@functools.lru_cache(maxsize=None)
def _want(k, variant):
    c = cases()[k]
    out = ref.glare(c["q"], c["R"], c["px"], c["py"], c["on"], c["psf"], c["tx"], c["ty"], variant=variant)
    out.setflags(write=False)
    return out


def want(k, variant=None):
    """the restatement's result for case k, computed once; read-only"""
    return _want(k, variant)
