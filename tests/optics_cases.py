"""The shared case list of the lens tests (include/ssx.h "Developing through a lens"): what tests/test_optics_gpu.py feeds ssx_optics_images and compares with
tests/optics_ref.py bit for bit, and what tests/test_optics_cpu.py uses to show that those inputs tell the definition from its near misses.

Every image size, bin count, R, scale and centre the sizes and paths of the kernels make interesting appears at least once: 1 x 1; rows shorter than, equal to
and longer than a wave (7, 16, 67) and longer than a 256-lane chunk of (pixel, bin) elements (300 x 3, and every case with width * B > 256); B = 20 (256 is no
multiple of it: a chunk starts in the middle of a pixel); radii mixed per bin, with 0 and with r_b above the image's width; centres at the middle, at a
non-half-integer and outside the image; NaN, +-Inf, -0 and denormals in the input.  The taps are random, positive and NOT symmetric: a walk in descending order
meets other products first."""
import numpy as np

F = np.float32
SCALES = (1.0, 0.98, 1.03, 0.5, 1.5)


def _case(name, W, H, B, R, radii, scales, centre, specials, seed):
    g = np.random.default_rng(seed)
    q = g.uniform(0.05, 4.0, size=(H, W, B)).astype(F)
    flat = q.reshape(-1)
    if specials:
        at = g.permutation(flat.size)[:6]
        for k, v in zip(at, (np.nan, np.inf, -np.inf, -0.0, 1e-41, -3e-45)):   # (the last two are denormal in binary32)
            flat[k] = F(v)
    radius = np.array([radii[b % len(radii)] for b in range(B)], dtype=np.uint32)
    assert radius.max(initial=0) <= R
    scale = np.array([scales[b % len(scales)] for b in range(B)], dtype=F)
    taps = g.uniform(0.1, 1.0, size=(B, 2 * R + 1)).astype(F)
    for b in range(B):                                                        # normalised over the taps the bin visits; the rest is noise the kernels must not read,
        r = int(radius[b])                                                    # the centre tap of an r_b = 0 bin included
        if r == 0:
            continue
        taps[b, R - r:R + r + 1] = (taps[b, R - r:R + r + 1] / taps[b, R - r:R + r + 1].sum(dtype=np.float64)).astype(F)
    cx, cy = {"middle": (W / 2.0, H / 2.0), "odd": (W * 0.37 + 0.3, H * 0.61 + 0.2), "outside": (-3.25, H + 4.6)}[centre]
    return {"name": name, "q": q, "cx": float(F(cx)), "cy": float(F(cy)), "R": R, "scale": scale, "radius": radius, "taps": taps, "specials": specials}


def cases():
    mixed = SCALES
    return [
        _case("1x1-b4-r0", 1, 1, 4, 0, (0,), mixed, "middle", False, 1),
        _case("1x1-b8-r3", 1, 1, 8, 3, (0, 3, 1, 2), mixed, "odd", False, 2),
        _case("7x5-b8-r1", 7, 5, 8, 1, (1, 0, 1), mixed, "odd", False, 3),
        _case("7x5-b20-r12", 7, 5, 20, 12, (12, 0, 8, 3, 1), mixed, "outside", False, 4),
        _case("16x16-b64-r3", 16, 16, 64, 3, (3, 2, 0, 1, 3), mixed, "middle", True, 5),
        _case("16x16-b4-r12", 16, 16, 4, 12, (12, 5, 0, 9), (1.03, 1.0, 0.5, 0.98), "odd", False, 6),
        _case("67x9-b20-r3", 67, 9, 20, 3, (0, 3, 1, 2), mixed, "odd", True, 7),
        _case("67x9-b64-r12", 67, 9, 64, 12, (12, 0, 1, 7, 11, 4), mixed, "outside", True, 8),
        _case("300x3-b8-r12", 300, 3, 8, 12, (12, 3, 0, 6), mixed, "middle", False, 9),
        _case("300x3-b4-r1", 300, 3, 4, 1, (1, 0), (0.98, 1.5, 1.0, 1.03), "odd", True, 10),
        _case("300x3-b64-r0", 300, 3, 64, 0, (0,), mixed, "outside", False, 11),
        _case("16x16-b20-identity", 16, 16, 20, 3, (0,), (1.0,), "middle", True, 12),
        _case("67x9-b8-blur-only", 67, 9, 8, 3, (3, 0, 2), (1.0,), "middle", True, 13),
    ]


def params_of(case):
    """the lens dict Renderer.optics_images takes (simple_spectral_amd.renderer.lens_optics)"""
    return {"cx": case["cx"], "cy": case["cy"], "max_radius": case["R"], "scale": case["scale"], "radius": case["radius"], "taps": case["taps"]}
