"""The shared case list of the sensor tests (tests/test_sensor_cpu.py, tests/test_sensor_gpu.py): images 3 x 3, 7 x 5 and 37 x 23 (odd sizes put every phase on
every border; 23 rows are two tiles of the demosaic kernel) and 131 x 19 (three tiles across, the last one ragged), bins 4, 16 and 64, the four Bayer patterns,
both demosaic methods; noise, ADC, both and neither; and q at the edges of binary32.  Seeded: every process builds the same list."""
import numpy as np

import sensor_ref as ref

F = np.float32
SIZES = ((3, 3), (7, 5), (37, 23))                                                # (W, H)
BINS = (4, 16, 64)
MODES = ("plain", "noise", "adc", "noise+adc")


def scales(mode, k):
    """a sensor's scalar fields: 900 .. 1500 electrons per unit of the develop, a 10- or 12-bit ADC above a black level"""
    s = dict(exposure=F(900.0 + 150.0 * (k % 5)), noise=0, seed=17 + k, frame=k % 3, read_var=F(0.0), dn_per_e=F(1.0), e_per_dn=F(1.0), black=F(0.0), white=F(0.0))
    s["inv_exposure"] = F(1.0) / s["exposure"]
    if "noise" in mode:
        s["noise"], s["read_var"] = 1, F(6.25)
    if "adc" in mode:
        white, black = F(1023.0 if k % 2 else 4095.0), F(64.0)
        full_well = s["exposure"] * F(2.5)
        s.update(white=white, black=black, dn_per_e=(white - black) / full_well, e_per_dn=full_well / (white - black))
    return {n: (float(v) if isinstance(v, np.floating) else v) for n, v in s.items()}


def cases():
    out = []
    k = 0
    for (W, H) in SIZES + ((131, 19),):
        for B in BINS:
            g = np.random.default_rng(1000 + k)
            pattern, method, mode = ref.PATTERNS[k % 4], ("mhc", "bilinear")[(k // 2) % 2], MODES[k % 4]
            cfa, taps = ref.bayer(pattern, method)
            c = dict(name="%dx%d-b%d-%s-%s-%s" % (W, H, B, pattern, method, mode), q=g.uniform(0.0, 2.5, size=(H, W, B)).astype(F),
                     weights=g.uniform(0.0, 1.0 / B, size=(3, B)).astype(F) * np.array([[1.0], [1.4], [0.8]], dtype=F), cfa=cfa, taps=taps,
                     ccm=(np.eye(3) + g.uniform(-0.3, 0.3, size=(3, 3))).astype(F), **scales(mode, k))
            out.append(c)
            k += 1
    out.append(edge_case(7, 5, 16, "plain"))
    out.append(edge_case(37, 23, 4, "noise+adc"))
    return out


def edge_case(W, H, B, mode):
    """NaN, +-inf, -0 and denormals in q, weights of both signs so that v is negative in places; the clamp of the ADC and max(e, 0) under the root both bite"""
    g = np.random.default_rng(W * H + B)
    q = g.uniform(-2.0, 2.5, size=(H, W, B)).astype(F)
    flat = q.reshape(-1)
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000007, 0x80000001, 0x007FFFFF], dtype=np.uint32).view(F)
    at = g.choice(flat.size, size=3 * special.size, replace=False)
    flat[at] = np.tile(special, 3)
    q[H // 2, :, :] = (g.integers(1, 0x007FFFFF, size=(W, B)).astype(np.uint32).view(F))          # a row of denormals
    q[0, 0, :] = -np.abs(q[0, 0, :])                                                               # a corner that is negative whatever its filter
    cfa, taps = ref.bayer("GBRG", "mhc")
    w = g.uniform(-0.2, 1.0, size=(3, B)).astype(F)
    return dict(name="edges-%dx%d-b%d-%s" % (W, H, B, mode), q=q, weights=w, cfa=cfa, taps=taps, ccm=(np.eye(3) + g.uniform(-0.3, 0.3, size=(3, 3))).astype(F),
                **scales(mode, 3))


def sensor_of(case):
    """the dict Renderer.sensor_images / demosaic_images / develop(sensor=) take"""
    return {k: v for k, v in case.items() if k not in ("name", "q")}
