#!/usr/bin/env python3
"""Cost of ssx_denoise on the headline image size (cornell-srgb 512^2, crystal-lizard-512): milliseconds per call with L levels, next to the same call with one
level, alternating between the two in one process and on one context (the guide buffers are cached after the first call, the buffers allocated: what is timed
is the variance kernel, the L launches of ssx_atrous_kernel, the synchronisation and -- asked for with --read-back -- the copy of the image to the host).
Medians of wall-clock times per call; the figure is to be read next to the render time of the headline workload (21.3 ms).
Prints one JSON line.      python tools/denoise_cost.py [--calls 64] [--levels 5] [--res 512] [--spp 16]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--read-back", action="store_true")
    a = ap.parse_args()
    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, spp_per_launch=max(1, a.spp // 4), texture="crystal-lizard-512.png"))
    r.set_noise_estimate(True)
    r.render_start(); r.render_wait()
    import numpy as np
    out = np.zeros((a.res, a.res, 4), dtype=np.float32)
    dst = out.ctypes.data if a.read_back else None

    def call(levels):
        p = r._denoise_params(levels, 1.0, 0.1)
        t = time.perf_counter()
        r._check(r._lib.ssx_denoise(r._ctx, ctypes.byref(p), dst, None))
        return (time.perf_counter() - t) * 1e3

    t0 = time.perf_counter(); r.guides(); guides_ms = (time.perf_counter() - t0) * 1e3   # first call: the guides kernel and the copies to the host
    for levels in (1, a.levels, 1, a.levels):  # warm-up
        call(levels)
    ms = {1: [], a.levels: []}
    for _ in range(a.calls):
        for levels in (1, a.levels):
            ms[levels].append(call(levels))
    summary = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
    per_level = (statistics.median(ms[a.levels]) - statistics.median(ms[1])) / max(1, a.levels - 1)
    pixels = a.res * a.res
    print(json.dumps({"image": "cornell-srgb %d^2" % a.res, "levels": a.levels, "read_back": bool(a.read_back), "denoise": summary(ms[a.levels]), "one_level": summary(ms[1]),
                      "ms_per_further_level": round(per_level, 4), "guides_first_call_ms": round(guides_ms, 3),
                      "bytes_per_level_compulsory": pixels * 60, "bytes_per_level_gathered": pixels * (25 * 40 + 9 * 20 + 20),
                      "headline_render_ms_parent": 21.3}))


if __name__ == "__main__":
    main()
