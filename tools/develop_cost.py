#!/usr/bin/env python3
"""Cost of ssx_spectral_develop on the headline image size (cornell-srgb 512^2, crystal-lizard-512): milliseconds per call for the raw and the denoised source,
C = 3 and C = 12 output channels, alternating between the cases in one process and on one context; `out` is NULL, so nothing is copied to the host (what is
timed is the upload of the 4 KB of weights, the kernels and the synchronisation).  The denoised source is read next to ssx_denoise_spectral alone in the same
loop: the difference is the develop kernel; the raw one next to the same call on an 8 x 8 image, which is all overhead.  Medians of wall-clock times per call, and the bytes per second the raw develop's compulsory traffic (8 B bytes of
sums read, 4 C written per pixel) implies.  Prints one JSON line.      python tools/develop_cost.py [--calls 64] [--bins 64] [--res 512] [--spp 16]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd.renderer import develop_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=64)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, spp_per_launch=max(1, a.spp // 4), texture="crystal-lizard-512.png"))
    r.set_noise_estimate(True)
    r.set_spectral_bins(a.bins)
    r.render_start(); r.render_wait()
    d = r.scene.desc.contents
    w3 = develop_weights(a.bins, d.lambda_min, d.lambda_step)
    weights = {3: w3, 12: np.ascontiguousarray(np.tile(w3, (4, 1)))}
    dp = r._denoise_params(5, 1.0, 0.1)

    def call(kind):
        source, channels = kind
        t = time.perf_counter()
        if source == "filter":
            r._check(r._lib.ssx_denoise_spectral(r._ctx, ctypes.byref(dp), None, None, None))
        else:
            w = weights[channels]
            r._check(r._lib.ssx_spectral_develop(r._ctx, ctypes.byref(dp) if source == "denoised" else None, w.ctypes.data, channels, None))
        return (time.perf_counter() - t) * 1e3

    # what a call costs beyond its kernel (weights upload, launch, synchronisation): the same raw call on an 8 x 8 image of a second context
    tiny = Renderer(Options(scene_name="cornell-srgb", res=(8, 8), spp=a.spp, spp_per_launch=max(1, a.spp // 4), texture="crystal-lizard-512.png"))
    tiny.set_spectral_bins(a.bins)
    tiny.render_start(); tiny.render_wait()

    def call_tiny():
        t = time.perf_counter()
        tiny._check(tiny._lib.ssx_spectral_develop(tiny._ctx, None, w3.ctypes.data, 3, None))
        return (time.perf_counter() - t) * 1e3

    kinds = (("raw", 3), ("raw", 12), ("denoised", 3), ("denoised", 12), ("filter", 0))
    for k in kinds + kinds:  # warm-up: guides, buffers
        call(k)
    ms = {k: [] for k in kinds}
    floor = [call_tiny() for _ in range(4)][:0]
    for _ in range(a.calls):
        for k in kinds:
            ms[k].append(call(k))
        floor.append(call_tiny())
    summary = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
    pixels = a.res * a.res
    out = {"image": "cornell-srgb %d^2" % a.res, "bins": a.bins}
    for (source, channels), v in ms.items():
        out["%s_C%d" % (source, channels) if channels else "denoise_spectral_alone"] = summary(v)
    out["call_on_8x8_image"] = summary(floor)
    for channels in (3, 12):
        must = pixels * (8 * a.bins + 4 * channels)
        out["raw_C%d_bytes" % channels] = must
        out["raw_C%d_GBps_at_median" % channels] = round(must / statistics.median(ms[("raw", channels)]) / 1e6, 1)
        out["raw_C%d_GBps_at_median_minus_8x8_call" % channels] = round(must / max(1e-6, statistics.median(ms[("raw", channels)]) - statistics.median(floor)) / 1e6, 1)
        out["denoised_C%d_minus_filter_ms" % channels] = round(statistics.median(ms[("denoised", channels)]) - statistics.median(ms[("filter", 0)]), 4)
    out["streaming_rate_GBps_float4_copy"] = 6290
    print(json.dumps(out))


if __name__ == "__main__":
    main()
