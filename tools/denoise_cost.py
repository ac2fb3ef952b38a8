#!/usr/bin/env python3
"""Cost of ssx_denoise on the headline image size (cornell-srgb 512^2, crystal-lizard-512): milliseconds per call with L levels, next to the same call with one
level, alternating between the two in one process and on one context (the guide buffers are cached after the first call, the buffers allocated: what is timed
is the variance kernel, the L launches of ssx_atrous_kernel, the synchronisation and -- asked for with --read-back -- the copy of the image to the host).
Medians of wall-clock times per call; the figure is to be read next to the render time of the headline workload (21.3 ms).
Prints one JSON line.      python tools/denoise_cost.py [--calls 64] [--levels 5] [--res 512] [--spp 16]
With --spectral B the same for ssx_denoise_spectral with B bins (mean_out NULL unless --read-back), alternating with ssx_denoise at the same L in the same
loop -- the XYZ filter is the baseline the spectral filter is read against -- and next to the wall-clock time of the render of that image (spectral output and
noise estimate on, --spp samples in four launches) and the bytes a level must move: 40 + 4E read and 20 + 4E written per pixel, E = B + B / 4.
With --spectral B --demod: the demodulated mode for K = 1, 2, 4 -- the first ssx_albedo_bins call (the kernel; nothing copied to the host), a
cached one, and ssx_denoise_spectral_demod alternating with ssx_denoise_spectral at the same L in one loop, nothing copied to the host, medians of --calls calls."""
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
    ap.add_argument("--spectral", type=int, default=0, metavar="B")
    ap.add_argument("--demod", action="store_true")
    a = ap.parse_args()
    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, spp_per_launch=max(1, a.spp // 4), texture="crystal-lizard-512.png"))
    r.set_noise_estimate(True)
    if a.spectral:
        r.set_spectral_bins(a.spectral)
    r.render_start(); r.render_wait()
    import numpy as np
    if a.spectral and a.demod:
        return demod(a, r, np)
    if a.spectral:
        return spectral(a, r, np)
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


def spectral(a, r, np):
    B, pixels = a.spectral, a.res * a.res
    E = B + B // 4
    mean = np.zeros((a.res, a.res, B), dtype=np.float32)
    image = np.zeros((a.res, a.res, 4), dtype=np.float32)

    def call(which, levels):
        p = r._denoise_params(levels, 1.0, 0.1)
        t = time.perf_counter()
        if which == "spectral":
            r._check(r._lib.ssx_denoise_spectral(r._ctx, ctypes.byref(p), mean.ctypes.data if a.read_back else None, image.ctypes.data if a.read_back else None, None))
        else:
            r._check(r._lib.ssx_denoise(r._ctx, ctypes.byref(p), image.ctypes.data if a.read_back else None, None))
        return (time.perf_counter() - t) * 1e3

    def render():
        t = time.perf_counter()
        r._check(r._lib.ssx_render_start(r._ctx, ctypes.byref(r.params())))
        r._check(r._lib.ssx_render_wait(r._ctx, None))
        return (time.perf_counter() - t) * 1e3

    kinds = (("spectral", a.levels), ("spectral", 1), ("xyz", a.levels))
    for k in kinds + kinds:  # warm-up: guides, buffers
        call(*k)
    ms = {k: [] for k in kinds}
    for _ in range(a.calls):
        for k in kinds:
            ms[k].append(call(*k))
    renders = [render() for _ in range(5)][1:]
    summary = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
    per_level = (statistics.median(ms[kinds[0]]) - statistics.median(ms[kinds[1]])) / max(1, a.levels - 1)
    must = pixels * ((40 + 4 * E) + (20 + 4 * E))
    print(json.dumps({"image": "cornell-srgb %d^2" % a.res, "bins": B, "channels": E, "levels": a.levels, "read_back": bool(a.read_back),
                      "denoise_spectral": summary(ms[kinds[0]]), "denoise_spectral_one_level": summary(ms[kinds[1]]), "denoise_xyz": summary(ms[kinds[2]]),
                      "ms_per_further_level": round(per_level, 4), "render_ms_spp_%d" % a.spp: summary(renders),
                      "bytes_per_level_must_move": must, "bytes_per_level_gathered": pixels * (25 * 40 + 9 * 20 + 25 * 16 * ((E + 3) // 4) + 16 * ((E + 3) // 4)),
                      "must_move_GBps_at_per_level_time": round(must / max(per_level, 1e-9) / 1e6, 1)}))


def demod(a, r, np):
    from simple_spectral_amd import _capi
    B = a.spectral
    summary = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}
    p = r._denoise_params(a.levels, 1.0, 0.1)
    out = {"image": "cornell-srgb %d^2" % a.res, "bins": B, "levels": a.levels, "read_back": False}

    def bins(K):
        t = time.perf_counter()
        r._check(r._lib.ssx_albedo_bins(r._ctx, a.res, a.res, B, K, None))
        return (time.perf_counter() - t) * 1e3

    def call(which, dm, w):
        t = time.perf_counter()
        if which == "demod":
            r._check(r._lib.ssx_denoise_spectral_demod(r._ctx, ctypes.byref(p), ctypes.byref(dm), w.ctypes.data, None, None, None))
        else:
            r._check(r._lib.ssx_denoise_spectral(r._ctx, ctypes.byref(p), None, None, None))
        return (time.perf_counter() - t) * 1e3

    for K in (1, 2, 4):
        first, cached = bins(K), [bins(K) for _ in range(8)]
        dm, w = r._demod_args(dict(supersample=K), B)
        for which in ("demod", "plain") * 2:  # warm-up: guides, buffers
            call(which, dm, w)
        ms = {"demod": [], "plain": []}
        for _ in range(a.calls):
            for which in ("demod", "plain"):
                ms[which].append(call(which, dm, w))
        out["K=%d" % K] = {"albedo_bins_first_call_ms": round(first, 3), "albedo_bins_cached_call": summary(cached),
                           "denoise_spectral_demod": summary(ms["demod"]), "denoise_spectral": summary(ms["plain"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
