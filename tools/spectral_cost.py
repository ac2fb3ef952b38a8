#!/usr/bin/env python3
"""Cost of the spectral output on the headline workload (cornell-srgb 512^2, 256 spp, crystal-lizard-512) through ssx_render_start + ssx_render_wait:
renders with spectral output off and on (B bins), alternating between two contexts of one process, wall-clock per render; then the stage timers of ssx_get_timing for both.
Prints one JSON line.      python tools/spectral_cost.py [--renders 32] [--bins 16] [--res 512] [--spp 256]"""
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
    ap.add_argument("--renders", type=int, default=32)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    a = ap.parse_args()
    ctx = {}
    for bins in (0, a.bins):  # a context each: switching one context back and forth would put the allocation of the bins into every render
        ctx[bins] = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, texture="crystal-lizard-512.png"))
        ctx[bins].set_spectral_bins(bins)

    def render(bins):
        r = ctx[bins]
        t = time.perf_counter()
        r._check(r._lib.ssx_render_start(r._ctx, ctypes.byref(r.params())))
        r._check(r._lib.ssx_render_wait(r._ctx, None))
        return (time.perf_counter() - t) * 1e3

    for bins in (0, a.bins, 0, a.bins):  # warm-up
        render(bins)
    ms = {0: [], a.bins: []}
    for _ in range(a.renders):
        for bins in (0, a.bins):
            ms[bins].append(render(bins))
    stages = {}
    for bins in (0, a.bins):
        r = ctx[bins]
        render(bins)
        r.set_timing(True)
        wall = [render(bins) for _ in range(4)]
        stages[bins] = {k: round(v / 4, 3) for k, v in r.get_timing().items()}
        stages[bins]["wall"] = round(statistics.median(wall), 3)
        r.set_timing(False)
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}
    samples = a.res * a.res * a.spp
    out = {"workload": "cornell-srgb %d^2 spp %d" % (a.res, a.spp), "bins": a.bins, "off": summary(ms[0]), "on": summary(ms[a.bins]),
           "msamples_per_s_off": round(samples / statistics.median(ms[0]) / 1e3, 1), "msamples_per_s_on": round(samples / statistics.median(ms[a.bins]) / 1e3, 1),
           "stage_ms_per_render_off": stages[0], "stage_ms_per_render_on": stages[a.bins], "kernel_off": ctx[0].plan_info()["kernel"], "kernel_on": ctx[a.bins].plan_info()["kernel"],
           "sample_bytes_off": ctx[0].scratch_info()["sample_bytes"], "sample_bytes_on": ctx[a.bins].scratch_info()["sample_bytes"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
