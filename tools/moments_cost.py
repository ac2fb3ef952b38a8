#!/usr/bin/env python3
"""Cost of the spectral moments on the headline workload (cornell-srgb 512^2, 256 spp, crystal-lizard-512) through ssx_render_start + ssx_render_wait: renders with
spectral output on and the moments off and on, alternating between two contexts of one process, wall-clock per render; the moment kernel's own time -- a
one-launch render with and without it, so that the difference is one launch of the kernel over all samples --; and one ssx_spectral_probe call (four rectangles).
Prints one JSON line.      python tools/moments_cost.py [--renders 32] [--bins 16] [--res 512] [--spp 256]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd.renderer import labels_from_rects  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--renders", type=int, default=32)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=256)
    a = ap.parse_args()
    ctx = {}
    for on in (False, True):  # a context each: switching one context back and forth would put the allocation of Q into every render
        ctx[on] = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, texture="crystal-lizard-512.png"))
        ctx[on].set_spectral_bins(a.bins)
        ctx[on].set_spectral_moments(on)

    def render(on, **over):
        r = ctx[on]
        t = time.perf_counter()
        r._check(r._lib.ssx_render_start(r._ctx, ctypes.byref(r.params(**over))))
        r._check(r._lib.ssx_render_wait(r._ctx, None))
        return (time.perf_counter() - t) * 1e3

    for on in (False, True, False, True):  # warm-up
        render(on)
    ms = {False: [], True: []}
    for _ in range(a.renders):
        for on in (False, True):
            ms[on].append(render(on))
    one = {False: [], True: []}  # the whole render in ONE launch: the bin kernel, and with the moments the moment kernel, run once over every sample
    for on in (False, True):
        render(on, spp_per_launch=a.spp)
    for _ in range(max(4, a.renders // 2)):
        for on in (False, True):
            one[on].append(render(on, spp_per_launch=a.spp))
    r = ctx[True]
    q = a.res // 4
    labels = labels_from_rects((a.res, a.res), [(0, 0, q, q), (q, q, 3 * q, 3 * q), (0, 2 * q, a.res, a.res), (a.res - 1, 0, a.res, 1)])
    r.probe_raw(labels)
    probe = []
    for _ in range(8):
        t = time.perf_counter()
        r.probe_raw(labels)
        probe.append((time.perf_counter() - t) * 1e3)
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}
    samples = a.res * a.res * a.spp
    out = {"workload": "cornell-srgb %d^2 spp %d" % (a.res, a.spp), "bins": a.bins, "moments_off": summary(ms[False]), "moments_on": summary(ms[True]),
           "msamples_per_s_off": round(samples / statistics.median(ms[False]) / 1e3, 1), "msamples_per_s_on": round(samples / statistics.median(ms[True]) / 1e3, 1),
           "one_launch_off": summary(one[False]), "one_launch_on": summary(one[True]),
           "moment_kernel_ms": round(statistics.median(one[True]) - statistics.median(one[False]), 3),
           "moment_kernel_reread_bytes": samples * 32, "probe_call": summary(probe), "probe_regions": 4,
           "q_bytes": ctx[True].scratch_info()["sample_bytes"] - ctx[False].scratch_info()["sample_bytes"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
