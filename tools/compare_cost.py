#!/usr/bin/env python3
"""Cost of one comparison of two spectral renders (include/ssx.h "Comparing two spectral renders") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of one
ssx_spectral_compare call (the other render's S, Q and N up, the context's own exported on the device, the labels up, two kernels, six [R][B] arrays back) with the
whole image as one region -- without the maps, and with the two float maps read back too; against ssx_spectral_probe of the whole image on the same context (which
exports one S, Q, N set where the comparison handles two), and against a render step of `--step` samples per pixel (ssx_render_continue + ssx_render_wait, the
moments on).  The other render is the same scene under another seed, rendered once before the timing.  The calls alternate.  Also the bytes of the two S, Q, N
sets.  Prints one JSON line.      python tools/compare_cost.py [--runs 32] [--bins 64] [--res 512] [--step 16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--step", type=int, default=16)
    a = ap.parse_args()

    def context(seed):
        r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.step, seed=seed, texture="crystal-lizard-512.png"))
        r.set_spectral_bins(a.bins)
        r.set_spectral_moments(True)
        r.render_start()
        r.render_wait()
        return r

    b = context(6)
    info, _, NB, SB = b.spectral_read(sums=True)
    QB = b.spectral_variance(q=True)[2]
    b.close()
    other = (info, SB, NB, QB)
    r = context(5)
    labels = np.zeros((a.res, a.res), dtype=np.uint8)      # the whole image: one region

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def step():
        r.render_continue(a.step)
        r.render_wait()

    calls = {
        "probe_whole_image": lambda: r.probe_raw(labels, 1),
        "compare": lambda: r.compare_spectral_raw(other, labels, 1, maps=False),
        "render_step": step,
        "compare_with_maps": lambda: r.compare_spectral_raw(other, labels, 1, maps=True),
        "settle": step,                                    # (the call after the maps' large copies back pays for them on the host: kept off the probe)
    }
    for fn in calls.values():                              # warm-up: code objects, the temporaries
        fn()
    ms = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}
    pixels, B = a.res * a.res, a.bins
    out = {"workload": "cornell-srgb %d^2, %d bins, steps of %d spp" % (a.res, a.bins, a.step), "done_spp": r.done_spp()}
    out.update({k: summary(v) for k, v in ms.items()})
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["compare_over_probe"] = round(med["compare"] / med["probe_whole_image"], 4)
    out["compare_over_step"] = round(med["compare"] / med["render_step"], 4)
    out["maps_extra_ms"] = round(med["compare_with_maps"] - med["compare"], 3)
    out["array_bytes_read"] = 2 * pixels * (2 * B * 8 + (B // 4) * 4)      # S, Q [pixels][B] binary64 and N [pixels][M] uint32 of both renders, each once
    out["other_bytes_uploaded"] = pixels * (2 * B * 8 + (B // 4) * 4)      # ... of which the other render's come from the host with every call
    out["map_bytes"] = 2 * pixels * B * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
