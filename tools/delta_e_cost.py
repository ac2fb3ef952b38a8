#!/usr/bin/env python3
"""Cost of one colour difference of two developments (include/ssx.h "Colour difference of two developments") on cornell-srgb 512^2, crystal-lizard-512: wall-clock
of one ssx_spectral_delta_e call -- both sides developed raw from the context's state (CIE 1931 against CIE 2006), the rows and reduce kernels, the six [1][2]
arrays back, the maps left on the device -- with the whole image as one region; the same with the two maps (de and lab) read back; against one raw
ssx_spectral_develop of the same context with its output left on the device, and against ssx_spectral_probe of the whole image.  The calls alternate.  Prints one
JSON line.      python tools/delta_e_cost.py [--runs 32] [--bins 64] [--res 512] [--spp 16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd.renderer import develop_weights, develop_white  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()

    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, seed=5, texture="crystal-lizard-512.png"))
    r.set_spectral_bins(a.bins)
    r.set_spectral_moments(True)                           # (the probe needs them)
    r.render_start()
    r.render_wait()
    c = r.scene.desc.contents
    w31, w06 = (develop_weights(a.bins, c.lambda_min, c.lambda_step, observer=o) for o in (1931, 2006))
    white = develop_white(w31, c.lambda_min, c.lambda_step)
    labels = np.zeros((a.res, a.res), dtype=np.uint8)      # the whole image: one region

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    calls = {
        "develop_raw": lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w31.ctypes.data, 3, None)),
        "probe_whole_image": lambda: r.probe_raw(labels, 1),
        "delta_e": lambda: r.delta_e_raw(w31, w06, white, white, None, 1, maps=False),
        "delta_e_labelled": lambda: r.delta_e_raw(w31, w06, white, white, labels, 1, maps=False),
        "delta_e_with_maps": lambda: r.delta_e_raw(w31, w06, white, white, None, 1, maps=True, lab=True),
    }
    for fn in calls.values():                              # warm-up: code objects, the temporaries
        fn()
    ms = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}
    out = {"workload": "cornell-srgb %d^2, %d bins, %d spp" % (a.res, a.bins, a.spp)}
    out.update({k: summary(v) for k, v in ms.items()})
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["delta_e_over_develop"] = round(med["delta_e"] / med["develop_raw"], 3)
    out["delta_e_over_probe"] = round(med["delta_e"] / med["probe_whole_image"], 3)
    out["maps_extra_ms"] = round(med["delta_e_with_maps"] - med["delta_e"], 3)
    out["map_bytes"] = a.res * a.res * 8 * 4
    print(json.dumps(out))


if __name__ == "__main__":
    main()
