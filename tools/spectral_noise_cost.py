#!/usr/bin/env python3
"""Cost of one check of the spectral stopping rule (include/ssx.h "Spectral noise figure") on cornell-srgb 512^2, 64 bins, crystal-lizard-512: wall-clock of one
ssx_spectral_noise call (mask up when there is one, two kernels, the four [B] arrays back) without a mask, with a mask, and with the tile partials read back too;
against a render step of `--step` samples per pixel of the same context (ssx_render_continue + ssx_render_wait, the moments on) and against ssx_spectral_probe of
the whole image as one region (which exports S, Q and N to row-major first).  The figure and the step alternate, as render_until_spectral runs them.  Also the
bytes of S, Q and N one check reads.  Prints one JSON line.      python tools/spectral_noise_cost.py [--checks 32] [--bins 64] [--res 512] [--step 16]"""
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
    ap.add_argument("--checks", type=int, default=32)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--step", type=int, default=16)
    a = ap.parse_args()
    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.step, texture="crystal-lizard-512.png"))
    r.set_spectral_bins(a.bins)
    r.set_spectral_moments(True)
    B, tiles = a.bins, ((a.res + 7) // 8) ** 2
    EV, EM, PP, PU = np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    tEV, tEM, tPP, tPU = np.zeros((tiles, B)), np.zeros((tiles, B)), np.zeros((tiles, B), dtype=np.uint32), np.zeros((tiles, B), dtype=np.uint32)
    mask = np.zeros((a.res, a.res), dtype=np.uint8)
    mask[a.res // 8:a.res // 2, a.res // 4:] = 1
    labels = np.zeros((a.res, a.res), dtype=np.uint8)      # the probe's whole image: one region
    totals = [x.ctypes.data for x in (EV, EM, PP, PU)]
    partials = [x.ctypes.data for x in (tEV, tEM, tPP, tPU)]

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def step():
        r.render_continue(a.step)
        r.render_wait()

    calls = {
        "check": lambda: r._check(r._lib.ssx_spectral_noise(r._ctx, None, *totals, None, None, None, None)),
        "check_masked": lambda: r._check(r._lib.ssx_spectral_noise(r._ctx, mask.ctypes.data, *totals, None, None, None, None)),
        "check_with_partials": lambda: r._check(r._lib.ssx_spectral_noise(r._ctx, None, *totals, *partials)),
        "probe_whole_image": lambda: r.probe_raw(labels, 1),
        "render_step": step,
    }
    r.render_start()
    r.render_wait()
    for fn in calls.values():                              # warm-up: code objects, the stage buffers
        fn()
    ms = {k: [] for k in calls}
    for _ in range(a.checks):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}
    pixels = a.res * a.res
    out = {"workload": "cornell-srgb %d^2, %d bins, steps of %d spp" % (a.res, a.bins, a.step), "done_spp": r.done_spp()}
    out.update({k: summary(v) for k, v in ms.items()})
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["check_over_step"] = round(med["check"] / med["render_step"], 4)
    out["check_over_probe"] = round(med["check"] / med["probe_whole_image"], 4)
    out["state_bytes_read"] = tiles * 64 * (2 * B * 8 + (B // 4) * 4)      # S, Q [tiles][B][64] binary64 and N [tiles][M][64] uint32, each once
    out["pixels"] = pixels
    print(json.dumps(out))


if __name__ == "__main__":
    main()
