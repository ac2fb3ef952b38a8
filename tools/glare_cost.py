#!/usr/bin/env python3
"""Cost of glare (include/ssx.h "Glare: per-bin convolution by FFT") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of one ssx_spectral_develop_glare
call from the context's raw state, everything left on the device, at R = 12, 64 and 256 (plans 1024^2, 1024^2 and 1024^2: 512 + 2 R rounds up to 1024 for all
three); against ssx_spectral_develop_optics with a blur of R = 12, ssx_spectral_develop_lens with a defocus of R = 12, one raw ssx_spectral_develop of the same
context and one render step of the same sample count.  The host-side part of a glare call (packing the twiddles, uploading the psf: B (2 R + 1)^2 floats, 17
MB at R = 256 and 64 bins) is inside the wall-clock.  The calls alternate; medians.  Prints one JSON line per bin count.

The three kernels one by one (ssx_glare_rows_kernel, ssx_glare_columns_kernel, ssx_glare_rows_back_kernel): run ONE configuration under the profiler's kernel
trace, in a run of its own,
    rocprofv3 --kernel-trace --output-format csv -d DIR/b64_R64 -- python tools/glare_cost.py --bins 64 --only glare_R64
then
    python tools/glare_cost.py --summarise DIR
prints per trace and kernel the dispatches and the median, min and max duration; the rows and columns kernels run twice per chunk (the psf's pass, which
touches 2 R + 1 rows, and the image's), so their durations are listed per pass, told apart by the order of the dispatches.
    python tools/glare_cost.py [--runs 8] [--bins 16,64] [--res 512] [--spp 16] [--only NAME,...] | --summarise DIR"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd.renderer import _defocus_arg, _glare_arg, _optics_arg, develop_weights, glare_aperture, lens_optics, thin_lens_defocus  # noqa: E402


def summarise(folder):
    """One JSON line per kernel-trace file under `folder`, named by the configuration's folder: {kernel: {n, median_us, min_us, max_us}} of the glare's kernels
    and their neighbours.  The rows and columns kernels run twice per chunk, first for the psf, then for the image: the dispatches of each alternate, and are
    keyed by that order.  The first dispatch of each key (code object load, cold caches) is left out."""
    import csv
    import glob
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        per, seen = {}, {}
        rows = sorted(csv.DictReader(open(path)), key=lambda row: int(row["Start_Timestamp"]))
        for row in rows:
            name = row["Kernel_Name"].split("(")[0]
            if not ("glare" in name or "optics" in name or "defocus" in name or "develop" in name):
                continue
            key = name
            if name in ("ssx_glare_rows_kernel", "ssx_glare_columns_kernel"):
                key = "%s, %s pass" % (name, "image" if seen.get(name, 0) % 2 else "psf")
                seen[name] = seen.get(name, 0) + 1
            per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out = {"trace": os.path.relpath(path, folder).split(os.sep)[0]}
        for name, v in sorted(per.items()):
            v = v[1:] if len(v) > 1 else v
            out[name] = {"n": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--bins", default="16,64")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--only", default="")
    ap.add_argument("--summarise", default="")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)

    def timed(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    for bins in (int(x) for x in a.bins.split(",")):
        r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, seed=5, texture="crystal-lizard-512.png"))
        r.set_spectral_bins(bins)
        r.render_start()
        r.render_wait()
        c = r.scene.desc.contents
        w = develop_weights(bins, c.lambda_min, c.lambda_step)
        keep = []

        def glare_call(R):
            gp, arrays = _glare_arg(glare_aperture(bins, c.lambda_min, c.lambda_step, a.res, a.res, blades=6, ring_px=1.5, strength=0.1, radius=R))
            keep.append((gp, arrays))
            return lambda: r._check(r._lib.ssx_spectral_develop_glare(r._ctx, None, None, None, C.byref(gp), w.ctypes.data, 3, None, None))

        op, k1 = _optics_arg(lens_optics(bins, c.lambda_min, c.lambda_step, sigma=4.0, max_radius=12), a.res, a.res)
        df, k2 = _defocus_arg(thin_lens_defocus(r.scene, a.res, bins, aperture=0.1, focus_distance=3.0, max_radius=12))
        keep.append((k1, k2))
        calls = {"develop_raw": lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, 3, None)),
                 "render_step": lambda: (r.render_continue(a.spp), r.render_wait()),
                 "blur_R12": lambda: r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), w.ctypes.data, 3, None, None)),
                 "defocus_R12": lambda: r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None, C.byref(df), None, w.ctypes.data, 3, None, None))}
        for R in (12, 64, 256):
            calls["glare_R%d" % R] = glare_call(R)
        if a.only:
            calls = {k: calls[k] for k in a.only.split(",")}
        for fn in calls.values():
            fn()
        ms = {k: [] for k in calls}
        for _ in range(a.runs):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        out = {"workload": "cornell-srgb %d^2, %d bins, %d spp" % (a.res, bins, a.spp), "q_bytes": a.res * a.res * bins * 4}
        out.update({k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)} for k, v in ms.items()})
        print(json.dumps(out))
        r.close()


if __name__ == "__main__":
    main()
