#!/usr/bin/env python3
"""Cost of depth of field after the render (include/ssx.h "Depth of field after the render") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of one
ssx_spectral_develop_lens call from the context's raw state with an aperture and no lens, everything left on the device, at R = 3, 8 and 12 (the gain so large
that every circle of confusion reaches R off the focus: the worst case of the walk); beside it the separable blur of ssx_spectral_develop_optics at the same R,
one raw ssx_spectral_develop of the same context and one render step of the same sample count.  The calls alternate; medians.  One JSON line per bin count.

The two kernels one by one (ssx_defocus_prepare_kernel, ssx_defocus_gather_kernel), next to the blur kernels and the develop-images kernel: run ONE
configuration under the profiler's kernel trace, in a run of its own,
    rocprofv3 --kernel-trace --output-format csv -d DIR/b64_R12 -- python tools/defocus_cost.py --bins 64 --only defocus_R12,blur_R12
then
    python tools/defocus_cost.py --summarise DIR
prints per trace and kernel the median, min and max duration.
    python tools/defocus_cost.py [--runs 16] [--bins 16,64] [--res 512] [--spp 16] [--only NAME,...] | --summarise DIR"""
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
from simple_spectral_amd.renderer import _defocus_arg, _optics_arg, develop_weights, lens_optics  # noqa: E402


def summarise(folder):
    """One JSON line per kernel-trace file under `folder` (*kernel_trace.csv): {kernel: {n, median_us, min_us, max_us}} of the kernels of the aperture, the lens
    and the develop, the first dispatch of each (code object load, cold caches) left out."""
    import csv
    import glob
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].split("(")[0]
            if "defocus" in name or "optics" in name or "develop" in name:
                per.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out = {"trace": os.path.relpath(path, folder)}
        for name, v in sorted(per.items()):
            v = v[1:] if len(v) > 1 else v
            out[name] = {"n": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=16)
    ap.add_argument("--bins", default="16,64")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--only", default="", help="comma-separated call names: run only these (a kernel trace of one configuration)")
    ap.add_argument("--summarise", default="", help="a directory of kernel-trace CSV files: per kernel the number of dispatches and the median, min and max duration")
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

        def defocus_call(R):
            df, arrays = _defocus_arg({"max_radius": R, "gain": 1000.0, "focus": np.linspace(0.35, 0.15, bins).astype(np.float32)})
            keep.append((df, arrays))
            return lambda: r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None, C.byref(df), None, w.ctypes.data, 3, None, None))

        def blur_call(R):
            op, arrays = _optics_arg(lens_optics(bins, c.lambda_min, c.lambda_step, sigma=R / 3.0, max_radius=R), a.res, a.res)
            keep.append((op, arrays))
            return lambda: r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), w.ctypes.data, 3, None, None))

        calls = {"develop_raw": lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, 3, None)),
                 "render_step": lambda: (r.render_continue(a.spp), r.render_wait()),
                 "lens_both_null": lambda: r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None, None, None, w.ctypes.data, 3, None, None))}
        for R in (3, 8, 12):
            calls["defocus_R%d" % R] = defocus_call(R)
            calls["blur_R%d" % R] = blur_call(R)
        if a.only:
            calls = {k: calls[k] for k in a.only.split(",")}
        for fn in calls.values():                          # warm-up: code objects, the temporaries, the guides
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
