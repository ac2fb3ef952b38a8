#!/usr/bin/env python3
"""Cost of developing through a lens (include/ssx.h "Developing through a lens") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of one
ssx_spectral_develop_optics call from the context's raw state, everything left on the device, at R = 0 (warp only), 3, 8 and 12, with a warp-only and a
blur-only lens beside the full one; against one raw ssx_spectral_develop of the same context (its state kernel reads the same S once) and against one render
step of the same sample count.  The calls alternate; medians.  Prints one JSON line per bin count.

The four kernels one by one (ssx_optics_unpack_kernel, ssx_optics_warp_kernel, ssx_optics_blur_h_kernel, ssx_optics_blur_v_kernel) next to
ssx_develop_images_kernel_g1 at the same bins, which reads the same q once -- the yardstick of bytes moved: run ONE configuration under the profiler's kernel
trace, in a run of its own,
    rocprofv3 --kernel-trace --output-format csv -d DIR/b64_R12 -- python tools/optics_cost.py --bins 64 --only lens_R12
(every lens call ends in the develop-images kernel, so the yardstick is in the same trace), then
    python tools/optics_cost.py --summarise DIR
prints per trace and kernel the median, min and max duration.
    python tools/optics_cost.py [--runs 16] [--bins 16,64] [--res 512] [--spp 16] [--images] [--only NAME,...] | --summarise DIR"""
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
from simple_spectral_amd.renderer import _optics_arg, develop_weights, lens_optics  # noqa: E402


def summarise(folder):
    """One JSON line per kernel-trace file under `folder` (what the profiler's kernel trace writes as *kernel_trace.csv): {kernel: {n, median_us, min_us, max_us}}
    of the kernels of the lens and of the develop, the first dispatch of each (code object load, cold caches) left out."""
    import csv
    import glob
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].split("(")[0]
            if "optics" in name or "develop" in name:
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
    ap.add_argument("--images", action="store_true")
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

        def lens_call(lens):
            op, arrays = _optics_arg(lens, a.res, a.res)
            keep.append((op, arrays))
            return lambda: r._check(r._lib.ssx_spectral_develop_optics(r._ctx, None, C.byref(op), w.ctypes.data, 3, None, None))

        calls = {"develop_raw": lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, 3, None)),
                 "render_step": lambda: (r.render_continue(a.spp), r.render_wait())}
        for R in (0, 3, 8, 12):                            # sigma = R / 3: the widest bins reach R
            calls["lens_R%d" % R] = lens_call(lens_optics(bins, c.lambda_min, c.lambda_step, lateral=0.004, sigma=R / 3.0, axial=R / 3.0, max_radius=R))
        calls["warp_only_large"] = lens_call(lens_optics(bins, c.lambda_min, c.lambda_step, lateral=0.5, max_radius=0))   # |s_b - 1| up to 0.15: the gathers drift apart
        calls["blur_only_R12"] = lens_call(lens_optics(bins, c.lambda_min, c.lambda_step, sigma=4.0, max_radius=12))
        calls["identity"] = lens_call(lens_optics(bins, c.lambda_min, c.lambda_step))                                     # unpack + develop_images alone
        if a.images:
            q = np.zeros((a.res, a.res, bins), dtype=np.float32)
            calls["develop_images_with_copies"] = lambda: r.develop_images(q, w)
        if a.only:
            calls = {k: calls[k] for k in a.only.split(",")}
        for fn in calls.values():                          # warm-up: code objects, the temporaries
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
