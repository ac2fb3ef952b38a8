#!/usr/bin/env python3
"""Cost of developing onto a sensor (include/ssx.h "Developing onto a sensor") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of one
ssx_spectral_develop_sensor call from the context's raw state (unpack, SENSOR with noise and a 12-bit ADC, DEMOSAIC), everything left on the device; beside
it ssx_spectral_develop_lens with both stages NULL (unpack, then ssx_develop_images_kernel_g1 on the same q), one raw ssx_spectral_develop of the same context,
one render step of the same sample count, and a device-to-device copy of as many bytes as DEMOSAIC moves (one float in, three out per pixel: a copy of two
floats per pixel).  The calls alternate; medians.  One JSON line per bin count.

The kernels one by one (ssx_sensor_kernel against ssx_develop_images_kernel_g1; ssx_demosaic_kernel against the copy's kernel): run under the profiler's
kernel trace, in a run of its own,
    rocprofv3 --kernel-trace --output-format csv -d DIR/b64 -- python tools/sensor_cost.py --bins 64 --only sensor,lens_both_null,copy
then
    python tools/sensor_cost.py --summarise DIR
prints per trace and kernel the median, min and max duration.
    python tools/sensor_cost.py [--runs 16] [--bins 16,64] [--res 512] [--spp 16] [--only NAME,...] | --summarise DIR"""
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
from simple_spectral_amd.renderer import _sensor_arg, develop_weights, sensor_bayer, sensor_ccm, sensor_exposure  # noqa: E402


def summarise(folder):
    """One JSON line per kernel-trace file under `folder` (*kernel_trace.csv): {kernel: {n, median_us, min_us, max_us}} of the kernels of the sensor, the lens's
    unpack, the develop and the copy, the first dispatch of each (code object load, cold caches) left out."""
    import csv
    import glob
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].split("(")[0]
            if any(k in name.lower() for k in ("sensor", "demosaic", "optics", "develop", "copy", "elementwise")):
                per.setdefault(name[:96], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out = {"trace": os.path.relpath(path, folder).split(os.sep)[0]}   # the run's own directory (b16, b64), not the profiler's host and process names below it
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
        lam = np.arange(380.0, 731.0, 5.0)
        cam = develop_weights(bins, c.lambda_min, c.lambda_step,
                              responses=[(np.exp(-0.5 * ((lam - peak) / 35.0) ** 2).astype(np.float32), 380.0, 730.0) for peak in (600.0, 540.0, 460.0)])
        sensor = dict(sensor_bayer("RGGB", "mhc"), weights=cam, ccm=sensor_ccm(cam, develop_weights(bins, c.lambda_min, c.lambda_step, space="lrgb")), noise=1, seed=1)
        sensor.update(sensor_exposure(full_well=15000.0, white_level=40.0, bits=12, black=64.0, read_e=3.0))
        sp, keep = _sensor_arg(sensor)
        calls = {"develop_raw": lambda: r._check(r._lib.ssx_spectral_develop(r._ctx, None, w.ctypes.data, 3, None)),
                 "render_step": lambda: (r.render_continue(a.spp), r.render_wait()),
                 "lens_both_null": lambda: r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None, None, None, w.ctypes.data, 3, None, None)),
                 "sensor": lambda: r._check(r._lib.ssx_spectral_develop_sensor(r._ctx, None, None, None, C.byref(sp), None, None, None))}
        if not a.only or "copy" in a.only.split(","):
            import torch
            src = torch.zeros(a.res * a.res * 2, dtype=torch.float32, device="cuda")
            dst = torch.empty_like(src)
            calls["copy"] = lambda: (torch.mul(src, 1.0, out=dst), torch.cuda.synchronize())   # an elementwise kernel with float4 accesses (dst.copy_ would be a DMA-style buffer copy)
        if a.only:
            calls = {k: calls[k] for k in a.only.split(",")}
        for fn in calls.values():                          # warm-up: code objects, the temporaries
            fn()
        ms = {k: [] for k in calls}
        for _ in range(a.runs):
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        out = {"workload": "cornell-srgb %d^2, %d bins, %d spp" % (a.res, bins, a.spp), "q_bytes": a.res * a.res * bins * 4, "demosaic_bytes": a.res * a.res * 16}
        out.update({k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)} for k, v in ms.items()})
        print(json.dumps(out))
        r.close()


if __name__ == "__main__":
    main()
