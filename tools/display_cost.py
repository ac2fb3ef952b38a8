#!/usr/bin/env python3
"""Cost of finishing a development for a display (include/ssx.h "Finishing a development for a display") on cornell-srgb 512^2, crystal-lizard-512: wall-clock of
the pure entries on the developed image -- METER on the render and on a constant image (every lane of every wave on one key: the contention case), LOCAL at r = 4
and r = 32, TONE, and a whole Renderer.finish (meter, derive, local at r = 4, table, tone) -- host to host, so every figure includes the copies of a 3 MB image up
and of the result down.  Beside them, as yardsticks and not as thresholds: ssx_spectral_develop_lens with both stages NULL (unpack and
ssx_develop_images_kernel_g1, nothing read back), one render step of the same sample count, and a device-to-device copy of as many bytes as TONE moves (three
floats in, three out per pixel).  The calls alternate; medians.  One JSON line.

The kernels one by one: run under the profiler's kernel trace, in a run of its own,
    rocprofv3 --kernel-trace --output-format csv -d DIR/display -- python tools/display_cost.py --only meter,meter_constant,local_r4,local_r32,tone
then
    python tools/display_cost.py --summarise DIR
prints per trace and kernel the median, min and max duration.
    python tools/display_cost.py [--runs 16] [--bins 16] [--res 512] [--spp 16] [--only NAME,...] | --summarise DIR"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd.renderer import develop_weights, display_luma, display_matrix, meter_derive, tone_curve  # noqa: E402


def summarise(folder):
    """One JSON line per kernel-trace file under `folder` (*kernel_trace.csv): {kernel: {n, median_us, min_us, max_us}} of the display's kernels, the develop and
    the copy, the first dispatch of each (code object load, cold caches) left out."""
    import csv
    import glob
    for path in sorted(glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)):
        per = {}
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].split("(")[0]
            if any(k in name.lower() for k in ("meter", "local", "tone", "optics", "develop", "copy", "elementwise")):
                per.setdefault(name[:96], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        out = {"trace": os.path.relpath(path, folder).split(os.sep)[0]}
        for name, v in sorted(per.items()):
            v = v[1:] if len(v) > 1 else v
            out[name] = {"n": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=16)
    ap.add_argument("--bins", type=int, default=16)
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

    r = Renderer(Options(scene_name="cornell-srgb", res=(a.res, a.res), spp=a.spp, seed=5, texture="crystal-lizard-512.png"))
    r.set_spectral_bins(a.bins)
    r.render_start()
    r.render_wait()
    c = r.scene.desc.contents
    w = develop_weights(a.bins, c.lambda_min, c.lambda_step)
    image = r.develop(w)
    matrix = display_matrix()
    luma = display_luma(matrix)
    m = meter_derive(*r.meter_images(image, luma))
    constant = np.full_like(image, float(np.median(image[..., 1])))
    curve = tone_curve("reinhard", 2.0 ** -12, 16.0, 19, white=max(float(m["white_exposed"]), 1.0))
    gains = np.float32(m["exposure"]) * np.ones(3, dtype=np.float32)
    local = dict(exposure=m["exposure"], pivot=m["pivot"])
    calls = {"meter": lambda: r.meter_images(image, luma),
             "meter_constant": lambda: r.meter_images(constant, luma),
             "local_r4": lambda: r.local_images(image, luma, 4, 0.5, **local),
             "local_r32": lambda: r.local_images(image, luma, 32, 0.5, **local),
             "tone": lambda: r.tone_images(image, curve, gains=gains, matrix=matrix),
             "finish": lambda: r.finish(image, dict(curve="reinhard", local=dict(radius=4, compress=0.5))),
             "render_step": lambda: (r.render_continue(a.spp), r.render_wait()),
             "lens_both_null": lambda: r._check(r._lib.ssx_spectral_develop_lens(r._ctx, None, None, None, w.ctypes.data, 3, None, None))}
    if not a.only or "copy" in a.only.split(","):
        import torch
        src = torch.zeros(a.res * a.res * 3, dtype=torch.float32, device="cuda")
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
    out = {"workload": "cornell-srgb %d^2, %d bins, %d spp" % (a.res, a.bins, a.spp), "image_bytes": a.res * a.res * 12, "tone_bytes": a.res * a.res * 24,
           "exposure": float(m["exposure"]), "white_exposed": float(m["white_exposed"]), "keys_in_use": int((r.meter_images(image, luma)[0][3] != 0).sum())}
    out.update({k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)} for k, v in ms.items()})
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
