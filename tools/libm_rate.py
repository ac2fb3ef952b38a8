"""Rate of the two libm modes (ssx_render_params.libm) on one GPU, with a bit-exactness check of each image against its own oracle on a
few 8x8 tiles: cornell-srgb 512x512 spp=256 (lizard texture) and plane-srgb 1024x1024 spp=64.  Prints one JSON line.

    python tools/libm_rate.py [--repeats N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import glibc_oracle as go  # noqa: E402
import oracle_lib as ol  # noqa: E402
from simple_spectral_amd import Options, Renderer  # noqa: E402

WORKLOADS = (("cornell-srgb", 512, 512, 256, "crystal-lizard-512.png"), ("plane-srgb", 1024, 1024, 64, "crystal-lizard-512.png"))
TILES = ((0, 0), (248, 248), (504, 496))


def run(scene, W, H, spp, tex, libm, repeats):
    r = Renderer(Options(scene_name=scene, res=(W, H), spp=spp, texture=tex, libm=libm))
    r.render_start(); r.render_wait()                        # warm-up (and the image checked below)
    img = r.xyza.copy()
    times = []
    for _ in range(repeats):
        t = time.perf_counter(); r.render_start(); r.render_wait(); times.append(time.perf_counter() - t)
    o = go.Oracle(scene, texture=tex) if libm != "build" else ol.Oracle(scene, texture=tex)
    diff = 0
    for i0, j0 in TILES:
        i0, j0 = min(i0, W - 8), min(j0, H - 8)
        ref = o.render(W, H, spp, rect=(i0, j0, i0 + 8, j0 + 8))
        diff += int((img[j0:j0 + 8, i0:i0 + 8].view(np.uint32) != ref[j0:j0 + 8, i0:i0 + 8].view(np.uint32)).sum())
    best = min(times)
    return {"msamples_per_s": round(W * H * spp / best / 1e6, 1), "best_s": round(best, 4), "median_s": round(float(np.median(times)), 4),
            "kernel": r.plan_info()["kernel"], "kernel_info": r.kernel_info(), "tile_floats_differing_from_oracle": diff}, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    out = {"tool": "libm_rate", "gpus": 1}
    for scene, W, H, spp, tex in WORKLOADS:
        key = "%s_%dx%d_spp%d" % (scene, W, H, spp)
        b, ib = run(scene, W, H, spp, tex, "build", a.repeats)
        g, ig = run(scene, W, H, spp, tex, "glibc-2.35", a.repeats)
        differ = (ib.view(np.uint32) != ig.view(np.uint32)).any(axis=-1)
        out[key] = {"build": b, "glibc-2.35": g, "glibc_over_build_rate": round(g["msamples_per_s"] / b["msamples_per_s"], 4),
                    "pixels_differing_between_modes": round(float(differ.mean()), 5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
