"""Worker of tests/test_pretrace_gpu.py: ONE process = ONE way of tracing the camera rays (SSX_PRE_HITS under SSX_DEBUG_ENV=1 is read at every
scene upload; the parent sets both), forced on scenes whose calibration would choose the other: crafted and random scenes beyond the built-in
ones, per sample and as an image, against the oracle's results, which the parent computed once and passes by file.  Prints one JSON line.
Test infrastructure.      usage: python tests/pretrace_worker.py <oracle results .npz>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import pretrace_cases as pc  # noqa: E402
from simple_spectral_amd import Options, Renderer  # noqa: E402


def same(a, b):
    """bit equality of float32 arrays; NaN matches NaN of any payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    ref = np.load(sys.argv[1])
    W, H = pc.SAMPLE_RES
    spp = pc.SAMPLE_SPP
    report = {"env": {k: v for k, v in os.environ.items() if k.startswith("SSX_")}, "scenes": {}}
    for name in pc.SAMPLE_CASES:
        c, flags, seed = pc.sample_case(name)
        r = Renderer(Options(scene_name="cornell", res=(W, H), spp=spp, seed=seed, observer=c.observer, indirect_only=flags["indirect_only"],
                             explicit_light_sampling=flags["els"], flat_field_correction=flags["flat_field"]))
        r.upload_scene_desc(c.desc(c.oracle()))
        info = r.plan_info()
        xyza, state, _ = r.debug_samples()
        r.render_start(); r.render_wait()
        report["scenes"][name] = {"camera_rays": info["camera_rays"], "pass1": info["pass1"], "n_prims": len(c.quads),
                                  "states": bool(np.array_equal(state, ref[name + "/state"])), "samples": same(xyza, ref[name + "/xyza"]),
                                  "image": same(r.xyza, ref[name + "/image"])}
        r.close()
    print(json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
