"""Worker of tests/test_generate_gpu.py: ONE process = ONE place where a plane-topology render makes its samples (SSX_FUSE_GEN under SSX_DEBUG_ENV=1 is
read at every launch; the parent sets both, or neither): the path kernel's refill, or the generate kernel.  The same scene per sample (whole image) and
as an image under an uneven tile layout, against the oracle's results, which the parent computed once and passes by file; and what the library says
about where its launches got their samples (ssx_generate_info).  Prints one JSON line.  Test infrastructure.
usage: python tests/generate_worker.py <oracle results .npz>"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import generate_cases as gc  # noqa: E402
from simple_spectral_amd import Options, Renderer  # noqa: E402
from simple_spectral_amd import dist as sdist  # noqa: E402


def same(a, b):
    """bit equality of float32 arrays; NaN matches NaN of any payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def main():
    ref = np.load(sys.argv[1])
    (W, H), spp, seed = gc.FUSED_RES, gc.FUSED_SPP, gc.FUSED_SEED
    report = {"env": {k: v for k, v in os.environ.items() if k.startswith("SSX_")}}
    r = Renderer(Options(scene_name="plane-srgb", res=(W, H), spp=spp, seed=seed, texture="test-img.png"))
    info = r.plan_info()
    report.update(pass1=info["pass1"], camera_rays=info["camera_rays"], launches_before=r.generate_info())
    xyza, state, _ = r.debug_samples()
    report.update(samples=same(xyza, ref["xyza"]), states=bool(np.array_equal(state, ref["state"])), launches_samples=r.generate_info())
    r.close()
    lay = gc.FUSED_LAYOUT
    r = Renderer(Options(scene_name="plane-srgb", res=(W, H), spp=spp, seed=seed, texture="test-img.png", **lay))
    r.render_start(); r.render_wait()
    own = sdist.tile_owner_mask(W, H, lay["tile_first"], lay["tile_stride"], lay["tile_skew"])
    report.update(owned_pixels=int(own.sum()), image=same(r.xyza[own], ref["image"][own]), launches_image=r.generate_info())
    r.close()
    print(json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
