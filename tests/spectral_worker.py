"""Worker of tests/test_spectral_gpu.py: ONE process = one kernel plan (the environment switches are read when a scene is uploaded).  Renders a
built-in scene with spectral output on and saves what ssx_spectral_read returns, with the name of the kernel that ran.  Test infrastructure.
    usage: python tests/spectral_worker.py <scene> <W> <H> <spp> <spp_per_launch> <seed> <bins> <out.npz>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
from simple_spectral_amd import Options, Renderer  # noqa: E402


def main():
    scene, out = sys.argv[1], sys.argv[8]
    W, H, spp, chunk, seed, bins = (int(x) for x in sys.argv[2:8])
    r = Renderer(Options(scene_name=scene, res=(W, H), spp=spp, seed=seed, texture="test-img.png", spp_per_launch=chunk))
    r.set_spectral_bins(bins)
    r.render_start(); r.render_wait()
    _, mean, counts, sums = r.spectral_read(sums=True)
    np.savez(out, mean=mean, counts=counts, sums=sums, xyza=r.xyza, kernel=np.array(r.plan_info()["kernel"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
