"""Child process of tests/test_plain_switches_gpu.py: the built-in renders of that test, as the environment it is started in has them run
(SSX_DEBUG_ENV=1 SSX_PLAIN_KERNEL=0: the general kernels), written to an .npz.  TEST INFRASTRUCTURE.
    python tests/plain_switches_worker.py OUT.npz"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simple_spectral_amd import Options, Renderer  # noqa: E402

BUILTIN = (("cornell-srgb", 24, 16, 8, 5), ("plane-srgb", 16, 16, 8, 6))   # scene, width, height, spp, seed


def builtin_render(scene, W, H, spp, seed):
    """-> image, the choice plan_info reports for that render, and ssx_debug_samples' three arrays"""
    r = Renderer(Options(scene_name=scene, res=(W, H), spp=spp, seed=seed, texture="test-img.png"))
    r.render_start(); r.render_wait()
    image, switches = r.xyza.copy(), r.plan_info()["switches"]
    xyza, state, levels = r.debug_samples()
    return r, image, switches, xyza, state, levels


if __name__ == "__main__":
    out = {}
    for scene, W, H, spp, seed in BUILTIN:
        _, image, switches, xyza, state, levels = builtin_render(scene, W, H, spp, seed)
        out.update({scene + "/image": image, scene + "/switches": np.array(switches), scene + "/xyza": xyza, scene + "/state": state, scene + "/levels": levels})
    np.savez(sys.argv[1], **out)
