"""Write tests/golden/spectral_sample_flux.npz: the per-sample hero fluxes and first hero wavelengths of one small render, as ssx_debug_sample_flux hands them
out (needs the GPU; tests/test_spectral_gpu.py holds those fluxes to the CPU oracle's samples).  tests/test_spectral_accumulate_cpu.py bins them in two orders
to measure whether a render's data shows the order of addition.

    python tests/golden/make_spectral_flux_fixture.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from simple_spectral_amd import Options, Renderer  # noqa: E402

SCENE, TEX, W, H, SPP, SEED = "cornell-srgb", "test-img.png", 20, 12, 32, 5

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "spectral_sample_flux.npz")
    r = Renderer(Options(scene_name=SCENE, res=(W, H), seed=SEED, texture=TEX))
    r.set_spectral_bins(4)
    flux, lam = r.debug_sample_flux(spp=SPP)
    d = r.scene.desc.contents
    np.savez_compressed(out, flux=flux, lambda_0=lam, lambda_min=np.float32(d.lambda_min), lambda_step=np.float32(d.lambda_step),
                        scene=SCENE, texture=TEX, seed=SEED)
    print("%s: flux %r, lambda_0 %r, %d bytes" % (out, flux.shape, lam.shape, os.path.getsize(out)))
