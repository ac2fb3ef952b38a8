"""Depth of field from the command line (include/ssx.h "Depth of field after the render"): --develop-defocus with --develop-output writes the bytes the Python
path writes, on one device and on two (SSX_TEST_ONE_GPU=1: both on the one GPU), where the host gathers the bins and runs the pure entries; alone and in front
of --develop-lens; and the options are refused where --develop-lens is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_spectral_amd import Options, Renderer
from simple_spectral_amd.renderer import develop_weights, lens_optics, thin_lens_defocus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
W, H, SEED, SPP, BINS = 24, 16, 5, 8, 8


def test_cli_develops_with_an_aperture(tmp_path):
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=SEED, texture="test-img.png"))
    r.set_spectral_bins(BINS)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=SPP))))
    r.render_wait()
    d = r.scene.desc.contents
    lmin, lstep = float(d.lambda_min), float(d.lambda_step)
    w = develop_weights(BINS, lmin, lstep)
    ap = thin_lens_defocus(r.scene, H, BINS, 0.5, 3.25, axial=0.2, lambda_ref=520.0, max_radius=5)
    assert ap["gain"] > 0 and len(set(ap["focus"].tolist())) == BINS
    lens = lens_optics(BINS, lmin, lstep, lateral=0.02, sigma=0.7, axial=3.0, lambda_ref=520.0, max_radius=5)

    def save(xyz, name):
        r.framebuffer = r.scene.xyza_to_srgba(np.concatenate([xyz, r.xyza[..., 3:]], axis=2))
        r.save(str(tmp_path / name))
        return open(str(tmp_path / name), "rb").read()

    plain, defocused, both = save(r.develop(w), "plain.pfm"), save(r.develop(w, defocus=ap), "defocus.pfm"), save(r.develop(w, defocus=ap, optics=lens), "both.pfm")
    assert len({plain, defocused, both}) == 3
    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=%d" % SPP, "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + str(tmp_path / "o.pfm"),
              "--spectral-bins=%d" % BINS]
    flags = ["--develop-defocus=0.5,3.25,0.2,520", "--develop-defocus-radius=5"]
    lens_flags = ["--develop-lens=0.02,0.7,3,520", "--develop-lens-radius=5"]
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    for n, (want, extra) in enumerate(((defocused, flags), (defocused, flags + ["--gpus=2"]), (both, flags + lens_flags), (both, flags + lens_flags + ["--gpus=2"]), (plain, []))):
        path = str(tmp_path / ("d%d.pfm" % n))
        p = subprocess.run(common + ["--develop-output=" + path] + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr
        assert open(path, "rb").read() == want, extra
    # refused where --develop-output is refused, and without it; malformed values; a radius without its option; side B without a comparison
    x = "--develop-output=" + str(tmp_path / "x.pfm")
    for extra in (flags, [x, "--rgb"] + flags, [x, "--develop-defocus=1"], [x, "--develop-defocus=-1,2"], [x, "--develop-defocus=1,0"], [x, "--develop-defocus=1,2,3,4,5"],
                  [x, "--develop-defocus=0.5,3", "--develop-defocus-radius=13"], [x, "--develop-defocus-radius=3"], [x, "--delta-e-defocus=0.5,3"]):
        p = subprocess.run(common[:-1] + (["--spectral-bins=%d" % BINS] if "--rgb" not in extra else []) + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode != 0, extra
