"""The sensor from the command line (include/ssx.h "Developing onto a sensor"): --develop-sensor and its options with --develop-output write the bytes the Python
path writes, and --sensor-raw-output its mosaic, at 24 x 16, on one device and on two (SSX_TEST_ONE_GPU=1: both on the one GPU), where the host gathers the bins
and runs the pure entries; alone and behind --develop-defocus and --develop-lens; with the stand-in curves and with curves from files; --develop-sensor-curves
on its own equals a develop with develop_weights(responses=); and the options are refused where --develop-lens is."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_spectral_amd import Options, Renderer
from simple_spectral_amd.renderer import (develop_weights, lens_optics, load_spectrum_csv, sensor_bayer, sensor_ccm, sensor_exposure, sensor_standin_curves,
                                          thin_lens_defocus)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
W, H, SEED, SPP, BINS = 24, 16, 5, 8, 8


def test_cli_develops_onto_a_sensor(tmp_path):
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=SEED, texture="test-img.png"))
    r.set_spectral_bins(BINS)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=SPP))))
    r.render_wait()
    d = r.scene.desc.contents
    lmin, lstep = float(d.lambda_min), float(d.lambda_step)
    target = develop_weights(BINS, lmin, lstep)
    # a camera's curves in files of data/*.csv's format: not the stand-ins
    lam = np.arange(400.0, 701.0, 10.0)
    paths = []
    for name, peak, width in (("r", 610.0, 40.0), ("g", 530.0, 45.0), ("b", 450.0, 30.0)):
        paths.append(str(tmp_path / ("%s-400+10+700.csv" % name)))
        open(paths[-1], "w").write("".join("%.9g\n" % v for v in np.exp(-0.5 * ((lam - peak) / width) ** 2).astype(np.float32)))
    file_curves = [load_spectrum_csv(p) for p in paths]
    standins = sensor_standin_curves()
    assert [int(np.argmax(s)) * 5 + 380 for s, _, _ in standins] == [600, 540, 460] and all((lo, hi) == (380.0, 730.0) for _, lo, hi in standins)

    def a_sensor(curves, pattern, method, white_level):
        cam = develop_weights(BINS, lmin, lstep, responses=curves)
        s = dict(sensor_bayer(pattern, method), weights=cam, ccm=sensor_ccm(cam, target), noise=1, seed=7)
        s.update(sensor_exposure(full_well=12000.0, white_level=white_level, bits=12, black=64.0, read_e=2.5))
        return s

    def save(xyz, name):
        r.framebuffer = r.scene.xyza_to_srgba(np.concatenate([xyz, r.xyza[..., 3:]], axis=2))
        r.save(str(tmp_path / name))
        return open(str(tmp_path / name), "rb").read()

    white_level = float(r.develop(target)[..., 1].max())
    ap = thin_lens_defocus(r.scene, H, BINS, 0.5, 3.25, axial=0.2, lambda_ref=520.0, max_radius=5)
    lens = lens_optics(BINS, lmin, lstep, lateral=0.02, sigma=0.7, axial=3.0, lambda_ref=520.0, max_radius=5)
    s_std, s_file = a_sensor(standins, "GRBG", "mhc", white_level), a_sensor(file_curves, "BGGR", "bilinear", white_level)
    img_std, raw_std, _ = r.develop(None, sensor=s_std, return_raw=True)
    img_all, raw_all, _ = r.develop(None, sensor=s_file, defocus=ap, optics=lens, return_raw=True)
    plain_sensor = dict(s_std, noise=0, white=0.0, dn_per_e=1.0, e_per_dn=1.0, black=0.0, read_var=0.0, **{k: v for k, v in sensor_exposure(15000.0, 1.0).items() if "exposure" in k})
    want = {"std": save(img_std, "std.pfm"), "all": save(img_all, "all.pfm"), "plain": save(r.develop(target), "plain.pfm"),
            "default": save(r.develop(None, sensor=plain_sensor), "default.pfm"),
            "curves": save(r.develop(develop_weights(BINS, lmin, lstep, responses=file_curves)), "curves.pfm")}
    assert len(set(want.values())) == 5                                                               # (plain: only to tell the others from it)

    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=%d" % SPP, "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + str(tmp_path / "o.pfm"),
              "--spectral-bins=%d" % BINS]
    scales = ["--develop-sensor-exposure=12000,%.17g" % white_level, "--develop-sensor-noise=2.5,7", "--develop-sensor-bits=12,64"]
    std = ["--develop-sensor=GRBG"] + scales
    everything = ["--develop-sensor=BGGR,bilinear", "--develop-sensor-curves=" + ",".join(paths)] + scales + ["--develop-defocus=0.5,3.25,0.2,520", "--develop-defocus-radius=5",
                                                                                                               "--develop-lens=0.02,0.7,3,520", "--develop-lens-radius=5"]
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    runs = (("std", std, raw_std), ("all", everything, raw_all), ("all", everything + ["--gpus=2"], raw_all),
            ("default", ["--develop-sensor=GRBG,mhc"], None), ("curves", ["--develop-sensor-curves=" + ",".join(paths)], None))
    for n, (key, extra, raw) in enumerate(runs):
        path, raw_path = str(tmp_path / ("d%d.pfm" % n)), str(tmp_path / ("raw%d.npy" % n))
        p = subprocess.run(common + ["--develop-output=" + path] + extra + (["--sensor-raw-output=" + raw_path] if raw is not None else []), cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr
        assert open(path, "rb").read() == want[key], extra
        if raw is not None:
            got = np.load(raw_path)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), raw.view(np.uint32)), extra
    # refused where --develop-lens is refused (without --develop-output, with --rgb); malformed values; the sensor's other options without the sensor
    x = "--develop-output=" + str(tmp_path / "x.pfm")
    for extra in (std, ["--develop-sensor-curves=" + ",".join(paths)], [x, "--rgb"] + std, [x, "--develop-sensor=RGBG"], [x, "--develop-sensor=RGGB,nearest"], [x, "--develop-sensor=RGGB,mhc,3"],
                  [x, "--develop-sensor=RGGB", "--develop-sensor-curves=" + paths[0]], [x, "--develop-sensor=RGGB", "--develop-sensor-curves=" + ",".join(paths[:2] + ["nowhere-400+10+700.csv"])],
                  [x, "--develop-sensor=RGGB", "--develop-sensor-exposure=0,1"], [x, "--develop-sensor=RGGB", "--develop-sensor-exposure=100"], [x, "--develop-sensor=RGGB", "--develop-sensor-noise=-1"],
                  [x, "--develop-sensor=RGGB", "--develop-sensor-bits=0"], [x, "--develop-sensor=RGGB", "--develop-sensor-bits=25"], [x, "--develop-sensor=RGGB", "--develop-sensor-bits=8,255"],
                  [x] + scales, [x, "--sensor-raw-output=" + str(tmp_path / "r.npy")], [x, "--develop-sensor=RGGB", "--delta-e-output=" + str(tmp_path / "de.npy")]):
        p = subprocess.run(common[:-1] + (["--spectral-bins=%d" % BINS] if "--rgb" not in extra else []) + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode != 0, extra
