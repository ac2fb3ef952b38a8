"""The display's finish from the command line (include/ssx.h "Finishing a development for a display") on a 32 x 32 render: --develop-display with
--develop-display-local writes the bytes the Python chain writes (a PNG: floor(255 v + 0.5) of the finished image, no second transfer function; and a PFM through
the same store), with a white balance and the filmic curve too; --meter-output writes the metering Renderer.meter_images gives; the options are refused where
--develop-output is and where they are malformed; and the command without the new options writes the bytes the plain develop path writes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from simple_spectral_amd import Options, Renderer
from simple_spectral_amd.renderer import develop_weights, display_luma, display_matrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
W, H, SEED, SPP, BINS = 32, 32, 5, 4, 16


def test_cli_finishes_a_development_for_a_display(tmp_path):
    r = Renderer(Options(scene_name="cornell-srgb", res=(W, H), seed=SEED, texture="test-img.png"))
    r.set_spectral_bins(BINS)
    r._check(r._lib.ssx_render_start(r._ctx, C.byref(r.params(spp=SPP))))
    r.render_wait()
    d = r.scene.desc.contents
    w = develop_weights(BINS, float(d.lambda_min), float(d.lambda_step))
    xyz = r.develop(w)

    def save(rgb, name, encoded):
        """the store of --output: `encoded` images go to it as they are, X, Y, Z through the observer's matrix and transfer function"""
        rgba = np.concatenate([rgb, r.xyza[..., 3:]], axis=2).astype(np.float32)
        r.framebuffer = rgba if encoded else r.scene.xyza_to_srgba(rgba)
        r.save(str(tmp_path / name))
        return open(str(tmp_path / name), "rb").read()

    reinhard = r.develop(w, display=dict(curve="reinhard", local=dict(radius=4, compress=0.5)))
    filmic, (hist, special) = r.finish(xyz, dict(curve="filmic", key=0.3, white_percentile=0.95, wb="grey", local=dict(radius=2, compress=0.7, boost=1.5, eps=0.05)), return_meter=True)
    want = {"reinhard.png": save(reinhard, "w0.png", True), "reinhard.pfm": save(reinhard, "w1.pfm", True), "filmic.png": save(filmic, "w2.png", True),
            "plain.png": save(xyz, "w3.png", False)}
    assert len(set(want.values())) == 4
    # the PNG holds floor(255 v + 0.5) of the finished image: no second transfer function on the way
    import zlib
    png = want["reinhard.png"]
    at, idat = 8, b""
    while at < len(png):
        n, kind = int.from_bytes(png[at:at + 4], "big"), png[at + 4:at + 8]
        if kind == b"IDAT":
            idat += png[at + 8:at + 8 + n]
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 4 * W)
    assert (rows[:, 0] == 0).all()
    assert np.array_equal(rows[:, 1:].reshape(H, W, 4)[::-1, :, :3], np.floor((np.float32(255.0) * reinhard).astype(np.float64) + 0.5).astype(np.uint8))   # (the product in binary32, as the store makes it)

    common = [CLI, "-s=cornell-srgb", "-w=%d" % W, "-h=%d" % H, "-spp=%d" % SPP, "--seed=%d" % SEED, "--texture=data/scenes/test-img.png", "-o=" + str(tmp_path / "o.pfm"),
              "--spectral-bins=%d" % BINS]
    env = dict(os.environ, SSX_TEST_ONE_GPU="1")
    csv = str(tmp_path / "hist.csv")
    runs = (("reinhard.png", ["--develop-display=reinhard", "--develop-display-local=4,0.5"]), ("reinhard.pfm", ["--develop-display=reinhard,0.18,0.99", "--develop-display-local=4,0.5,1,0.25", "--develop-display-wb=none"]),
            ("filmic.png", ["--develop-display=filmic,0.3,0.95", "--develop-display-local=2,0.7,1.5,0.05", "--develop-display-wb=grey", "--meter-output=" + csv]),
            ("plain.png", []), ("plain.png", ["--meter-output=" + csv]))
    for n, (key, extra) in enumerate(runs):
        path = str(tmp_path / ("d%d.%s" % (n, key.split(".")[1])))
        p = subprocess.run(common + ["--develop-output=" + path] + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode == 0, p.stderr
        assert open(path, "rb").read() == want[key], extra
    # the metering: the lines of the non-zero counters, the luminance the display sees
    h2, s2 = r.meter_images(xyz, display_luma(display_matrix()))
    assert np.array_equal(h2, hist) and np.array_equal(s2, special)
    lines = open(csv).read().split("\n")
    assert lines[0] == "quantity,key,lower_edge,count" and lines[-1] == ""
    got_h, got_s = np.zeros_like(hist), np.zeros_like(special)
    for ln in lines[1:-1]:
        k, key, edge, count = ln.split(",")
        if key.isdigit():
            got_h[int(k), int(key)] = int(count)
            assert np.float32(edge) == np.array([int(key) << 19], dtype=np.uint32).view(np.float32)[0]
        else:
            got_s[int(k), ("zero", "negative", "inf", "nan").index(key)] = int(count)
    assert np.array_equal(got_h, hist) and np.array_equal(got_s, special) and hist[3].sum() > 0
    # refused: without --develop-output; where --develop-output is (--rgb); the companions without --develop-display; malformed values
    x = "--develop-output=" + str(tmp_path / "x.png")
    for extra in (["--develop-display=reinhard"], ["--meter-output=" + csv], [x, "--rgb", "--develop-display=reinhard"], [x, "--develop-display-local=4,0.5"], [x, "--develop-display-wb=grey"],
                  [x, "--develop-display=aces"], [x, "--develop-display=reinhard,0"], [x, "--develop-display=reinhard,0.18,1.5"], [x, "--develop-display=reinhard,0.18,0.9,1"],
                  [x, "--develop-display=clip", "--develop-display-local=0,0.5"], [x, "--develop-display=clip", "--develop-display-local=33,0.5"], [x, "--develop-display=clip", "--develop-display-local=4"],
                  [x, "--develop-display=clip", "--develop-display-local=4,0.5,1,0"], [x, "--develop-display=clip", "--develop-display-local=2.5,0.5"],
                  [x, "--develop-display=clip", "--develop-display-wb=auto"]):
        p = subprocess.run(common[:-1] + (["--spectral-bins=%d" % BINS] if "--rgb" not in extra else []) + extra, cwd=ROOT, capture_output=True, text=True, env=env)
        assert p.returncode != 0, extra
