"""Record the outputs of the reference's own self-contained sources (oracle/_ref, built by `make -C oracle ref` where the reference
is at hand) for the inputs tests/test_ref_pins.py uses, into tests/golden/ref_vectors.npz and ref_digests.json, so that those pins -- and
the Meng et al. grid the GPU tests render with -- need nothing outside the repository.

    python tests/golden/make_ref_vectors.py      (needs oracle/_ref/*.so and a built host library)

Stored: the Meng et al. grid as the reference's header defines it and spectrum_xyz_to_p on the pins' inputs; what rgb2spec_load read
from the file the host wrote, with rgb2spec_fetch / rgb2spec_eval_precise on the pins' inputs; lodepng's decodes (and error codes) of
the PNG files the pins generate, and one file written by lodepng's encoder.  Stored as data (ref_vectors.npz): the grid and that file,
which the tests use as inputs.  Everything else is compared bit for bit and stored as SHA-256 digests (ref_digests.json): outputs in
blocks of test_ref_pins.BLOCK rows, and the inputs the pins generate from fixed seeds."""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_lib  # noqa: E402
import test_ref_pins as pins  # noqa: E402

OUT = os.path.join(HERE, "ref_vectors.npz")
OUT_DIGESTS = os.path.join(HERE, "ref_digests.json")


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def meng(g, d):
    lib = ref_lib.meng()
    t = ref_lib.meng_table_from_library()
    for k in ("grid_w", "grid_h", "n_points", "n_samples"):  # (the grid itself: the GPU and CLI tests render with it)
        g["meng_" + k] = np.int32(t[k])
    for k in ("sample_min", "sample_max", "equal_energy_reflectance"):
        g["meng_" + k] = np.float32(t[k])
    g["meng_xy_to_uv"], g["meng_cells"], g["meng_points"] = t["xy_to_uv"], t["cells"], t["points"]
    fp = C.POINTER(C.c_float)
    xyz, lam = pins.meng_xyz_to_p_inputs()
    d["meng_xyz_to_p_inputs_sha256"] = pins.array_sha(xyz) + pins.array_sha(lam)
    d["meng_xyz_to_p_sha256"] = pins.block_shas(np.array([lib.ref_meng_xyz_to_p(C.c_float(l), v.ctypes.data_as(fp)) for v, l in zip(xyz, lam)], np.float32))
    _, _, xyz, lam = pins.meng_specrefl_inputs()
    d["meng_specrefl_inputs_sha256"] = pins.array_sha(xyz) + pins.array_sha(lam)
    d["meng_specrefl_sha256"] = pins.block_shas(np.array([[lib.ref_meng_xyz_to_p(C.c_float(l), v.ctypes.data_as(fp)) for l in ls] for v, ls in zip(xyz, lam)], np.float32))


def jh(d, tmp):
    lib = ref_lib.rgb2spec()
    path = os.path.join(tmp, "model.coeff")
    pins.jh_scene(path)
    model = lib.rgb2spec_load(path.encode())
    assert bool(model)
    m = model.contents
    d["jh_file_sha256"] = sha(path)
    d["jh_res"] = int(m.res)
    d["jh_scale_sha256"] = pins.array_sha(np.ctypeslib.as_array(m.scale, shape=(m.res,)))
    d["jh_data_sha256"] = pins.array_sha(np.ctypeslib.as_array(m.data, shape=(3 * m.res ** 3 * 3,)))
    fp = C.POINTER(C.c_float)
    rgbs, lams = pins.jh_inputs()
    coeffs, evals = [], []
    for k, rgb in enumerate(rgbs):
        c = np.zeros(3, np.float32)
        lib.rgb2spec_fetch(model, rgb.ctypes.data_as(fp), c.ctypes.data_as(fp))
        coeffs.append(c)
        if not np.isnan(c).any():
            evals += [lib.rgb2spec_eval_precise(c.ctypes.data_as(fp), C.c_float(l)) for l in pins.jh_eval_lams(k, lams)]
    lib.rgb2spec_free(model)
    d["jh_inputs_sha256"] = pins.array_sha(np.array(rgbs)) + pins.array_sha(lams)
    d["jh_fetch_sha256"] = pins.block_shas(pins.canonical_nan(coeffs))
    d["jh_eval_sha256"] = pins.block_shas(np.array(evals, np.float32))


def png(g, d, tmp):
    for name in ("test-img.png", "crystal-lizard-512.png"):
        p = os.path.join(pins.DATA, "scenes", name)
        err, img = ref_lib.lodepng_decode(p)
        assert err == 0
        d["png_shipped_%s_sha256" % name] = sha(p)
        d["png_shipped_%s_decoded_sha256" % name] = pins.array_sha(img)
    for ctype, depth in pins.VARIANTS:
        for interlace in (0, 1):
            for key, p in pins.png_variant_files(tmp, ctype, depth, interlace):
                err, img = ref_lib.lodepng_decode(p)
                assert err == 0, key
                d[key + "_sha256"], d[key + "_decoded_sha256"] = sha(p), pins.array_sha(img)
    for name, p in pins.png_bad_files(tmp):
        err, _ = ref_lib.lodepng_decode(p)
        d["png_bad_%s_sha256" % name], d["png_bad_%s_error" % name] = sha(p), int(err)
    fb, expect = pins.png_writer_inputs()
    ours = os.path.join(tmp, "ours.png")
    assert pins._capi.host_lib().ssh_save_image(ours.encode(), fb.ctypes.data, fb.shape[1], fb.shape[0]) == 0
    err, dec = ref_lib.lodepng_decode(ours, rgba=True)
    assert err == 0
    d["png_writer_ours_sha256"], d["png_writer_ours_decoded_sha256"] = sha(ours), pins.array_sha(dec)
    theirs = os.path.join(tmp, "theirs.png")
    assert ref_lib.lodepng().ref_png_encode_rgba8(theirs.encode(), expect.ctypes.data, expect.shape[1], expect.shape[0]) == 0
    g["png_writer_theirs_file"] = np.frombuffer(open(theirs, "rb").read(), np.uint8)


def main():
    if ref_lib.meng() is None or ref_lib.rgb2spec() is None or ref_lib.lodepng() is None:
        raise SystemExit("oracle/_ref/*.so not built: make -C oracle ref (needs the reference's sources)")
    g, d = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        meng(g, d)
        jh(d, tmp)
        png(g, d, tmp)
    np.savez_compressed(OUT, **g)
    with open(OUT_DIGESTS, "w") as f:
        json.dump(d, f, indent=0, sort_keys=True)
        f.write("\n")
    for path in (OUT, OUT_DIGESTS):
        print("%s: %d bytes" % (os.path.relpath(path, ROOT), os.path.getsize(path)))


if __name__ == "__main__":
    main()
