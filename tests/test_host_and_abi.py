"""Host-side product code (libssx_host.so) and the shape of the C ABI; no GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.renderer import Scene, SsxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ss[xh]_[a-z0-9_]+)\s*\(", text)))


def test_libraries_export_every_declared_symbol():
    sbuild.build_all(formal=True)  # (the GPU box gets the formal variant from the same build: tests/test_gpu_variants.py)
    hip = C.CDLL(sbuild.HIP_LIB)   # loads without a GPU; no compute call is made
    host = C.CDLL(sbuild.HOST_LIB)
    fx, fh = declared_functions("ssx.h"), declared_functions("ssx_host.h")
    assert set(fx) == set(_capi.HIP_SYMBOLS) and set(fh) == set(_capi.HOST_SYMBOLS)
    for s in fx:
        getattr(hip, s)
    for s in fh:
        getattr(host, s)
    hip.ssx_abi_version.restype = C.c_int
    assert hip.ssx_abi_version() == _capi.SSX_ABI_VERSION == 2


def test_struct_layouts_match_the_headers():
    # sizes the C compiler reports for the ABI structs (guards the ctypes mirrors)
    import subprocess, tempfile
    src = '#include "ssx.h"\n#include <stdio.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n",sizeof(ssx_spectrum),sizeof(ssx_quad),sizeof(ssx_material),sizeof(ssx_texture),sizeof(ssx_scene_desc),sizeof(ssx_render_params),sizeof(ssx_meng_grid));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    mine = [C.sizeof(x) for x in (_capi.SsxSpectrum, _capi.SsxQuad, _capi.SsxMaterial, _capi.SsxTexture, _capi.SsxSceneDesc, _capi.SsxRenderParams, _capi.SsxMengGrid)]
    assert sizes == mine


@pytest.mark.parametrize("scene,observer", [("cornell", 1931), ("cornell-srgb", 1931), ("plane-srgb", 1931), ("cornell-srgb", 2006)])
def test_host_scene_tables_equal_the_oracle(scene, observer):
    """The product's host code and the oracle are written independently; the POD the kernel gets
    must hold the same numbers the oracle computes."""
    s = Scene(scene, observer=observer, texture="test-img.png")
    o = ol.Oracle(scene, observer=observer, texture="test-img.png")
    d = s.desc.contents
    pv = o.lib.orc_scene_pv_inv(o.scene)
    assert [d.pv_inv[i] for i in range(16)] == [pv[i] for i in range(16)]
    cp = o.lib.orc_scene_cam_pos(o.scene)
    assert [d.cam_pos[i] for i in range(3)] == [cp[i] for i in range(3)]
    for key, name in (("spec_xbar", "xbar"), ("spec_ybar", "ybar"), ("spec_zbar", "zbar"), ("spec_basis_r", "basis_r"),
                      ("spec_basis_g", "basis_g"), ("spec_basis_b", "basis_b")):
        sp = d.spectra[getattr(d, key)]
        data, low, high, dr = o.spectrum(name)
        got = np.ctypeslib.as_array(d.samples, shape=(d.n_samples,))[sp.offset:sp.offset + sp.n]
        assert (sp.n, sp.low, sp.high, sp.delta_recip) == (len(data), low, high, dr)
        assert np.array_equal(got.view(np.uint32), data.view(np.uint32))
    m = o.lib.orc_color_matrix(o.color, b"xyz_to_lrgb")
    assert np.array_equal(s.color_values("xyz_to_lrgb"), np.array([m[i] for i in range(9)], dtype=np.float32))
    npr, nl = C.c_int(), C.c_int()
    o.lib.orc_scene_counts(o.scene, C.byref(npr), C.byref(nl), None)
    assert (d.n_quads, d.n_lights) == (npr.value, nl.value)
    # texel decode LUT == srgb_to_lrgb of the oracle
    lut = np.array(d.srgb_to_linear[:], dtype=np.float32)
    for u in (0, 1, 10, 11, 128, 255):
        a = (C.c_float * 3)(*([np.float32(u) * np.float32(1.0 / 255.0)] * 3)); b = (C.c_float * 3)()
        o.lib.orc_srgb_to_lrgb(a, b)
        assert lut[u] == b[0]
    # XYZ -> sRGB store
    xyza = np.random.RandomState(0).uniform(0, 3000, (50, 4)).astype(np.float32)
    assert np.array_equal(s.xyza_to_srgba(xyza).view(np.uint32), o.to_srgba(xyza).view(np.uint32))


def test_host_error_codes_mirror_the_reference():
    with pytest.raises(SsxError) as e:
        Scene("nonsense")
    assert e.value.code == -3 and "Unrecognized scene" in str(e.value)  # src/renderer.cpp:32-38
    with pytest.raises(SsxError) as e:
        Scene("cornell", data_dir="/nonexistent")
    assert e.value.code == -1  # src/spectrum.cpp:179-182
    with pytest.raises(SsxError) as e:
        Scene("cornell-srgb", texture="/nonexistent.png")
    assert e.value.code == -1  # src/material.cpp:15-18


def test_png_decoder_and_writers(tmp_path):
    from PIL import Image
    host = _capi.host_lib()
    for name in ("test-img.png", "crystal-lizard-512.png"):
        p = os.path.join(ROOT, "data", "scenes", name)
        ptr, w, h = C.POINTER(C.c_uint8)(), C.c_uint32(), C.c_uint32()
        assert host.ssh_load_png_rgb8(p.encode(), C.byref(ptr), C.byref(w), C.byref(h)) == 0
        got = np.ctypeslib.as_array(ptr, shape=(h.value, w.value, 3)).copy()
        host.ssh_free(ptr)
        assert np.array_equal(got, np.asarray(Image.open(p).convert("RGB")))
    rs = np.random.RandomState(3)
    W, H = 13, 7
    fb = rs.uniform(-0.1, 1.2, (H, W, 4)).astype(np.float32)
    png = str(tmp_path / "o.png")
    assert host.ssh_save_image(png.encode(), fb.ctypes.data, W, H) == 0
    back = np.asarray(Image.open(png))  # RGBA8, top row first
    want = np.floor(np.clip(np.float32(255.0) * fb, 0, 255) + np.float32(0.5)).astype(np.uint8)[::-1]  # std::round (half away from zero)
    assert back.shape == (H, W, 4) and np.array_equal(back, want)
    pfm = str(tmp_path / "o.pfm")
    assert host.ssh_save_image(pfm.encode(), fb.ctypes.data, W, H) == 0
    raw = open(pfm, "rb").read()
    header = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(header) and len(raw) == len(header) + 12 * W * H
    first = np.frombuffer(raw[len(header):len(header) + 12], dtype="<f4")  # top row first
    lin = (C.c_float * 3)(); src = (C.c_float * 3)(*fb[H - 1, 0, :3])
    ol.load().orc_srgb_to_lrgb(src, lin)
    assert np.array_equal(first, np.array(lin[:], dtype=np.float32))
    csv = str(tmp_path / "o.csv")
    assert host.ssh_save_image(csv.encode(), fb.ctypes.data, W, H) == 0
    rows = open(csv).read().strip().split("\n")
    assert len(rows) == H and len(rows[0].split(",")) == 3 * W
    hdr = str(tmp_path / "o.hdr")
    assert host.ssh_save_image(hdr.encode(), fb.ctypes.data, W, H) == 0
    raw = open(hdr, "rb").read()
    assert raw.startswith(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n") and raw.endswith(raw[-4 * W * H:]) and b"-Y 7 +X 13\n" in raw


def test_float_image_writers_byte_for_byte(tmp_path):
    """VERDICT r02 "smaller": the .csv / .hdr / .pfm writers against an INDEPENDENT encoding of src/framebuffer.cpp:40-135,
    written here from the reference's text (every non-PNG writer first converts the stored sRGB back to linear RGB with
    Color::srgb_to_lrgb -- the oracle's, i.e. the platform powf the reference calls): whole files, byte for byte, on values
    that include negatives, zeros, tiny and > 1 components."""
    import ctypes as C
    import math
    import struct
    host = _capi.host_lib()
    lib = ol.load()
    rs = np.random.RandomState(11)
    W, H = 9, 6
    fb = rs.uniform(-0.05, 1.3, (H, W, 4)).astype(np.float32)
    fb[0, 0, :3] = 0.0; fb[1, 2, :3] = (1e-12, 0.0, 1e-20); fb[2, 3, :3] = (3.5, 0.25, 1e-3); fb[3, 1, :3] = (-0.2, -0.1, -0.3)
    lin = np.zeros((H, W, 3), dtype=np.float32)
    src, dst = (C.c_float * 3)(), (C.c_float * 3)()
    for j in range(H):
        for i in range(W):
            src[:] = [float(x) for x in fb[j, i, :3]]
            lib.orc_srgb_to_lrgb(src, dst)
            lin[j, i] = dst[:]

    def g(x):  # printf("%g") of a double
        return "%g" % float(x)
    # .csv (:40-63): rows in STORAGE order (row 0 = bottom first), "%g,%g,%g" per pixel, comma between pixels, "\n" per row
    want = "".join(",".join("%s,%s,%s" % (g(lin[j, i, 0]), g(lin[j, i, 1]), g(lin[j, i, 2])) for i in range(W)) + "\n" for j in range(H)).encode()
    path = str(tmp_path / "o.csv")
    assert host.ssh_save_image(path.encode(), fb.ctypes.data, W, H) == 0
    assert open(path, "rb").read() == want
    # .pfm (:112-140): "PF\n<w> <h>\n-1.0\n", then rows TOP to bottom (file row j = storage row H-1-j), 3 little-endian floats per pixel
    want = b"PF\n%d %d\n-1.0\n" % (W, H) + b"".join(lin[H - 1 - j, i].astype("<f4").tobytes() for j in range(H) for i in range(W))
    path = str(tmp_path / "o.pfm")
    assert host.ssh_save_image(path.encode(), fb.ctypes.data, W, H) == 0
    assert open(path, "rb").read() == want
    # .hdr (:64-111): flat RGBE, rows top to bottom; v = max(r,g,b); v < 1e-32 -> four zero bytes; else frexp, scale = m*256/v,
    # bytes = clamp(int(round(round(c*scale))), 0, 255), exponent byte = e + 128 (as uint8)
    def f32(x):
        return np.float32(x)
    body = b""
    for j in range(H):
        for i in range(W):
            r_, g_, b_ = (f32(c) for c in lin[H - 1 - j, i])
            v = max(r_, max(g_, b_))
            if v < f32(1.0e-32):
                body += struct.pack("<I", 0)
                continue
            m, e = math.frexp(float(v))
            scale = f32(f32(m) * f32(256.0)) / v          # std::frexp(v,&e) * 256.0f / v in float
            # glm::round(x) = std::round(x) (half away from zero); the second std::round of an integer-valued float is the identity
            def cround(c):
                x = float(f32(c * scale))
                return math.floor(abs(x) + 0.5) * (1.0 if x >= 0 else -1.0)
            body += bytes([int(min(max(int(cround(c)), 0), 255)) for c in (r_, g_, b_)] + [(e + 128) & 0xFF])
    want = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\nSOFTWARE=simple-spectral\n\n-Y %d +X %d\n" % (H, W) + body
    path = str(tmp_path / "o.hdr")
    assert host.ssh_save_image(path.encode(), fb.ctypes.data, W, H) == 0
    got = open(path, "rb").read()
    assert got == want, [k for k in range(min(len(got), len(want))) if got[k] != want[k]][:8]


def test_missing_hip_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_capi, "_hip", None)
    monkeypatch.setattr(sbuild, "HIP_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        _capi.hip_lib()


def test_host_library_links_against_neither_hip_nor_the_device_library():
    """The host resolves the C ABI at run time (host/renderer.cpp: Renderer::Api), and takes its prototypes from include/ssx.h without using the functions:
    libssx_host.so needs no HIP runtime and no libssx_hip.so, and loads on a machine without a GPU."""
    sbuild.build_host()
    _, needed = _capi._elf_dynamic(sbuild.HOST_LIB)
    assert needed, "no dynamic section read from libssx_host.so"
    assert not [n for n in needed if "libamdhip64" in n or "libssx_hip" in n], needed
    host = C.CDLL(sbuild.HOST_LIB)
    for s in _capi.HOST_SYMBOLS:
        getattr(host, s)


def test_jakob_hanika_model_host_vs_oracle_and_round_trip(tmp_path):
    """RENDER_MODE_SPECTRAL_JH (config 3): the table is fitted by the build's own optimiser (the
    authors' .coeff blob is missing from the reference); fetch/eval must equal the oracle's
    restatement of rgb2spec.c bit for bit, and the uplift must round-trip colours."""
    path = str(tmp_path / "m.coeff")
    s = Scene("cornell-srgb", texture="test-img.png", uplift="jh", jh_res=16, jh_coeff_path=path)
    res, scale, data = s.jh_model()
    assert res == 16 and os.path.getsize(path) == 8 + 4 * 16 + 4 * 3 * 16 ** 3 * 3 and open(path, "rb").read(4) == b"SPEC"
    s2 = Scene("cornell-srgb", texture="test-img.png", uplift="jh", jh_coeff_path=path)   # loads the file
    assert np.array_equal(s2.jh_model()[2], data)
    o = ol.Oracle("cornell-srgb", texture="test-img.png", jh=(res, scale, data))
    rs = np.random.RandomState(5)
    worst = 0.0
    xb, yb, zb = (o.spectrum(n)[0].astype(np.float64) for n in ("xbar", "ybar", "zbar"))
    d65 = o.spectrum("D65_rad")[0].astype(np.float64)[16:]          # 380..780 of the 300..780 table
    m = np.array([o.lib.orc_color_matrix(o.color, b"xyz_to_lrgb")[i] for i in range(9)], dtype=np.float64).reshape(3, 3).T
    for _ in range(300):
        rgb = rs.uniform(0.03, 0.97, 3).astype(np.float32)
        co = (C.c_float * 3)()
        o.lib.orc_jh_fetch(o.color, (C.c_float * 3)(*rgb), co)
        spec = np.array([o.lib.orc_jh_eval_precise(co, np.float32(380 + 5 * k)) for k in range(81)], dtype=np.float64)
        assert spec.min() >= 0.0 and spec.max() <= 1.0
        xyz = np.array([(spec * d65 * b).sum() * 5.0 for b in (xb, yb, zb)])
        worst = max(worst, np.abs(m @ xyz - rgb).max())
    assert worst < 0.05          # res 16 is coarse; res 64 reaches ~1e-3
    with pytest.raises(SsxError) as e:
        Scene("cornell-srgb", texture="test-img.png", uplift="jh", observer=2006)
    assert e.value.code == -3    # src/stdafx.hpp:107-109


@pytest.mark.parametrize("scene", ["cornell", "cornell-srgb", "plane-srgb"])
def test_rgb_mode_host_scene_equals_the_oracle(scene):
    """RENDER_MODE_RGB: the host encodes every lRGB triple as the table {r,g,b,0} on the grid 0,1,2,3
    (include/ssx.h, SSX_MODE_RGB); per quad those triples must be the oracle's (src/scene.cpp:69-82,
    106,300-314,337-343), and the output transform is the sRGB transfer function alone."""
    s = Scene(scene, texture="test-img.png", render_mode="rgb")
    o = ol.Oracle(scene, texture="test-img.png", rgb=True)
    d = s.desc.contents
    assert d.uplift == _capi.SSX_MODE_RGB and (d.lambda_min, d.lambda_step) == (0.0, 1.0)
    samples = np.ctypeslib.as_array(d.samples, shape=(d.n_samples,))
    for i in range(d.n_spectra):
        sp = d.spectra[i]
        assert (sp.n, sp.low, sp.delta_recip) == (4, 0.0, 1.0) and samples[sp.offset + 3] == 0.0
    npr, nl = C.c_int(), C.c_int()
    o.lib.orc_scene_counts(o.scene, C.byref(npr), C.byref(nl), None)
    assert (d.n_quads, d.n_lights) == (npr.value, nl.value)
    for q in range(d.n_quads):
        m = d.materials[d.quads[q].material]
        want = np.zeros(6, np.float32)
        mode = o.lib.orc_scene_material_rgb(o.scene, o.lib.orc_scene_quad_material(o.scene, q), want.ctypes.data_as(C.POINTER(C.c_float)))
        assert mode == m.albedo_mode
        e = d.spectra[m.emission_spectrum]
        assert np.array_equal(samples[e.offset:e.offset + 3], want[:3]), q
        if mode == 0:
            a = d.spectra[m.albedo_spectrum]
            assert np.array_equal(samples[a.offset:a.offset + 3], want[3:]), q
        assert bool(d.quads[q].flags & 1) == bool((want[:3] > 0).any())
    x = np.random.RandomState(1).uniform(0, 2, (64, 4)).astype(np.float32)
    assert np.array_equal(s.xyza_to_srgba(x).view(np.uint32), o.to_srgba(x).view(np.uint32))
    with pytest.raises(SsxError):
        Scene(scene, texture="test-img.png", render_mode="nope")


def test_generated_pass1_header_is_up_to_date():
    """csrc/ssx_pass1_gen.h (pass 1 specialised to the built-in scenes' mesh topologies) is generated from the host's
    scene builder by tools/gen_pass1.py and committed: regenerating must give the same text."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, os.path.join(root, "tools", "gen_pass1.py"), "--check"]).returncode == 0


def test_runtime_pass1_generator_equals_the_committed_one():
    """ssx_set_jit compiles pass 1 for an uploaded scene's own mesh topology; its C++ generator (csrc/ssx_jit.h) must write what
    tools/gen_pass1.py wrote into csrc/ssx_pass1_gen.h for the two built-in topologies, character for character (no device
    needed: ssx_debug_pass1_source only generates text)."""
    import ctypes as C
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import gen_pass1
    from simple_spectral_amd import build as b
    lib = C.CDLL(b.HIP_LIB)
    lib.ssx_debug_pass1_source.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_char_p, C.c_char_p, C.c_size_t]
    header = open(os.path.join(root, "simple_spectral_amd", "csrc", "ssx_pass1_gen.h")).read()
    for name, _tid, scene, cull in gen_pass1.TOPOLOGIES:
        vids = gen_pass1.scene_vids(scene)
        flat = (C.c_uint8 * (4 * len(vids)))(*[v for row in vids for v in row])
        buf = C.create_string_buffer(1 << 20)
        n = lib.ssx_debug_pass1_source(flat, len(vids), name.encode(), buf, len(buf))
        assert 0 < n < len(buf)
        text = buf.value.decode()
        assert text == "\n".join(gen_pass1.emit_topology(name, vids)) + "\n"
        # (the committed header's plane topology also culls the triangles behind the ray's origin, which the run-time generator does not: tools/gen_pass1.py)
        assert ("\n".join(gen_pass1.emit_topology(name, vids, cull)) + "\n") in header and (cull or text in header)
    # and a pattern of its own: two quads sharing an edge, one apart
    vids = [[0, 1, 2, 3], [1, 4, 5, 2], [6, 7, 8, 9]]
    flat = (C.c_uint8 * 12)(*[v for row in vids for v in row])
    buf = C.create_string_buffer(1 << 16)
    lib.ssx_debug_pass1_source(flat, 3, b"jit", buf, len(buf))
    text = buf.value.decode()
    assert text == "\n".join(gen_pass1.emit_topology("jit", vids)) + "\n"
    assert "10 distinct vertices of 12 corners, 14 distinct edges of 15" in text and text.count("// quads") == 2


def test_one_hip_runtime_whatever_the_import_order():
    """"torch must initialise first" was a usage rule.  Now a mechanism: simple_spectral_amd/_capi.py maps
    ONE libamdhip64 into the process in either import order (torch's bundled copy when torch is installed, so that streams and
    device pointers can be handed between the two), checks that it stayed one, and the C library itself refuses to create a
    context in a process that holds two (a host that bypassed the Python loader).  No GPU needed: the checks precede any device call."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    head = "import sys; sys.path.insert(0, %r)\nfrom simple_spectral_amd import _capi\n" % root
    for first in ("_capi.hip_lib()\nimport torch\n", "import torch\n_capi.hip_lib()\n"):
        out = subprocess.run([sys.executable, "-c", head + first + "print(len(_capi.mapped_hip_runtimes()))"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "1", (first, out.stdout, out.stderr[-1500:])
    # two runtimes on purpose: /opt/rocm's by path, then torch (which maps its own copy beside it)
    two = head + ("import ctypes as C\nC.CDLL('/opt/rocm/lib/libamdhip64.so.7', mode=C.RTLD_GLOBAL)\nimport torch\n"
                  "print('mapped', len(_capi.mapped_hip_runtimes()))\n"
                  "lib = C.CDLL(_capi._build.HIP_LIB)\nlib.ssx_last_error.restype = C.c_char_p\nctx = C.c_void_p()\n"
                  "print('create', lib.ssx_create(0, C.byref(ctx)), lib.ssx_last_error(None).decode())\n"
                  "try:\n    _capi.hip_lib()\n    print('loader accepted')\nexcept RuntimeError as e:\n    print('loader refused:', e)\n")
    out = subprocess.run([sys.executable, "-c", two], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    if "mapped 2" not in out.stdout:
        pytest.skip("could not provoke two HIP runtimes on this image: " + out.stdout)
    assert ("create %d two HIP runtimes are mapped" % _capi.SSX_ERR_DEVICE) in out.stdout and "loader refused: two HIP runtimes" in out.stdout, out.stdout
