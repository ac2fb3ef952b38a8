"""libm = glibc-2.35 on the CPU: include/ssx_glibc_math.h against the host's glibc on every binary32 input, and the shim oracle
(tests/glibc_oracle.py) against oracle/libssx_oracle_libm.so -- the oracle that calls the host's glibc -- per sample.  Both comparisons
need glibc 2.35 on an x86-64 host with FMA and AVX2 (glibc then runs the FMA variant of sinf / cosf that the header restates)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import glibc_oracle as go
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def glibc_version():
    libc = C.CDLL("libc.so.6")
    libc.gnu_get_libc_version.restype = C.c_char_p
    return libc.gnu_get_libc_version().decode()


def cpu_flags():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("flags"):
                return set(line.split(":", 1)[1].split())
    except OSError:
        pass
    return set()


def host_is_the_restated_glibc():
    v, flags = glibc_version(), cpu_flags()
    fma = {"fma", "avx2"} <= flags
    return v == "2.35" and fma, "glibc %s, FMA/AVX2 variant %s" % (v, "selected" if fma else "not available")


needs_glibc_235 = pytest.mark.skipif(not host_is_the_restated_glibc()[0], reason="needs glibc 2.35 with its FMA/AVX2 variant: host has %s"
                                     % host_is_the_restated_glibc()[1])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glibc_math") / "glibc_math_check")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fno-builtin", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "glibc_math_check.c"), "-o", exe, "-lm", "-lpthread"])
    return exe


def run_checker(exe, lo=0, hi=1 << 32):
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    out = subprocess.run([exe, str(threads), str(lo), str(hi)], capture_output=True, text=True, check=True).stdout
    return json.loads(out)


@needs_glibc_235
def test_restatement_matches_glibc_on_hard_ranges(checker):
    """The quick part: the reduction boundaries (|x| around 0.75, 120, 2^-12), the acos ranges and the tails."""
    for lo, hi in ((0x39000000, 0x39900000), (0x3F300000, 0x3F500000), (0x42E00000, 0x43000000), (0xBF000000, 0xBF800001),
                   (0x3F000000, 0x3F800001), (0x7F000000, 0x7FC00001), (0xFF700000, 0xFFC00001)):
        r = run_checker(checker, lo, hi)
        bad = {k: v for k, v in r.items() if isinstance(v, list) and v[0]}
        assert not bad, (hex(lo), hex(hi), bad)


@needs_glibc_235
@pytest.mark.slow
def test_restatement_matches_glibc_on_all_inputs(checker):
    """sinf, cosf, sincosf, acosf: every one of the 2^32 inputs, bit for bit (NaN matches NaN); and (float)cos((double)x) -- the
    reference's random.cpp:134 -- equals ssx_cosf(x) for all 0 <= x <= 4, the range of its argument tri.b * r0 (in [0, pi)), so the glibc
    mode keeps ssx_fmath.h's cosine there (and the shim oracle's cos is ssx_cosf)."""
    r = run_checker(checker)
    print(json.dumps(dict(r, host=host_is_the_restated_glibc()[1])))
    assert r["glibc"] == "2.35" and r["inputs"] == 1 << 32
    for name in ("sinf", "cosf", "sincosf_sin", "sincosf_cos", "acosf", "cos_double_vs_ssx_cosf"):
        assert r[name][0] == 0, (name, r[name])


def test_shim_oracle_uses_no_libm_transcendental():
    """The shim oracle's sinf / cosf / sincosf / acosf / cos are its own: nothing of the kind is left for the dynamic linker to bind to
    the host's libm (which is what makes the GPU tests of the mode independent of the GPU machine's C library)."""
    path = go.library_path()
    assert os.path.exists(path), path
    und = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True, check=True).stdout.split()
    names = {s.split("@")[0] for s in und}
    assert not names & {"sinf", "cosf", "sincosf", "acosf", "cos", "sin", "acos"}, names


@needs_glibc_235
@pytest.mark.parametrize("scene,W,H,spp,seed,io,els", [("cornell-srgb", 24, 16, 8, 3, False, True), ("plane-srgb", 24, 16, 8, 5, False, True),
                                                       ("cornell", 16, 16, 4, 7, True, True), ("plane-srgb", 16, 16, 4, 2, False, False)])
def test_shim_oracle_equals_the_glibc_linked_oracle(scene, W, H, spp, seed, io, els):
    """Per sample -- XYZA, the final PCG32 state (the draws consumed) and the path statistics (levels, rays) -- the shim oracle is the
    oracle linked against the host's glibc (oracle/Makefile's libssx_oracle_libm.so)."""
    tex = None if scene == "cornell" else "test-img.png"
    a = go.Oracle(scene, texture=tex)
    b = ol.Oracle(scene, texture=tex, variant="libm")
    xa, sa, ta = a.samples(W, H, spp, seed=seed, indirect_only=io, els=els)
    xb, sb, tb = b.samples(W, H, spp, seed=seed, indirect_only=io, els=els)
    assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
    assert np.array_equal(sa, sb)
    assert ta.as_dict() == tb.as_dict()


def test_shim_oracle_differs_from_the_build_oracle():
    """The two libm modes are different functions: the same samples through the default oracle differ somewhere."""
    a = go.Oracle("cornell-srgb", texture="test-img.png")
    b = ol.Oracle("cornell-srgb", texture="test-img.png")
    xa, _, _ = a.samples(16, 16, 8, seed=1)
    xb, _, _ = b.samples(16, 16, 8, seed=1)
    assert not np.array_equal(xa.view(np.uint32), xb.view(np.uint32))


def test_render_params_mirror_has_libm():
    from simple_spectral_amd import _capi
    P = _capi.SsxRenderParams
    assert P.libm.offset == P.seed.offset + 8 and C.sizeof(P) == P.libm.offset + 8
    assert _capi.LIBM_MODES == {"build": 0, "glibc-2.35": 1}
