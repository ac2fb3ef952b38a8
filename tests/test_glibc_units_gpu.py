"""libm = glibc-2.35, function by function on the device: include/ssx_glibc_math.h as the GPU evaluates it against the same header on the
host (every one of the 2^32 inputs, through digests: ssx_debug_sweep SSX_SWEEP_GLIBC_*), and the units the _glibc kernels inline (spherical
triangle, Arvo's sampler, light sampling, cosine hemisphere) against the shim oracle's units (tests/glibc_oracle.py) on random and crafted
degenerate inputs (ssx_debug_eval SSX_DBG_*_GLIBC).  tests/test_glibc_math_cpu.py links the host restatement to glibc itself."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import crafted
import glibc_oracle as go
import oracle_lib as ol
import unit_cases as uc
from simple_spectral_amd import Options, Renderer, _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits_or_both_nan(got_u32, ref_u32, float_cols):
    g, r = np.asarray(got_u32), np.asarray(ref_u32)
    ok = g == r
    for c in float_cols:
        ok[:, c] |= np.isnan(g[:, c].view(np.float32)) & np.isnan(r[:, c].view(np.float32))
    return ok


@pytest.fixture(scope="module")
def cornell():
    return Renderer(Options(scene_name="cornell-srgb", res=(8, 8), spp=1, texture="test-img.png")), go.Oracle("cornell-srgb", texture="test-img.png")


def custom_pair(c):
    orc = go.custom_oracle(c)
    r = Renderer(Options(scene_name="cornell", res=(8, 8), spp=1, observer=c.observer))
    r.upload_scene_desc(c.desc(orc))
    return r, orc


def test_device_restatement_equals_the_host_restatement_on_all_inputs(cornell, tmp_path):
    """Every float through ssx_glibc_sinf / cosf / acosf on the device, summed into a digest the host recomputes with the same header
    (tests/glibc_math_check.c digest: no libm involved); sincosf equal to sinf / cosf on the device for every input; and the one ssx_fmath.h
    function the _glibc kernels keep, ssx_cosf_lds, unchanged by their LDS table."""
    r, _ = cornell
    exe = str(tmp_path / "glibc_math_check")
    subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-fno-builtin", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "glibc_math_check.c"), "-o", exe, "-lm", "-lpthread"])
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    host = subprocess.Popen([exe, "digest", str(threads)], stdout=subprocess.PIPE, text=True)   # (runs while the device sweeps)
    try:
        got = {}
        for name, op in (("sinf", _capi.SSX_SWEEP_GLIBC_SIN), ("cosf", _capi.SSX_SWEEP_GLIBC_COS), ("acosf", _capi.SSX_SWEEP_GLIBC_ACOS)):
            bad, digest, ex = r.debug_sweep(op)
            assert bad == 0, (name, [hex(e) for e in ex])                # sincosf == (sinf, cosf)
            got[name] = digest
        bad, _, ex = r.debug_sweep(_capi.SSX_SWEEP_GLIBC_COS_LDS)
        assert bad == 0, [hex(e) for e in ex]
        out, _ = host.communicate(timeout=600)
    finally:
        if host.poll() is None:
            host.kill()
    want = json.loads(out)
    print(json.dumps({"device": got, "host": want}))
    assert got == want


def test_glibc_functions_equal_the_shim_oracle(cornell):
    r, orc = cornell
    w = uc.fmath_inputs()
    got = r.debug_eval(_capi.SSX_DBG_GLIBC_MATH, w, 5)
    ref = bits(uc.oracle_fmath(orc.lib, w))
    assert same_bits_or_both_nan(got, ref, range(5)).all()
    # and they are not ssx_fmath.h's: the default op differs somewhere on the same inputs
    assert not np.array_equal(got, r.debug_eval(_capi.SSX_DBG_FMATH, w, 5))


def test_spherical_triangle_incl_degenerate_ladder(cornell):
    """src/util/spherical-tri.cpp:18-124 with glibc's acosf / sinf, on random, tiny, coinciding, antipodal, coplanar and NaN vertices"""
    r, orc = cornell
    tri = uc.sphtri_inputs()
    got = r.debug_eval(_capi.SSX_DBG_SPHTRI_GLIBC, uc.f2u(tri), 5)
    ref = bits(uc.oracle_sphtri(orc.lib, tri))
    ok = same_bits_or_both_nan(got, ref, range(5))
    assert ok.all(), (np.argwhere(~ok)[:5], tri[np.argwhere(~ok)[0][0]])


def test_arvo_sampler_incl_denominator_zero(cornell):
    """src/util/random.cpp:101-154 with glibc's sincosf / sinf (the triangles are the shim oracle's, degenerate families included)"""
    r, orc = cornell
    w = uc.arvo_inputs(orc.lib)
    got = r.debug_eval(_capi.SSX_DBG_ARVO_GLIBC, w, 5)
    ref = uc.oracle_arvo(orc.lib, w)
    ok = same_bits_or_both_nan(got, ref, range(3))
    assert ok.all(), np.argwhere(~ok)[:5]


def test_cosine_hemisphere_incl_rejection_retry(cornell):
    r, orc = cornell
    w = uc.coshemi_inputs()
    got = r.debug_eval(_capi.SSX_DBG_COSHEMI_GLIBC, w, 6)
    ref = uc.oracle_coshemi(orc.lib, w)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("view", ["edge_ab", "room"])
def test_light_sampling_from_degenerate_positions(view):
    """src/scene.cpp:417-431 in glibc mode from points on a light edge's extension, on light vertices (NaN directions), in the light's
    plane, and random ones (tests/crafted.py degenerate_light_scene)"""
    c = crafted.degenerate_light_scene(view)
    r, orc = custom_pair(c)
    g = np.random.default_rng(15)
    e = 2e-3
    pts = np.concatenate([
        g.uniform(-3.9, 3.9, size=(2000, 3)),
        np.array([3, 1, 0]) + g.uniform(-e, e, size=(400, 3)) * [0, 1, 1],
        np.array([1, 1, 3]) + g.uniform(-e, e, size=(400, 3)) * [1, 1, 0],
        np.array([[0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1], [0.5, 1, 0.5], [0.5, 1, 0], [2, 1, 2], [-3, 1, 0.5]], dtype=np.float64),
        np.stack([g.uniform(-3, 3, 200), np.full(200, 1.0), g.uniform(-3, 3, 200)], axis=1),
    ]).astype(np.float32)
    w = uc.sample_light_inputs(pts)
    st = ol.Stats()
    orc.lib.orc_debug_set_stats(C.byref(st))
    try:
        ref = uc.oracle_sample_light(orc, w)
    finally:
        orc.lib.orc_debug_set_stats(None)
    if view == "edge_ab":
        assert st.sphtri_half_pi > 0 and st.sphtri_nan > 0      # the degenerate ladder is reached
    got = r.debug_eval(_capi.SSX_DBG_SAMPLE_LIGHT_GLIBC, w, 7)
    ok = same_bits_or_both_nan(got, ref, (0, 1, 2, 4))
    assert ok.all(), (np.argwhere(~ok)[:5], pts[np.argwhere(~ok)[0][0]])
