"""Denoising the spectral bins, the parts that need no GPU: the numpy restatement of the extra channels (tests/denoise_spectral_ref.py; the GPU kernels are
compared with it bit for bit in test_denoise_spectral_gpu.py) against the existing restatement of the filter and against properties of the definition, and
the presence of the two entry points, their ctypes mirrors and the command-line flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_spectral_ref as sr
from simple_spectral_amd import _capi, build as sbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
F = np.float32
bits = sr.bits
SIZES = ((72, 40), (20, 12), (16, 8), (5, 3))
SIGMAS = (dict(sigma_l=dr.DEFAULTS["sigma_l"], sigma_a=dr.DEFAULTS["sigma_a"]), dict(sigma_l=4.0, sigma_a=0.037))


# ---- the restatement against the existing one ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("res", SIZES)
def test_image_and_variance_are_the_filters_and_xyz_as_extras_follow_them(res):
    W, H = res
    c, var, prim, albedo = dr.synthetic(W, H, seed=W * 100 + H)
    for levels in range(1, 7):
        for sig in SIGMAS:
            want_c, want_v = dr.atrous(c, var, prim, albedo, levels=levels, **sig)
            got_c, got_v, got_e = sr.atrous_channels(c, var, prim, albedo, c[..., :3], levels=levels, **sig)
            assert np.array_equal(bits(got_c), bits(want_c)) and np.array_equal(bits(got_v), bits(want_v)), (res, levels, sig)
            assert np.array_equal(bits(got_e), bits(want_c[..., :3])), (res, levels, sig)      # the NaN pixel included: it keeps what it has


# ---- the ratio --------------------------------------------------------------------------------------------------------------------------------------

def test_a_constant_mean_under_varying_counts_comes_back():
    """One primitive, every pixel valid, per-bin mean mu[b] everywhere, counts N[p][m] drawn from 0..3 (a third of them 0), n = 16 samples: S = mu * N is exact
    in binary64, so e0[b] = fl(mu[b] * N / n) and e0[B + m] = fl(N / n) carry a relative error of at most u = 2^-24 each (or are exactly 0).  A level
    replaces a channel by sum(w * e) / sw over T <= 25 counted taps with positive w and non-negative e: each product errs by u, the T - 1 additions of
    non-negative terms by (T - 1) u at most, the division by u -- (T + 1) u <= 26 u on top of the inputs' relative error, which a positive combination does
    not enlarge.  The exact combinations of numerator and denominator are in the ratio mu[b] (same weights, same sw), so after L levels each side is within
    (1 + 26 L) u of its exact value and the quotient, one more rounding, within (2 (1 + 26 L) + 1) u of mu[b]; 1 % is added for the second-order terms.
    L = 5: 263 u = 1.57e-5."""
    H, W, B, n, L = 24, 31, 16, 16, 5
    M = B // 4
    g = np.random.default_rng(7)
    c = g.uniform(0.5, 4, size=(H, W, 4)).astype(F)
    var = (g.uniform(0.05, 0.5, size=(H, W)) ** 2).astype(F)
    prim = np.zeros((H, W), dtype=np.uint32)
    albedo = g.uniform(0, 1, size=(H, W, 4)).astype(F)
    mu = g.uniform(0.25, 40.0, size=B).astype(F)
    N = g.integers(0, 4, size=(H, W, M)).astype(np.uint32)
    S = mu.astype(np.float64)[None, None, :] * np.tile(N, (1, 1, 4)).astype(np.float64)
    out, _, _ = sr.denoise_spectral(S, N, n, c, var, prim, albedo, levels=L)
    empty = np.tile(N, (1, 1, 4)) == 0
    assert empty.mean() > 0.2 and (out[empty] != 0).all()                                  # a bin without a sample is filled from the neighbours
    bound = (2 * (1 + 26 * L) + 1) * 2.0 ** -24 * 1.01
    rel = np.abs(out.astype(np.float64) - mu.astype(np.float64)) / mu.astype(np.float64)
    print("largest relative deviation %.3g, bound %.3g" % (rel.max(), bound))
    assert (rel <= bound).all()


# ---- non-finite extras ---------------------------------------------------------------------------------------------------------------------------------

def clean_inputs(W, H, seed, E):
    c, var, prim, albedo = dr.synthetic(W, H, seed)
    bad = ~dr.valid_mask(c, var)
    c[bad] = np.abs(np.nan_to_num(c[bad], nan=1.0, posinf=1.0)); var[bad] = F(0.01)
    e = np.random.default_rng(seed + 1).uniform(-1, 3, size=(H, W, E)).astype(F)
    return c, var, prim, albedo, e


@pytest.mark.parametrize("value", [np.inf, np.nan])
def test_a_non_finite_extra_in_a_valid_pixel_spreads_only_to_the_pixels_that_tap_it(value):
    H, W, E = 21, 33, 5
    c, var, prim, albedo, e = clean_inputs(W, H, 11, E)
    y0, x0, j0 = 9, 14, 3
    e2 = e.copy(); e2[y0, x0, j0] = F(value)
    yy, xx = np.mgrid[0:H, 0:W]
    # one level: exactly the pixels with a counted tap at (x0, y0) -- at most two steps away in each direction and of the same primitive (all are valid)
    clean = sr.atrous_channels(c, var, prim, albedo, e, levels=1)
    out = sr.atrous_channels(c, var, prim, albedo, e2, levels=1)
    taps = (np.abs(yy - y0) <= 2) & (np.abs(xx - x0) <= 2) & (prim == prim[y0, x0])
    assert 9 < taps.sum() < 25                                                              # (a primitive edge runs through the footprint)
    assert np.array_equal(~np.isfinite(out[2][..., j0]), taps)
    other = np.ones(E, dtype=bool); other[j0] = False
    assert np.array_equal(bits(out[2][..., other]), bits(clean[2][..., other]))           # the other channels of every pixel
    assert np.array_equal(bits(out[2][~taps]), bits(clean[2][~taps]))
    assert np.array_equal(bits(out[0]), bits(clean[0])) and np.array_equal(bits(out[1]), bits(clean[1]))   # the weights never depend on e
    # three levels: nothing beyond the sum of the levels' reaches
    L = 3
    clean = sr.atrous_channels(c, var, prim, albedo, e, levels=L)
    out = sr.atrous_channels(c, var, prim, albedo, e2, levels=L)
    reach = sum(2 * (1 << l) for l in range(L))
    far = (np.abs(yy - y0) > reach) | (np.abs(xx - x0) > reach) | (prim != prim[y0, x0])
    assert far.any() and np.array_equal(bits(out[2][far]), bits(clean[2][far])) and np.isfinite(out[2][far]).all()
    assert not np.isfinite(out[2][y0, x0, j0])
    assert np.array_equal(bits(out[0]), bits(clean[0])) and np.array_equal(bits(out[1]), bits(clean[1]))


def test_a_non_finite_extra_in_an_invalid_pixel_spreads_nowhere():
    H, W, E = 21, 33, 5
    c, var, prim, albedo, e = clean_inputs(W, H, 12, E)
    y0, x0 = 10, 15
    var[y0, x0] = F(np.inf)                                                                 # invalid by its variance
    e2 = e.copy(); e2[y0, x0, 1] = F(np.nan); e2[y0, x0, 4] = F(-np.inf)
    clean = sr.atrous_channels(c, var, prim, albedo, e, levels=4)
    out = sr.atrous_channels(c, var, prim, albedo, e2, levels=4)
    here = np.zeros((H, W), dtype=bool); here[y0, x0] = True
    assert np.array_equal(bits(out[2][~here]), bits(clean[2][~here])) and np.isfinite(out[2][~here]).all()
    assert np.array_equal(bits(out[2][y0, x0]), bits(e2[y0, x0]))                          # it keeps its e at every level
    assert np.array_equal(bits(out[0]), bits(clean[0])) and np.array_equal(bits(out[1]), bits(clean[1]))


# ---- presence ------------------------------------------------------------------------------------------------------------------------------------------

NEW = ("ssx_denoise_channels", "ssx_denoise_spectral")


def test_the_libraries_export_the_new_symbols():
    sbuild.build_host()
    if not os.path.exists(sbuild.HIP_LIB):
        sbuild.build_hip()
    lib = C.CDLL(sbuild.HIP_LIB)
    for s in NEW:
        assert s in _capi.HIP_SYMBOLS and hasattr(lib, s), s
    # libssx_host.so: the C++ host's methods (Itanium names carry the class and the method)
    names = subprocess.check_output(["nm", "-D", "--defined-only", sbuild.HOST_LIB], text=True)
    assert re.search(r"\b_ZN3ssx8Renderer16denoise_spectralE", names), "Renderer::denoise_spectral"
    assert len(re.findall(r"\b_ZN3ssx8Renderer19save_spectral_imageE", names)) == 2, "Renderer::save_spectral_image(path) and (path, bins)"


def header_parameters(name):
    """the parameter types of `int name(...)` in include/ssx.h, comments removed: "ptr" for every pointer, else the type's name"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssx.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    return ["ptr" if "*" in p else p.split()[-2] for p in m.group(1).split(",")]


def test_the_ctypes_mirrors_match_the_header():
    lib = _capi.hip_lib()
    kinds = {"ptr": (C.c_void_p,), "uint32_t": (C.c_uint32,)}
    for s in NEW:
        want, got = header_parameters(s), getattr(lib, s).argtypes
        assert len(want) == len(got), (s, want, got)
        for w, g in zip(want, got):
            assert g in kinds[w] or (w == "ptr" and issubclass(g, C._Pointer)), (s, w, g)
    assert header_parameters("ssx_denoise_channels") == ["ptr"] * 2 + ["uint32_t"] * 2 + ["ptr"] * 4 + ["uint32_t"] + ["ptr"] * 4
    assert header_parameters("ssx_denoise_spectral") == ["ptr"] * 5
    assert lib.ssx_abi_version() == _capi.SSX_ABI_VERSION == 2                             # appended: the same ABI version


def test_the_command_line_names_the_flag():
    sbuild.build_host()
    p = subprocess.run([CLI, "--help"], cwd=ROOT, capture_output=True, text=True)
    assert "--spectral-denoise" in p.stdout
    common = [CLI, "-s=cornell-srgb", "-w=16", "-h=8", "-o=/dev/null"]
    p = subprocess.run(common + ["-spp=8", "--spectral-denoise"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--spectral-output" in p.stderr                           # it requires --spectral-output
    p = subprocess.run(common + ["-spp=1", "--spectral-output=/dev/null", "--spectral-denoise"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "at least two samples" in p.stderr                        # --denoise's refusals
    p = subprocess.run(common + ["-spp=8", "--spectral-output=/dev/null", "--spectral-denoise", "--tile-major"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--tile-major" in p.stderr
    p = subprocess.run(common + ["-spp=8", "--spectral-output=/dev/null", "--spectral-denoise", "--noise-step=8"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--noise-step" in p.stderr
