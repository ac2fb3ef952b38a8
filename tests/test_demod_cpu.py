"""Demodulated denoising, the parts that need no GPU: the numpy restatement (tests/demod_ref.py; the GPU kernels are compared with it bit for bit in
test_demod_gpu.py) against the guide buffers' restatement and against itself, the mode's effect on the luminance of low-sample oracle renders at the chosen
defaults, and the presence of the new entry points and their ctypes mirrors.  The oracle renders are tests/test_denoise_cpu.py's: 72 x 40, 16 spp in 4 batches,
held against 1024 spp.  The oracle returns a sample's XYZ, not its hero flux, so it has no wavelength bins: the conditions on the bins are held where bins exist,
by test_demod_gpu.py::test_quality_against_a_1024_spp_render on the same renders."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import demod_ref as mr
import denoise_ref as dr
import oracle_lib as ol
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.renderer import develop_weights
from test_denoise_cpu import QH, QW, noisy_and_reference, rmse_y
from test_denoise_spectral_cpu import header_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
bits = mr.bits
QBINS = 16         # the bins behind the channel albedo of these tests


@functools.lru_cache(maxsize=None)
def albedo_of(scene, B=QBINS, K=mr.DEFAULT_SUPERSAMPLE):
    o = ol.Oracle(scene, texture="test-img.png")
    col = C.cast(o.color, C.POINTER(dr._OrcColorHead)).contents
    rho = mr.albedo_bins(o, QW, QH, B, K)
    return rho, develop_weights(B, float(col.lambda_min), float(col.lambda_step))


def image_only(image, var, prim, rho, wc, floor, levels, sigma_l):
    """the mode's image and variance (the bins' channels do not enter the weights: a single zero channel stands in for them)"""
    rho_c = mr.channel_albedo(rho, wc)
    B = rho.shape[-1]
    e0 = np.zeros(image.shape[:2] + (B + B // 4,), dtype=F)
    _, c1, v1, valid = mr.demodulate(e0, image, var, rho, rho_c, floor)
    cL, vL = dr.atrous(c1, v1, prim, np.zeros_like(image), levels=levels, sigma_l=sigma_l, sigma_a=1.0) if levels else (c1, v1)
    _, c_out, v_out = mr.remodulate(e0, cL, vL, rho, rho_c, floor, valid)
    return c_out, v_out


# ---- the reference against itself ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_one_ray_and_four_bins_are_the_guides_albedo(scene):
    _, _, g, _ = noisy_and_reference(scene)
    rho = albedo_of(scene, 4, 1)[0]
    assert np.array_equal(bits(rho), bits(g["albedo"]))
    assert not np.array_equal(bits(albedo_of(scene, 4, 2)[0]), bits(rho))                    # four rays see more than the centre


@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_demodulating_and_remodulating_without_a_level_is_the_identity_within_an_ulp(scene):
    """(x / r) * r: two roundings, each within half an ulp of its own result, so the relative error is at most (1 + u)^2 - 1 with u = 2^-24.  An ulp of x is
    between u and 2 u of x, so the general bound is two ulps and one ulp is what the definition of the mode is asked to keep: the check holds every bin,
    channel and variance of both renders to ONE ulp (np.spacing of the larger of the two magnitudes).  var goes through r * r both ways: the same two roundings."""
    image, var, g, _ = noisy_and_reference(scene)
    rho, wc = albedo_of(scene)
    e = np.random.default_rng(1).uniform(0, 50, size=(QH, QW, QBINS + QBINS // 4)).astype(F)
    rho_c = mr.channel_albedo(rho, wc)
    e1, c1, v1, valid = mr.demodulate(e, image, var, rho, rho_c, mr.DEFAULT_FLOOR)
    assert valid.all() and not np.array_equal(bits(c1), bits(image))
    back = np.concatenate([e1[..., :QBINS] * mr.floored(rho, mr.DEFAULT_FLOOR), e1[..., QBINS:]], axis=-1)
    e1[..., QBINS:] = F(1)                                                                   # counts of 1: the ratio is the sum channel itself
    out, c2, v2 = mr.remodulate(e1, c1, v1, rho, rho_c, mr.DEFAULT_FLOOR, valid)
    assert np.array_equal(bits(out), bits(back[..., :QBINS]))
    for got, want in ((out, e[..., :QBINS]), (c2, image), (v2, var)):
        ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(F))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    assert np.array_equal(bits(c2[..., 3]), bits(image[..., 3]))                             # alpha is untouched


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["cornell-srgb", "plane-srgb"])
def test_luminance_error_at_the_defaults(scene):
    """Y RMSE against the 1024-spp oracle render, 72 x 40, 16 spp in 4 batches, each mode at its defaults (DESIGN.md section 15 has the scan the defaults come
    from).  plane-srgb: unfiltered 1276.60, plain filter 648.97, demodulated 571.83 -- asserted: demodulated < plain.  cornell-srgb: unfiltered 1281.18, plain
    1189.64, demodulated 1186.67 -- asserted: demodulated <= unfiltered; against the plain filter it is recorded only."""
    image, var, g, ref = noisy_and_reference(scene)
    rho, wc = albedo_of(scene)
    plain, _ = dr.atrous(image, var, g["prim"], g["albedo"], **dr.DEFAULTS)
    demod, _ = image_only(image, var, g["prim"], rho, wc, mr.DEFAULT_FLOOR, 5, mr.DEFAULT_SIGMA_L)
    before, a, b = rmse_y(image, ref), rmse_y(plain, ref), rmse_y(demod, ref)
    print("%s: Y RMSE %.6g unfiltered, %.6g plain filter, %.6g demodulated" % (scene, before, a, b))
    if scene == "plane-srgb":
        assert b < a
    else:
        assert b <= before


# ---- presence -----------------------------------------------------------------------------------------------------------------------------------------------

NEW = ("ssx_albedo_bins", "ssx_denoise_spectral_demod", "ssx_spectral_develop_demod")


def test_the_library_exports_the_new_symbols_and_the_mirrors_match_the_header(tmp_path):
    if not os.path.exists(sbuild.HIP_LIB):
        sbuild.build_hip()
    lib = _capi.hip_lib()
    kinds = {"ptr": (C.c_void_p,), "uint32_t": (C.c_uint32,)}
    for s in NEW:
        assert s in _capi.HIP_SYMBOLS and hasattr(lib, s), s
        want, got = header_parameters(s), getattr(lib, s).argtypes
        assert len(want) == len(got), (s, want, got)
        for w, g in zip(want, got):
            assert g in kinds[w] or (w == "ptr" and issubclass(g, C._Pointer)), (s, w, g)
    assert lib.ssx_abi_version() == _capi.SSX_ABI_VERSION == 2                               # appended: the same ABI version
    src = ('#include "ssx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %.9g %.9g\\n",sizeof(ssx_demod_params),'
           'offsetof(ssx_demod_params,supersample),offsetof(ssx_demod_params,albedo_floor),(double)SSX_DEMOD_DEFAULT_FLOOR,(double)SSX_DEMOD_DEFAULT_SIGMA_L);return 0;}')
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    S = _capi.SsxDemodParams
    out = subprocess.check_output([str(tmp_path / "t")]).split()
    assert list(map(int, out[:3])) == [C.sizeof(S), S.supersample.offset, S.albedo_floor.offset] == [12, 4, 8]
    assert float(out[3]) == _capi.SSX_DEMOD_DEFAULT_FLOOR == float(mr.DEFAULT_FLOOR) and float(out[4]) == _capi.SSX_DEMOD_DEFAULT_SIGMA_L == mr.DEFAULT_SIGMA_L


def test_the_command_line_and_the_host_library_name_the_mode():
    sbuild.build_host()
    cli = os.path.join(ROOT, "simple-spectral")
    p = subprocess.run([cli, "--help"], cwd=ROOT, capture_output=True, text=True)
    assert "--demodulate" in p.stdout and "--albedo-output" in p.stdout
    common = [cli, "-s=cornell-srgb", "-w=16", "-h=8", "-o=/dev/null", "-spp=8"]
    p = subprocess.run(common + ["--demodulate"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--spectral-denoise" in p.stderr                            # a mode of that filter
    p = subprocess.run(common + ["--spectral-output=/dev/null", "--spectral-denoise", "--demodulate=3"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--demodulate" in p.stderr
    p = subprocess.run(common + ["--albedo-output=/dev/null"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0 and "--spectral-bins" in p.stderr
    names = subprocess.check_output(["nm", "-D", "--defined-only", sbuild.HOST_LIB], text=True)
    assert "_ZN3ssx8Renderer11albedo_binsE" in names and "_ZN3ssx8Renderer16save_albedo_binsE" in names
