"""Depth of field without a GPU (include/ssx.h "Depth of field after the render"): the numpy restatement (tests/defocus_ref.py) against what the definition
implies, the shared case list (tests/defocus_cases.py) against the definition's near misses, the host's thin lens (ssh_defocus_thin_lens) against its closed
form, and the parameter struct and the exported symbols against the headers."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import defocus_cases as dc
import defocus_ref as ref
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd.renderer import Scene, SsxError, thin_lens_defocus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def differ(a, b):
    """where two results differ in bits, two NaNs counting as equal (the payload of a NaN an operation makes is not the definition's)"""
    return (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))


def run(case, mutant=None):
    return ref.defocus(case["q"], case["depth"], case["R"], case["K"], case["focus"], mutant=mutant)


@functools.lru_cache(maxsize=None)
def results():
    """the definition on every shared case, computed once"""
    return {c["name"]: run(c) for c in dc.cases()}


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------

def test_no_gain_or_no_radius_is_a_copy():
    g = np.random.default_rng(1)
    q = g.uniform(-3, 3, size=(6, 9, 8)).astype(F)
    q.reshape(-1)[:6] = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0x80000000, 0x00000007, 0x80000001], dtype=np.uint32).view(F)
    depth = g.uniform(1, 9, size=(6, 9)).astype(F)
    focus = np.full(8, 0.3, F)
    assert np.array_equal(bits(ref.defocus(q, depth, 5, 0.0, focus)), bits(q))
    assert np.array_equal(bits(ref.defocus(q, depth, 0, 25.0, focus)), bits(q))
    assert not np.array_equal(bits(ref.defocus(q, depth, 5, 25.0, focus)), bits(q))


def test_the_vectorised_walk_equals_the_scalar_loops():
    g = np.random.default_rng(2)
    q = g.uniform(0.1, 3, size=(7, 9, 4)).astype(F)
    depth = np.where(np.arange(9)[None, :] < 4, F(2.0), F(8.0)) * np.ones((7, 1), F)
    depth[3, 6], depth[0, 0], depth[6, 8] = 0.0, np.nan, np.inf
    q[2, 2, 1], q[5, 7, 3] = np.nan, np.inf
    focus = np.array([0.5, 0.3, 0.125, 0.0], F)
    for R, K in ((1, 4.0), (3, 9.0), (12, 50.0)):
        assert not differ(ref.defocus(q, depth, R, K, focus), ref.scalar_defocus(q, depth, R, K, focus)).any(), R


def test_a_constant_image_stays_constant_to_a_few_ulp():
    """out = sum(w q0) / sum(w) over n <= (2 R + 1)^2 positive terms: each product, each add and the division within (1 + u), so out / q0 lies within
    (1 + u)^(2 n + 2) of 1 -- (2 n + 2) u to first order, the 1.01 covering the rest: 10 ulp at R = 1 (n = 9), the same reasoning at R = 5."""
    q0 = F(1.7)
    g = np.random.default_rng(3)
    depth = g.uniform(1.5, 12.0, size=(20, 23)).astype(F)
    focus = np.linspace(0.5, 0.1, 8).astype(F)
    for R, K in ((1, 3.0), (5, 14.0)):
        out = ref.defocus(np.full((20, 23, 8), q0, F), depth, R, K, focus)
        n = (2 * R + 1) ** 2
        assert (np.abs(out.astype(np.float64) / float(q0) - 1.0) <= 1.01 * (2 * n + 2) * 2.0 ** -24).all(), R
        assert (out != q0).any()


def step_scene(R=5, K=14.0):
    """the near side (columns < 10, depth 2) in focus in every bin, the far side (depth 10) blurred: c = |0.1 - 0.5| * 14 = 5.6 -> R"""
    g = np.random.default_rng(4)
    q = g.uniform(0.5, 3.0, size=(12, 20, 4)).astype(F)
    q[:, 10:, :] += F(5.0)
    depth = np.where(np.arange(20)[None, :] < 10, F(2.0), F(10.0)) * np.ones((12, 1), F)
    return q, depth.astype(F), R, K, np.full(4, 0.5, F)


def test_a_sharp_foreground_stays_clean_against_a_blurred_background():
    q, depth, R, K, focus = step_scene()
    out = ref.defocus(q, depth, R, K, focus)
    inv, c, a = ref.prepare(depth, R, K, focus)
    assert (c[:, :10] == 0).all() and (c[:, 10:] == F(R)).all()
    near = ((a[:, :10] * q[:, :10]) / a[:, :10]).astype(F)                                           # only its own tap: (a * q) / a, not q
    assert np.array_equal(bits(out[:, :10]), bits(near))
    assert not np.array_equal(bits(near), bits(q[:, :10]))                                           # ... which is not a copy (the header says so)
    assert (np.abs(near.astype(np.float64) - q[:, :10]) <= 2 * np.spacing(q[:, :10])).all()
    # without the occlusion rule the bright background leaks over the edge
    leaked = ref.defocus(q, depth, R, K, focus, mutant="no_occlusion")
    assert (leaked[:, 9] > out[:, 9] + F(0.1)).all()


def test_the_far_side_changes_next_to_the_edge():
    q, depth, R, K, focus = step_scene()
    out = ref.defocus(q, depth, R, K, focus)
    assert (out[:, 10:] != q[:, 10:]).all()
    assert (np.abs(out[:, 10] - q[:, 10]) > F(1e-3)).all()                                           # next to the edge, by more than rounding
    assert (out[:, 10:].std(axis=(0, 1)) < q[:, 10:].std(axis=(0, 1))).all()


# ---- the shared cases --------------------------------------------------------------------------------------------------------------------------------------

def test_the_case_list_covers_what_the_issue_names():
    cs = dc.cases()
    assert {c["q"].shape[:2][::-1] for c in cs} >= {(1, 1), (8, 8), (37, 29), (70, 5), (45, 43)}
    assert {c["q"].shape[2] for c in cs} == {4, 12, 64} and {c["R"] for c in cs} == {0, 1, 5, 12}
    assert any(c["R"] > max(c["q"].shape[:2]) for c in cs)
    assert any(min(c["q"].shape[:2]) > 16 + 2 * c["R"] and c["q"].shape[0] % 16 and c["q"].shape[1] % 16 and c["R"] == 12 for c in cs)
    for c in cs:
        if c["q"].shape[1] > 1:
            assert (c["depth"] == 0).any() and len(set(c["depth"][0].tolist())) > 1, c["name"]
        if c["R"] and c["K"] and c["q"].shape[1] > 1:
            inv, cc, a = ref.prepare(c["depth"], c["R"], c["K"], c["focus"])
            assert (cc == 0).any() and (cc == F(c["R"])).any(), c["name"]
        if c["specials"]:
            flat = c["q"].reshape(-1)
            tiny = np.abs(flat[np.isfinite(flat) & (flat != 0)]).min()
            assert np.isnan(flat).sum() == 1 and np.isinf(flat).sum() == 1 and (np.signbit(flat) & (flat == 0)).any() and tiny < np.finfo(F).tiny, c["name"]
            assert np.isnan(c["depth"]).sum() == 1 and np.isposinf(c["depth"]).sum() == 1, c["name"]
    assert sum(c["specials"] and c["R"] > 0 and c["K"] > 0 for c in cs) >= 4


def test_a_non_finite_source_stays_inside_its_own_disc():
    """a NaN or an infinity at source s, bin b reaches destination p only if its tap is taken: dist < ce + 1 <= c[s][b] + 1.  Every other pixel stays finite."""
    for c in dc.cases():
        if not c["specials"]:
            continue
        out = results()[c["name"]]
        H, W, B = out.shape
        reach = np.zeros((H, W, B), dtype=bool)
        if c["R"] == 0 or c["K"] == 0:
            reach = ~np.isfinite(c["q"])
        else:
            inv, cc, a = ref.prepare(c["depth"], c["R"], c["K"], c["focus"])
            yy, xx = np.mgrid[0:H, 0:W]
            for y, x, b in np.argwhere(~np.isfinite(c["q"])):
                dist = np.sqrt(((yy - y) ** 2 + (xx - x) ** 2).astype(F), dtype=F)
                reach[:, :, b] |= dist < cc[y, x, b] + F(1)
            assert reach.any(axis=2).sum() < H * W, c["name"]                                        # each disc covers only a part of the image
        assert np.isfinite(out[~reach]).all(), c["name"]
        assert (~np.isfinite(out)).any(), c["name"]                                                  # ... and inside it the value does arrive


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_the_shared_cases_tell_the_definition_from_a_near_miss(mutant):
    """What the GPU is fed must separate the definition from: a contracted sq + w * q, the dx loop outside, cover * (a * q), the occlusion test dropped, a
    replicated border."""
    hit = [c["name"] for c in dc.cases() if differ(run(c, mutant), results()[c["name"]]).any()]
    assert hit, "no shared case separates the mutant %r from the definition" % mutant


# ---- the host's thin lens ----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    return Scene("cornell-srgb", texture="test-img.png")


@pytest.mark.parametrize("lens", [(16, 64, 0.05, 3.5, 0.0, 550.0), (48, 16, 0.2, 1.25, 0.08, 520.0), (512, 4, 0.0, 2.0, -0.3, 600.0), (29, 12, 1.5, 0.7, -3.0, 450.0)])
def test_the_thin_lens_equals_its_closed_form(lens):
    height, bins, aperture, z_f, axial, lref = lens
    s = scene()
    d = s.desc.contents
    got = thin_lens_defocus(s, height, bins, aperture, z_f, axial=axial, lambda_ref=lref, max_radius=7)
    vfov = C.c_float()
    assert _capi.host_lib().ssh_scene_vfov(s._h, C.byref(vfov)) == 0 and vfov.value == 39.0
    gain, focus = ref.thin_lens(vfov.value, height, bins, d.lambda_min, d.lambda_step, aperture, z_f, axial, lref)
    assert got["max_radius"] == 7 and got["focus"].shape == (bins,) and got["focus"].dtype == F
    assert np.array_equal(bits(got["focus"]), bits(focus))                      # +, *, /, max and the final rounding: correctly rounded on both sides
    assert abs(got["gain"] - float(gain)) <= np.spacing(gain)                   # tan is libm's on both sides; one binary32 ulp covers two libms
    assert (got["focus"] >= 0).all() and (axial >= 0 or aperture == 1.5 or (got["focus"] > 0).all())
    if aperture == 0.0:
        assert got["gain"] == 0.0                                               # no aperture: the identity
    if aperture == 1.5:
        assert (got["focus"] == 0).any() and (got["focus"] > 0).any()           # max(0, .): a bin pushed beyond infinity focuses at infinity


def test_the_thin_lens_refuses_what_it_cannot_make():
    s = scene()
    for kw in (dict(aperture=-1.0), dict(aperture=float("nan")), dict(focus_distance=0.0), dict(focus_distance=float("inf")), dict(axial=float("nan")),
               dict(lambda_ref=0.0), dict(bins=6), dict(height=0), dict(aperture=1e300)):
        args = dict(height=16, bins=8, aperture=0.1, focus_distance=2.0)
        args.update(kw)
        with pytest.raises(SsxError) as e:
            thin_lens_defocus(s, **args)
        assert e.value.code == _capi.SSX_ERR_ARG and "ssh_defocus_thin_lens" in str(e.value), kw


# ---- the struct and the symbols ----------------------------------------------------------------------------------------------------------------------------

def test_the_parameter_struct_matches_the_header():
    src = ('#include "ssx.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %u\\n",sizeof(ssx_defocus_params),'
           'offsetof(ssx_defocus_params,max_radius),offsetof(ssx_defocus_params,gain),offsetof(ssx_defocus_params,focus),SSX_DEFOCUS_MAX_RADIUS);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    P = _capi.SsxDefocusParams
    assert got == [C.sizeof(P), P.max_radius.offset, P.gain.offset, P.focus.offset, _capi.SSX_DEFOCUS_MAX_RADIUS]


def test_the_libraries_export_the_new_symbols():
    hip, host = C.CDLL(sbuild.HIP_LIB), _capi.host_lib()
    for s in ("ssx_defocus_images", "ssx_spectral_develop_lens"):
        assert s in _capi.HIP_SYMBOLS and hasattr(hip, s), s
    for s in ("ssh_defocus_thin_lens", "ssh_scene_vfov"):
        assert s in _capi.HOST_SYMBOLS and hasattr(host, s), s
