"""The references of tests/test_generate_gpu.py, checked against themselves where no device is needed: orc_camera_sample is the camera part of
orc_render_sample (followed by the rest of the sample it reproduces Oracle.samples), tile_mask_ref.camera_dir in numpy binary64 gives the oracle's
direction bit for bit, the Python slot map is a bijection onto the owned tiles, and the cases reach what they are meant to reach -- asserted on the
reference alone, so that a vacuous run of the device test cannot pass."""
import ctypes as C
import os

import numpy as np
import pytest

import fold_cases as fc
import generate_cases as gc
import oracle_lib as ol
import step_cases as sc
import tile_mask_ref as tm
from simple_spectral_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_new_names_are_in_the_headers_and_the_binding():
    text = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "int ssx_debug_generate(ssx_ctx* ctx, const ssx_render_params* params, uint32_t k0, uint32_t n_k, int pre_hits," in text
    assert "int ssx_generate_info(ssx_ctx* ctx, uint64_t* generate_launches, uint64_t* fused_launches);" in text
    assert "#define SSX_GENERATE_FILL_BYTE 0x%Xu" % _capi.SSX_GENERATE_FILL_BYTE in text
    assert "ssx_debug_generate" in _capi.HIP_SYMBOLS and "ssx_generate_info" in _capi.HIP_SYMBOLS
    assert "#define SSX_ABI_VERSION %d" % _capi.SSX_ABI_VERSION in text    # appended: the version stays
    orc_h = open(os.path.join(ROOT, "oracle", "oracle.h")).read()
    assert "void orc_camera_sample(" in orc_h and "void orc_debug_camera_hit(" in orc_h
    blob = open(os.path.join(ROOT, "simple_spectral_amd", "csrc", "ssx_blob.h")).read()
    assert "#define SSX_NO_SLOT 0x%Xu" % gc.NO_SLOT in blob
    # the fill is a word no record holds in the places the header names: negative as a float, and even
    assert gc.FILL >> 31 == 1 and gc.FILL & 1 == 0


@pytest.mark.parametrize("name", ["cornell-srgb", "prims70", "cornell-srgb-rgb"])
def test_camera_sample_then_the_rest_of_the_sample_reproduces_render_sample(name):
    """orc_camera_sample, then L() as a chain of orc_debug_level from the camera ray and orc_fold_levels for the way back up: the xyza and the final stream
    of Oracle.samples (orc_render_sample), per sample"""
    ctx = gc.context(name)
    orc = ctx.oracle
    lib = sc.bind(orc.lib)
    W, H, spp, seed = 13, 11, 2, 3
    xyza, state, _ = orc.samples(W, H, spp, seed=seed)
    cam = ctx.cam_pos.copy()
    rng, d, lam = ol.Rng(), np.zeros(3, dtype=np.float32), C.c_float()
    lev = np.zeros((1, sc.LEVEL_WORDS), dtype=np.uint32)
    deepest = 0
    for j in range(H):
        for i in range(W):
            for k in range(spp):
                lib.orc_seed_sample(seed, j * W + i, k, C.byref(rng))
                lib.orc_camera_sample(orc.color, orc.scene, C.byref(rng), i, j, W, H, d.ctypes.data_as(C.POINTER(C.c_float)), C.byref(lam))
                # the stream advanced by exactly the sample's draws in front of L()
                again = ol.Rng()
                lib.orc_seed_sample(seed, j * W + i, k, C.byref(again))
                lib.orc_rand_1d(C.byref(again)); lib.orc_rand_1d(C.byref(again))
                if not ctx.rgb:
                    lib.orc_rand_1f(C.byref(again))
                assert (rng.state, rng.inc) == (again.state, again.inc) and (ctx.rgb == (lam.value == 0.0))
                rec = np.zeros(fc.ROW, dtype=np.uint32)
                rec[fc.LAMBDA0] = sc.f2u([lam.value])[0]
                rec[fc.CAM_DIR:fc.CAM_DIR + 3] = d.view(np.uint32)
                orig, direction, ignore, depth = cam.copy(), d.copy(), -1, 0
                while True:
                    lib.orc_debug_level(orc.color, orc.scene, C.byref(rng), orig.ctypes.data, direction.ctypes.data, ignore, depth, lam, 0, lev.ctypes.data, None)
                    rec[fc.LEVEL0 + depth * fc.LEVEL_WORDS:fc.LEVEL0 + (depth + 1) * fc.LEVEL_WORDS] = lev[0, sc.L_LEVEL:sc.L_LEVEL + fc.LEVEL_WORDS]
                    if depth == 0:
                        rec[fc.HIT] = int(lev[0, sc.L_HIT_PRIM].view(np.int32) >= 0)
                        hit = ol.CameraHit()
                        lib.orc_debug_camera_hit(orc.scene, d.ctypes.data_as(C.POINTER(C.c_float)), C.byref(hit))
                        assert hit.prim == int(lev[0, sc.L_HIT_PRIM].view(np.int32))
                        if hit.prim >= 0:
                            assert (hit.which, sc.f2u([hit.dist])[0]) == (int(lev[0, sc.L_HIT_WHICH]), int(lev[0, sc.L_HIT_DIST]))
                            assert (sc.f2u(hit.st[:]) == lev[0, sc.L_HIT_ST:sc.L_HIT_ST + 2]).all()
                    if not lev[0, sc.L_RECURSE]:
                        break
                    orig, direction = sc.u2f(lev[0, sc.L_NEXT_ORIG:sc.L_NEXT_ORIG + 3]).copy(), sc.u2f(lev[0, sc.L_NEXT_DIR:sc.L_NEXT_DIR + 3]).copy()
                    ignore, depth = int(lev[0, sc.L_HIT_PRIM].view(np.int32)), depth + 1
                rec[fc.N] = depth
                deepest = max(deepest, depth)
                out = np.zeros(4, dtype=np.uint32)
                lib.orc_fold_levels(orc.color, orc.scene, rec.ctypes.data, 1, 0, None, out.ctypes.data)
                want = sc.f2u(xyza[j, i, k])
                assert ((out == want) | (np.isnan(sc.u2f(out)) & np.isnan(sc.u2f(want)))).all(), (i, j, k)
                assert rng.state == int(state[j, i, k]), (i, j, k)
    assert deepest >= 2


@pytest.mark.parametrize("name", gc.CONTEXTS)
def test_numpy_camera_dir_equals_the_oracle_bit_for_bit(name):
    """the second opinion on the arithmetic: tile_mask_ref.camera_dir (numpy binary64) on the stream's sub-pixel offsets, normalised and rounded once, on
    every record of every case"""
    ctx = gc.context(name)
    for case in gc.cases_of(name):
        ref = gc.reference(name, case)
        sx, sy = gc.subpixels(case, ref.ijk)
        got = gc.numpy_dirs(ctx, case, ref.ijk, sx, sy)
        assert np.array_equal(got.view(np.uint32), ref.s["dir"].view(np.uint32)), (case.name, np.flatnonzero((got != ref.s["dir"]).any(axis=1))[:8])


def test_the_division_path_is_distinguished_at_24x16():
    """24 x 16 must divide: multiplying by the reciprocal of 24, as the power-of-two path does, changes bits of at least one record's ray -- not at the
    sample indices of the size table (0 of 1152 records: the two evaluations differ in a third of the binary64 image coordinates and in about one float
    record in 10^8), but at k = 708528, seed 3, the first k at which a record of 24 x 16 differs; 16 x 24, the mirror image (the width a power of two, the
    height not), has its first at k = 124628.  (tests/generate_cases.py RECIPROCAL_CASES.)  The power-of-two sizes agree in every record: there the shortcut
    is exact."""
    ctx = gc.context("cornell-srgb")
    by_name = {c.name: c for c in gc.CASES}
    for size, differs in (("24x16/k708528", True), ("16x24/k124628", True), ("24x16", False), ("8x8", False), ("16x8", False), ("64x32", False)):
        case = by_name[size]
        ref = gc.reference("cornell-srgb", case)
        sx, sy = gc.subpixels(case, ref.ijk)
        recip = gc.numpy_dirs(ctx, case, ref.ijk, sx, sy, reciprocal=True)
        n = int((recip.view(np.uint32) != ref.s["dir"].view(np.uint32)).any(axis=1).sum())
        print("%s: %d of %d records differ under multiply-by-reciprocal" % (size, n, len(ref.ijk)))
        assert (n > 0) == differs, (size, n)


def test_slot_map_is_a_bijection_onto_the_owned_tiles():
    """every tile of the image is some slot of exactly one of the `stride` devices, for every layout and for skews beyond tiles_x; and the list is
    tile_mask_ref.slot_tiles', which builds it from dist.tile_owner_mask"""
    for (W, H) in ((29, 23), (13, 11), (64, 32), (37, 1), (1, 37)):
        tiles_x, tiles_y = gc.tiles_of(W, H)
        everything = sorted((x, y) for y in range(tiles_y) for x in range(tiles_x))
        for stride in (1, 2, 3):
            for skew in (0, 1, 5, 7, 9, tiles_x, tiles_x + 1):
                seen = []
                for first in range(stride):
                    case = gc.Case("", W, H, 0, 1, 0, first, stride, skew)
                    tiles = gc.slot_tiles(case)
                    assert tiles == tm.slot_tiles(W, H, first, stride, skew), (W, H, first, stride, skew)
                    seen += tiles
                assert sorted(seen) == everything, (W, H, stride, skew)
    for case in gc.CASES:
        i, j, k, inside = gc.record_pixels(case)
        px = np.stack([i[inside], j[inside], k[inside]], axis=1)
        assert len(np.unique(px, axis=0)) == len(px)                                # no pixel and sample twice
        if (case.first, case.stride) == (0, 1):
            assert len(px) == case.W * case.H * case.n_k                             # ... and all of them
    assert {c.skew for c in gc.LAYOUT_CASES if c.skew > gc.tiles_of(c.W, c.H)[0]} >= {5, 7, 9}
    # the large image: as many pixels as the API admits, more than 65 535 tiles across, its last slot the last tile, ragged on both sides
    large = {c.name: c for c in gc.CASES}["large"]
    assert large.W * large.H <= 1 << 28 < (large.W + 8) * large.H and gc.tiles_of(large.W, large.H)[0] > 0xFFFF
    tiles = gc.slot_tiles(large)
    assert len(tiles) == 14 and tiles[-1] == (gc.tiles_of(large.W, large.H)[0] - 1, gc.tiles_of(large.W, large.H)[1] - 1)
    _, _, _, inside = gc.record_pixels(large)
    assert not inside[-1].all() and inside[-1].any() and large.W % 8 and large.H % 8


def test_the_cases_cover_what_the_issue_lists():
    sizes = {(c.W, c.H) for c in gc.SIZE_CASES}
    assert sizes >= {(8, 8), (16, 8), (64, 32), (24, 16), (13, 11), (1, 1), (1, 37), (37, 1)}
    assert {c.n_k for c in gc.SIZE_CASES} >= {1, 3} and {c.k0 for c in gc.SIZE_CASES} == {0, 5, (1 << 32) - 4}
    assert {c.seed for c in gc.SIZE_CASES} == {0, 3, (1 << 64) - 1}
    assert any(c.k0 == (1 << 32) - 4 and c.n_k == 3 and c.seed == (1 << 64) - 1 for c in gc.SIZE_CASES)      # k + 1 = 2^32 - 1 under a seed of 2^64 - 1
    assert {(c.first, c.stride, c.skew) for c in gc.LAYOUT_CASES} >= {(0, 1, 0), (1, 3, 0), (0, 2, 1), (2, 3, 5)}
    tx, ty = gc.tiles_of(gc.LAYOUT_CASES[0].W, gc.LAYOUT_CASES[0].H)
    assert tx >= 4 and ty >= 3
    assert {gc.context(n).observer for n in gc.CONTEXTS} == {1931, 2006} and any(gc.context(n).rgb for n in gc.CONTEXTS)
    assert {gc.context(n).n_prims for n in gc.CONTEXTS} >= {33, 70, 128}


@pytest.mark.parametrize("name", gc.CONTEXTS)
def test_the_reference_reaches_hits_misses_primitive_groups_and_both_albedo_modes(name):
    ctx = gc.context(name)
    refs = [gc.reference(name, case) for case in gc.cases_of(name)]
    n = sum(len(r.ijk) for r in refs)
    hits = sum(int(r.hit.sum()) for r in refs)
    prims = np.unique(np.concatenate([r.s["prim"][r.hit] for r in refs]))
    print("%s: %d records, %.1f %% hit, %d of %d primitives hit" % (name, n, 100.0 * hits / n, len(prims), ctx.n_prims))
    assert hits >= 0.3 * n
    if name in gc.OPEN_SCENES:
        assert n - hits >= 0.05 * n
        modes = set(ctx.albedo_mode[prims].tolist())
        assert 0 in modes and modes - {0}, modes                   # hit_st computed for some hits and left out for others
    else:
        assert hits == n                                            # plane-srgb and the closed rooms: no ray leaves
    if ctx.n_prims > 16:
        assert (prims >= 16).any()
    if ctx.n_prims > 32:
        assert (prims >= 32).any()
    if name == "triangles":
        assert 8 in prims or 9 in prims                             # a top-level triangle primitive
    if name == "plane-srgb":
        assert (ctx.albedo_mode[prims] != 0).all()
    if ctx.rgb:
        assert all((r.s["lambda_0"] == 0.0).all() for r in refs)
    else:
        lam = np.concatenate([r.s["lambda_0"] for r in refs])
        assert lam.min() > 0.0 and len(np.unique(lam)) > n // 2
    # words(): a miss has the end-of-path st and the miss record, a hit the live stream
    for r in refs[:3]:
        ray, st, hit = r.words(1)
        ray0, st0, hit0 = r.words(0)
        assert (hit0 == gc.FILL).all() and np.array_equal(ray, ray0)
        assert (ray[~r.inside] == gc.FILL).all() and (st[~r.inside] == gc.FILL).all() and (hit[~r.inside] == gc.FILL).all()
        assert not (ray[r.inside] == gc.FILL).all(axis=1).any() and not (st[r.inside] == gc.FILL).all(axis=1).any() and not (hit[r.inside] == gc.FILL).all(axis=1).any()
        assert not (st0[r.inside] == gc.FILL).all(axis=1).any()
        y = st[r.inside][~r.hit][:, 1]
        assert ((y & 1) == 0).all() and (((y >> 1) & 1) == 0).all() and (((y >> 2) & 0xF) == 0).all() and (((y >> 6) & 0x1FFF) == gc.NO_SLOT).all()
        assert np.array_equal(st[r.inside][r.hit], st0[r.inside][r.hit]) and (st0[r.inside][:, 2] & 1).all()      # inc is odd
