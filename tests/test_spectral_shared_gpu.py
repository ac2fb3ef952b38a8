"""What the spectral fragments share on the device (csrc/ssx_spectral.hip): the ordered reduce behind the probes and the comparison, at row counts around its
unroll of 16, and the rows-into-LDS transposition of the two import kernels, on ragged images of one and of two tile columns.  Bit for bit ("same" compares the
integer views, a NaN equal to any NaN) against tests/spectral_stats_ref.py and tests/spectral_compare_ref.py, and against the exporter's own arrays."""
import functools

import numpy as np
import pytest

import spectral_compare_ref as cref
import spectral_stats_ref as sref
import test_spectral_checkpoint_gpu as ck
import test_spectral_gpu as base
import test_spectral_stats_gpu as stats
from simple_spectral_amd import Options, Renderer

pytestmark = pytest.mark.gpu
same = stats.same
SIZES = [(9, 1), (8, 15), (8, 16), (13, 17), (5, 33)]       # (W, H): the reduce walks H rows, 16 to an unrolled trip
SHAPES = [(4, 1), (64, 32), (12, 5)]                        # (B, R): R * B = 4 and 60 (the comparison's narrow row kernel) and 2048 (the wide one)


@functools.lru_cache(maxsize=None)
def pure():
    """one context for the pure calls: they need no state"""
    return base.renderer("cornell-srgb")


@functools.lru_cache(maxsize=None)
def synthetic(w, h, bins, regions, seed):
    """(S, Q float64 [h, w, bins], N uint32 [h, w, bins / 4], labels uint8 [h, w]): counts of 0, 1, 2 and many, S of either sign with a NaN and a -0.0, Q >= 0, labels
    0..regions-1 with some 255; read-only"""
    rng = np.random.default_rng([seed, w, h, bins, regions])
    N = rng.choice(np.array([0, 1, 2, 3, 17, 1000], dtype=np.uint32), size=(h, w, bins // 4))
    S = rng.normal(0.0, 3.0, (h, w, bins)) * np.tile(N, (1, 1, 4))
    Q = S * S / np.maximum(np.tile(N, (1, 1, 4)), 1) + rng.gamma(2.0, 2.0, (h, w, bins)) * (np.tile(N, (1, 1, 4)) >= 2)
    S[h - 1, w - 1, 1], S[0, w // 2, bins - 1] = np.nan, -0.0
    labels = rng.integers(0, regions, (h, w)).astype(np.uint8)
    labels[rng.random((h, w)) < 0.2] = 255
    labels[h // 2, 0] = 255
    for a in (S, Q, N, labels):
        a.setflags(write=False)
    return S, Q, N, labels


@pytest.mark.parametrize("bins,regions", SHAPES)
@pytest.mark.parametrize("w,h", SIZES)
def test_probe_arrays_around_the_unroll(w, h, bins, regions):
    S, Q, N, labels = synthetic(w, h, bins, regions, 1)
    n = np.tile(N, (1, 1, 4))
    assert w * h < 40 or all((n == k).any() for k in (0, 1, 2, 1000))
    got, want = pure().probe_arrays(S, Q, N, labels, regions), sref.probe(S, Q, N, labels, regions)
    for name, g, x in zip(("SS", "NN", "VV", "UU"), got, want):
        assert same(g, x), name
    assert np.isnan(got[0]).any() == (labels[h - 1, w - 1] != 255)                      # the NaN reaches its region's sum, and only that one


# (9 x 1 at 4 bins and one region is held by tests/test_spectral_compare_gpu.py test_hand_made_arrays[9-1-4-1])
@pytest.mark.parametrize("w,h,bins,regions", [(w, h, b, r) for w, h in SIZES for b, r in SHAPES if (w, h, b, r) != (9, 1, 4, 1)])
def test_compare_arrays_around_the_unroll(w, h, bins, regions):
    SA, QA, NA, labels = synthetic(w, h, bins, regions, 1)
    SB, QB, NB, _ = synthetic(w, h, bins, regions, 2)
    (sums, diff, var), want = pure().compare_arrays(SA, QA, NA, SB, QB, NB, labels, regions, t2=2.0), cref.compare(SA, QA, NA, SB, QB, NB, labels, regions, 2.0)
    for name, g, x in zip(("DD", "VV", "X2", "CC", "NC", "EX"), sums, want):
        assert same(g, x), name
    wd, wv = cref.maps(SA, QA, NA, SB, QB, NB)
    assert same(diff, wd) and same(var, wv)
    assert w * h < 40 or (want[3].any() and want[4].any() and want[5].any())             # comparable, not comparable and exceeding cells all occur


@pytest.mark.parametrize("bins", [4, 64])
@pytest.mark.parametrize("owner", [(0, 1, 0), (1, 2, 1)])                                # (tile_first, tile_stride, tile_skew)
@pytest.mark.parametrize("w,h", [(13, 11), (7, 20)])
def test_export_import_export_returns_the_bits(w, h, bins, owner):
    def context():
        r = Renderer(Options(scene_name="cornell-srgb", res=(w, h), seed=ck.SEED, texture=ck.TEX, spp_per_launch=4, tile_first=owner[0], tile_stride=owner[1], tile_skew=owner[2]))
        r.set_spectral_bins(bins)
        r.set_spectral_moments(True)
        return r
    r = context()
    ck.start(r, 3)
    info, sums, _ = r.export_sums()
    sinfo, S, N = r.export_spectral()
    _, Q = r.export_moments()
    assert S.any() and Q.any() and (N.sum(axis=2) == 3).any()
    fresh = context()
    fresh.import_sums(info, sums)
    fresh.import_spectral(sinfo, S, N)
    fresh.import_moments(sinfo, Q)
    assert ck.same(fresh.export_spectral()[1:] + (fresh.export_moments()[1],), (S, N, Q))
    assert ck.same((fresh.export_sums()[1],), (sums,))
