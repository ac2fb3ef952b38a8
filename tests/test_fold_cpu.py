"""The oracle's fold as a callable (orc_fold_levels) tied to the oracle's own recursion, and what tests/fold_cases.py reaches -- no GPU.
tests/test_fold_gpu.py holds the path kernel's fold (ssx_debug_fold) to orc_fold_levels on the same rows."""
import numpy as np
import pytest

import fold_cases as fc
import oracle_lib as ol

LAMBDA_MIN, LAMBDA_STEP = 400.0, 75.0   # any range does for what the cases REACH; the GPU tests take their context's


@pytest.fixture(scope="module")
def cornell():
    return ol.Oracle("cornell-srgb", texture="test-img.png")


@pytest.mark.parametrize("key", list(fc.REPLAY_CONFIGS))
def test_replay_equals_render_sample_bit_for_bit(key):
    """orc_fold_levels on the levels the recorder wrote while orc_render_sample ran = what orc_render_sample returned: flux and XYZA, every sample"""
    orc, flags, cases = fc.replay_cases(key)
    for c in cases:
        _, want_flux, want_xyza, _, _ = c.replay
        flux, xyza = fc.oracle_fold(orc, c.rows, flat_field=True)
        assert np.array_equal(flux, want_flux), c.name
        assert np.array_equal(xyza, want_xyza), c.name


def test_recorder_changes_no_result_and_is_off_by_default():
    orc, flags, cases = fc.replay_cases("cornell-srgb")
    c = cases[0]
    xyza, _, _ = orc.samples(fc.W, fc.H, c.spp, seed=fc.SEED, rect=(fc.TILES[0][0], fc.TILES[0][1], fc.TILES[0][0] + 8, fc.TILES[0][1] + 8))
    assert np.array_equal(fc.f2u(xyza.reshape(-1, 4)), c.replay[2])


def test_replay_without_flat_field_correction():
    """the flat-field multiply sits inside orc_fold_levels: a render built without the correction replays too"""
    orc, _, cases = fc.replay_cases("cornell-srgb")
    c = cases[1]
    i0, j0 = fc.TILES[1]
    xyza, _, _ = orc.samples(fc.W, fc.H, c.spp, seed=fc.SEED, rect=(i0, j0, i0 + 8, j0 + 8), flat_field=False)
    _, got = fc.oracle_fold(orc, c.rows, flat_field=False)
    assert np.array_equal(got, fc.f2u(xyza.reshape(-1, 4)))
    assert not np.array_equal(got, c.replay[2])


@pytest.mark.parametrize("key", list(fc.REPLAY_CONFIGS))
def test_pixel_sums_restated_in_binary64_match_the_oracles_pixels(key):
    """+= float32(x * 0.001f), widened, in ascending k: the oracle's binary64 accumulators bit for bit (orc_pixel_sums) -- and then, with orc_render's
    own division, its float32 pixel"""
    orc, flags, cases = fc.replay_cases(key)
    for c in cases:
        sums = fc.pixel_sums(c.replay[2], c.spp, rgb=False)
        assert np.array_equal(sums.view(np.uint64), c.replay[4].view(np.uint64)), c.name
        mean = (sums * (1000.0 / c.spp)).astype(np.float32)
        assert np.array_equal(fc.f2u(mean), fc.f2u(c.replay[3])), c.name


def test_pixel_sums_in_rgb_mode_add_the_sample_as_it_is():
    orc = ol.Oracle("cornell-srgb", texture="test-img.png", rgb=True)
    spp = 3
    image = orc.render(8, 8, spp, seed=fc.SEED, nthreads=1)
    xyza, _, _ = orc.samples(8, 8, spp, seed=fc.SEED)
    sums = fc.pixel_sums(fc.f2u(xyza.reshape(-1, 4)), spp, rgb=True)
    own = np.zeros((64, 4), dtype=np.float64)
    for p in range(64):
        fc.bind(orc.lib).orc_pixel_sums(orc.color, orc.scene, fc.SEED, p & 7, p >> 3, 8, 8, spp, 0, own[p].ctypes.data)
    assert np.array_equal(sums.view(np.uint64), own.view(np.uint64))
    assert np.array_equal(fc.f2u((sums / spp).astype(np.float32)), fc.f2u(image.reshape(64, 4)))


def all_cases():
    cases = fc.synthetic_cases(LAMBDA_MIN, LAMBDA_STEP)
    for key in fc.REPLAY_CONFIGS:
        cases += fc.replay_cases(key)[2]
    return cases


def test_cases_reach_what_they_claim():
    syn = fc.synthetic_cases(LAMBDA_MIN, LAMBDA_STEP)
    total = fc.counts(np.concatenate([c.rows for c in syn]))
    assert total["depth9"] >= 64 + 16 and min(total["depth_hist"]) >= 16          # every n in 0..9, all nine continued levels
    assert total["emission_below_last"] >= 500 and total["both_terms"] >= 500
    assert total["occluded"] >= 200 and total["inf_pdf"] >= 9 and total["misses"] == 128
    lad = fc.counts(fc.synthetic_ladders(LAMBDA_MIN, LAMBDA_STEP))
    assert lad["samples"] == 160 and lad["depth_hist"] == [16] * 10
    # partial and full last cohorts, both among the synthetic and among the replayed cases
    for group in (syn, [c for key in fc.REPLAY_CONFIGS for c in fc.replay_cases(key)[2]]):
        assert sum(c.partial_cohort for c in group) >= 2 and sum(not c.partial_cohort for c in group) >= 2
        assert {c.spp for c in group} >= {1, 2, 3, 4, 5}
        assert all(c.rows.shape == (64 * c.spp, fc.ROW) and 1 <= c.spp <= 5 for c in group)
    assert 2000 <= sum(len(c.rows) for c in all_cases()) <= 6000
    # the replayed tiles: what the scenes give without being asked
    mirror = fc.counts(np.concatenate([c.rows for c in fc.replay_cases("mirror-no-els")[2]]))
    assert mirror["emission_below_last"] > 0 and mirror["depth9"] > 0
    els = fc.counts(np.concatenate([c.rows for c in fc.replay_cases("cornell-srgb")[2]]))
    assert els["occluded"] > 0
    # with explicit light sampling only the camera ray's level emits (:169-172); without it the levels below do too
    deeper = lambda key: sum(int(((fc.level(c.rows, l)[:, fc.L_FLAGS] & fc.EMISSION) != 0)[c.rows[:, fc.N] >= l].sum()) for c in fc.replay_cases(key)[2] for l in range(1, 10))
    assert deeper("cornell-srgb") == 0 and deeper("mirror-no-els") > 0
    # the edge samples: every value in every position, NaN in one hero lane only
    edge, names = fc.edge_samples(LAMBDA_MIN, LAMBDA_STEP)
    assert len(set(names)) == len(names) == len(edge)
    assert {n.split("/", 1)[1] for n in names if n[0] == "n" and n[1].isdigit()} == {"%s/%s" % (p, v) for p in fc.EDGE_POSITIONS for v, _ in fc.EDGE_VALUES}
    for r, n in zip(edge, names):
        if n.endswith(fc.NAN_LANE) and ("/n_dot_l/" not in n and "/pdf/" not in n):
            assert int(np.isnan(fc.u2f(r)).sum()) == 1, n
    assert sum(n.startswith("minus-zero/") for n in names) == 6


def test_sum_order_cases_tell_ascending_k_from_any_other_order(cornell):
    """binary64 sums of ordinary samples are exact in any order; the sum-order cases are the ones whose pixels' sums change when k runs backwards"""
    syn = {c.name: c for c in fc.synthetic_cases(LAMBDA_MIN, LAMBDA_STEP)}
    for rgb, orc in ((False, cornell), (True, ol.Oracle("cornell-srgb", texture="test-img.png", rgb=True))):
        for name in ("sum-order-spp3", "sum-order-spp5"):
            c = syn[name]
            _, xyza = fc.oracle_fold(orc, c.rows)
            back = xyza.reshape(64, c.spp, 4)[:, ::-1].reshape(-1, 4)
            up, down = fc.pixel_sums(xyza, c.spp, rgb), fc.pixel_sums(back, c.spp, rgb)
            assert np.isfinite(up).all() and int((up[:, :3] != down[:, :3]).any(axis=1).sum()) == 64, (name, rgb)
        c = syn["ladders-spp3"]
        _, xyza = fc.oracle_fold(orc, c.rows)
        assert np.array_equal(fc.pixel_sums(xyza, 3, rgb), fc.pixel_sums(xyza.reshape(64, 3, 4)[:, ::-1].reshape(-1, 4), 3, rgb))


def test_the_oracle_answers_every_case(cornell):
    """scalar C evaluation of the fold is total: no row is left without an answer, whatever it holds (0xDEADBEEF = not written)"""
    for flat_field in (True, False):
        for c in all_cases():
            flux, xyza = fc.oracle_fold(cornell, c.rows, flat_field=flat_field)
            assert not (flux == 0xDEADBEEF).any() and not (xyza == 0xDEADBEEF).any(), c.name
            alpha = fc.u2f(xyza[:, 3])
            assert np.array_equal(alpha, (c.rows[:, fc.HIT] != 0).astype(np.float32)), c.name


def test_minus_zero_term_over_minus_zero_indirect_term_is_plus_zero(cornell):
    """The statement of the domain: L() starts every level from a literal 0 (renderer.cpp:149), so a level whose only term is -0 over a -0 indirect
    term comes out +0 -- 0 + -0 = +0 --, and so does a last level whose emission and next-event term are both -0."""
    edge, names = fc.edge_samples(LAMBDA_MIN, LAMBDA_STEP)
    rows = np.stack([r for r, n in zip(edge, names) if n.startswith("minus-zero/")])
    flux, _ = fc.oracle_fold(cornell, rows)
    assert (flux == 0).all()   # +0.0 in all four hero lanes
