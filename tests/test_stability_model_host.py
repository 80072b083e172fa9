"""tests/stability_model.py against brute force: keep masks from a scalar loop over the hash, half-samples
from the statement itself on the 0/1 vector, the complementarity of 2j / 2j + 1, the ranks against ``np.sort``, and what
two complementary halves' scores add up to.  No device, no ``ffsubsync_amd.stability``."""
import numpy as np
import pytest

import exact_reference as er
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm


def brute_force(v01, seed, s, block_runs):
    """The half-sample of a 0/1 vector by the statement itself: number the runs, hash each run's block, silence the runs
    that are not kept."""
    v01 = np.asarray(v01, dtype=np.uint8)
    pos = sm.boundaries(v01)
    out = np.zeros_like(v01)
    for j in range(pos.size // 2):
        if ((sm.key(seed, s >> 1, j // block_runs) >> 31) ^ (s & 1)) == 1:
            out[pos[2 * j]:pos[2 * j + 1]] = 1
    return out


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF, 123456789])
def test_keep_masks_equal_a_scalar_loop_over_the_key(seed):
    for s in (0, 1, 2, 3, 64, 65, 4094, 4095):
        for nb in (0, 1, 2, 63, 64, 65, 300):
            want = [((sm.key(seed, s >> 1, b) >> 31) ^ (s & 1)) == 1 for b in range(nb)]
            assert stm.keep_mask(seed, s, nb).tolist() == want
    # about half of many blocks is kept, and two pairs differ
    keep = stm.keep_mask(seed, 0, 4000)
    assert 1800 < int(keep.sum()) < 2200 and not np.array_equal(keep, stm.keep_mask(seed, 2, 4000))


@pytest.mark.parametrize("runs,block_runs", [(0, 1), (1, 1), (1, 4), (2, 1), (3, 2), (64, 1), (65, 7), (257, 7), (257, 64),
                                             (300, 1), (300, 400)])
def test_half_samples_equal_brute_force_and_pairs_are_complementary(runs, block_runs):
    rng = np.random.RandomState(runs * 31 + block_runs)
    if runs:
        pos, length = cases.random_list(rng, runs - 1, kind=runs % 4)
    else:
        pos, length = np.zeros(0, np.int64), 23
    v = sm.expand(pos, length)
    assert stm.n_blocks(pos.size, block_runs) == -(-runs // block_runs)
    for seed in (0, 0xFFFFFFFF, 77):
        for s in (0, 1, 2, 3, 8, 9):
            got = stm.subsample(pos, seed, s, block_runs)
            assert got.dtype == np.int64 and got.size % 2 == 0
            assert np.array_equal(sm.expand(got, length), brute_force(v, seed, s, block_runs)), (seed, s)
            assert set(got.tolist()) <= set(pos.tolist())  # positions untouched
        for j in (0, 1, 4):
            a = sm.expand(stm.subsample(pos, seed, 2 * j, block_runs), length).astype(np.int64)
            b = sm.expand(stm.subsample(pos, seed, 2 * j + 1, block_runs), length).astype(np.int64)
            assert np.array_equal(a + b, v)  # disjoint, and together the input
            na, nb = stm.subsample(pos, seed, 2 * j, block_runs).size, stm.subsample(pos, seed, 2 * j + 1, block_runs).size
            assert na + nb == pos.size


def test_a_list_of_one_block_is_kept_whole_by_one_member_of_every_pair():
    rng = np.random.RandomState(3)
    pos, length = cases.random_list(rng, 9)
    for j in range(8):
        sizes = sorted(stm.subsample(pos, 5, 2 * j + i, 10).size for i in (0, 1))
        assert sizes == [0, pos.size]
    assert {stm.subsample(pos, 5, 2 * j, 10).size for j in range(40)} == {0, pos.size}  # either member, over the pairs


def test_encoded_blocks_carry_exact_ones_before():
    rng = np.random.RandomState(4)
    pos, length = cases.random_list(rng, 99, kind=1)
    got = stm.subsample(pos, 11, 3, 2)
    words = stm.encode(got, length, got.size + 3)
    bits = sm.expand(got, length)
    assert tuple(words[:4]) == (got.size, int(bits.sum()), length, got.size + 3)
    assert np.array_equal(words[4:4 + 2 * got.size:2], got)
    assert np.array_equal(words[5:5 + 2 * got.size:2], np.concatenate([[0], np.cumsum(bits)])[got])
    assert tuple(words[-2:]) == (stm.INT32_MAX, int(bits.sum()))
    assert np.array_equal(stm.encode(np.zeros(0, np.int64), 50, 4), stm.empty_block(50, 4))
    assert [stm.status(*a) for a in ((4, 5, 4), (5, 6, 6), (4, 4, 4), (-2, 5, 4), (6, 7, 4), (7, 7, 4))] == [
        0, stm.BAD_ODD, stm.BAD_TRUNCATED, stm.BAD_TRUNCATED, stm.BAD_BOUND, stm.BAD_ODD | stm.BAD_TRUNCATED | stm.BAD_BOUND]


@pytest.mark.parametrize("k", [1, 2, 3, 19, 20, 21, 40, 41, 63, 64, 65, 257])
def test_ranks_equal_np_sort(k):
    rng = np.random.RandomState(k)
    off = rng.randint(-6000, 6001, k + 1).astype(np.int64) + (np.int64(1) << 40) * rng.randint(-1, 2, k + 1)
    sc = rng.rand(k + 1) * 100
    fl = np.zeros(k + 1, np.int32)
    bad = rng.rand(k + 1) < 0.2
    bad[0] = False
    fl[bad] = stm.FLAG_EMPTY_WINDOW
    rec = stm.offset_stats(sc, off, fl, 100)
    srt = np.sort(off[1:][~bad[1:]])
    c = srt.size
    assert rec["n_sub"] == c
    if c == 0:
        assert rec["flags"] & stm.EMPTY and rec["off_median"] == 0
        return
    assert rec["off_min"] == srt[0] and rec["off_max"] == srt[-1]
    assert rec["off_median"] == srt[(c - 1) // 2] and rec["off_lo"] == srt[(c - 1) // 20] and rec["off_hi"] == srt[c - 1 - (c - 1) // 20]
    assert rec["off_lo"] <= rec["off_median"] <= rec["off_hi"]
    assert rec["max_dev"] == int(np.abs(srt - off[0]).max()) and rec["n_within"] == int((np.abs(srt - off[0]) <= 100).sum())
    # at most (c - 1) // 20 usable offsets lie on either side of the interval
    assert int((srt < rec["off_lo"]).sum()) <= (c - 1) // 20 and int((srt > rec["off_hi"]).sum()) <= (c - 1) // 20


def test_records_by_hand():
    f = lambda **kw: {**dict.fromkeys(stm.FIELDS, 0), "pair_score_min": 0.0, **kw}
    # four subsamples, one unusable (NaN): its pair does not count
    rec = stm.offset_stats([10.0, 6.0, 5.0, np.nan, 7.0], [100, 101, 98, 5000, 100], [0, 0, 0, 0, 0], 1)
    assert rec == f(real_score=10.0, real_offset=100, off_min=98, off_max=101, off_median=100, off_lo=98, off_hi=101, max_dev=2,
                    max_pair_gap=3, pair_score_min=11.0, n_sub=3, n_within=2, n_pairs=1, n_pairs_within=0, tol=1, flags=0)
    # K = 1: no pair; an AMBIGUOUS record is carried
    rec = stm.offset_stats([10.0, 6.0], [-(1 << 40), (1 << 40)], [0, stm.FLAG_AMBIGUOUS], 0)
    assert rec["flags"] == stm.NO_PAIRS | stm.AMBIGUOUS and rec["max_dev"] == 1 << 41 and rec["n_within"] == 0
    assert rec["off_lo"] == rec["off_hi"] == rec["off_median"] == 1 << 40
    # the real record unusable: EMPTY, the order statistics 0, the pairs still reported
    rec = stm.offset_stats([-np.inf, 6.0, 5.0], [7, 50, 60], [stm.FLAG_EMPTY_WINDOW, 0, 0], 10)
    assert rec["flags"] == stm.EMPTY and rec["n_sub"] == 2 and rec["off_max"] == 0 and rec["max_dev"] == 0 and rec["n_within"] == 0
    assert (rec["n_pairs"], rec["max_pair_gap"], rec["n_pairs_within"], rec["pair_score_min"]) == (1, 10, 1, 11.0)
    # nothing usable
    rec = stm.offset_stats([3.0, np.inf, 1.0], [7, 50, 60], [0, 0, stm.FLAG_EMPTY_WINDOW], 10)
    assert rec["flags"] == stm.EMPTY | stm.NO_PAIRS and rec["n_sub"] == 0 and stm.share_within(rec) == 0.0
    # ties, and the odd last subsample without a partner
    rec = stm.offset_stats([1.0] * 4, [5, 5, 5, 5], [0] * 4, 0)
    assert (rec["n_sub"], rec["n_within"], rec["n_pairs"], rec["max_pair_gap"], rec["max_dev"]) == (3, 3, 1, 0, 0)


def test_two_complementary_halves_add_up_to_the_real_score_and_the_silent_one():
    """With the levels (0, 1) on both sides every sample is mapped to -1 / +1 (``exact_reference.pm1``), so the score is
    sum (2s - 1)(2r - 1) over the overlap.  For complementary halves A + B = s:
        score_A(d) + score_B(d) = score_real(d) + score_silent(d)    at every lag d,
    score_silent the score of the all-zero subtitle, sum (1 - 2r): NOT score_real alone (the 0.0 level of a subtitle is
    not a zero weight).  With subtitle levels (0.5, 1) silence weighs nothing and score_real = score_A + score_B holds as
    it stands; then max_A + max_B >= max (A + B), so pair_score_min >= real_score.  With (0, 1) the same argument gives
    pair_score_min >= real_score + the smallest silent score of the window: >= real_score whenever the reference is less
    than half speech over every overlap."""
    rng = np.random.RandomState(5)
    ref = (rng.rand(400) < 0.35).astype(np.uint8)
    sub = np.repeat(rng.rand(60) < 0.5, 5).astype(np.uint8)[:290]
    pos = sm.boundaries(sub)
    silent = np.zeros_like(sub)
    w = 80
    lags = range(-w + 1, w + 1)
    for block_runs in (1, 3):
        a = sm.expand(stm.subsample(pos, 9, 4, block_runs), sub.size)
        b = sm.expand(stm.subsample(pos, 9, 5, block_runs), sub.size)
        assert np.array_equal(a + b, sub) and a.any() and b.any()
        for d in lags:
            at = lambda v, lv: er.score_at(ref, v, (0.0, 1.0), lv, d)
            assert at(a, (0.0, 1.0)) + at(b, (0.0, 1.0)) == at(sub, (0.0, 1.0)) + at(silent, (0.0, 1.0)), d
            assert at(a, (0.5, 1.0)) + at(b, (0.5, 1.0)) == at(sub, (0.5, 1.0)), d
    for levels in ((0.0, 1.0), (0.5, 1.0)):
        sc, off, fl = stm.half_records(ref, sub, (0.0, 1.0), levels, w, 9, 16, 1)
        rec = stm.offset_stats(sc, off, fl, 0)
        slack = 0.0 if levels[0] == 0.5 else min(er.score_at(ref, silent, (0.0, 1.0), levels, d) for d in lags)
        assert rec["n_pairs"] == 8 and rec["pair_score_min"] >= rec["real_score"] + slack
        assert rec["pair_score_min"] == min(sc[1 + 2 * j] + sc[2 + 2 * j] for j in range(8))


def test_the_model_separates_matched_from_wrong_on_the_shared_problems():
    """What tests/test_gpu_stability.py relies on: on seeds 0-5 at 10 min every matched file keeps all its half-samples
    within TOL of the full solve and every wrong file less than half of them."""
    import stability_cases as sc

    for i, kind in enumerate(cases.sync_kinds()):
        model = sc.model_sync(i)
        assert model["record"]["n_sub"] == cases.K and model["record"]["flags"] == 0
        if kind == "matched":
            assert model["share_within"] == 1.0 and model["stable"] and model["reasons"] == []
            assert model["record"]["max_dev"] <= 3 and model["interval_samples"][1] - model["interval_samples"][0] <= 4
        else:
            assert model["share_within"] <= 4 / 16 and not model["stable"] and model["reasons"][0].startswith("%d of 64 half-samples within"
                                                                                                                % model["record"]["n_within"])
            assert model["record"]["max_dev"] > 1000
