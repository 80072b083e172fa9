"""Drift-tolerant alignment without a GPU: the numpy model (tests/drift_model.py) against split_model at max_step = 0,
its priority order and window edges on hand-built tables, its total against a brute-force maximum over all paths, the
host side of ffsubsync_amd.drift_align (argument checks, Segment construction, cue mapping), and the calibration claims
behind DEFAULT_MAX_STEP / DEFAULT_STEP_COST on workloads/drift.py."""
import numpy as np
import pytest

import drift_model as dm
import split_model as sm
from ffsubsync_amd import drift_align as da
from ffsubsync_amd import split_align as sa

J = dm.JUMP
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_max_step_zero_is_the_split_dp_bit_for_bit():
    rng = np.random.RandomState(5)
    for it in range(300):
        n_blocks, n_lags = int(rng.randint(1, 9)), int(rng.randint(1, 14))
        m = rng.randn(n_blocks, n_lags) * 1000.0 if it % 2 else rng.randint(-3, 4, (n_blocks, n_lags)).astype(np.float64)
        for p in (0.0, 3.0, 8192.0, INF):
            o, total = sm.dp(m, p)
            o2, jump, total2 = dm.dp(m, p, 0, 7.5)
            assert np.array_equal(o, o2) and _bits([total])[0] == _bits([total2])[0]
            assert jump[0] == 0 and np.array_equal(jump[1:], (o[1:] != o[:-1]).astype(np.uint8))


def _codes(row0, p, s, q):
    """The codes of block 1 over a previous row ``row0`` (block 1's own scores do not enter them)."""
    m = np.array([row0, np.zeros(len(row0))], dtype=np.float64)
    return dm.dp_tables(m, p, s, q)[1][1].tolist()


def test_priority_order_on_exact_ties():
    # everything ties: STAY wins over every move and over JUMP (P = 0: T equals the row maximum)
    assert _codes([1, 1, 1, 1, 1], 0.0, 2, 0.0) == [0, 0, 0, 0, 0]
    # +1 before -1
    assert _codes([2, 0, 2], INF, 1, 0.0) == [0, 1, 0]
    # +2 before -2, and a +-1 that is no better changes nothing
    assert _codes([3, 0, 0, 0, 3], INF, 2, 0.0)[2] == 2
    # smaller moves first: +1 at 2 - 1 ties -1 at 2 - 1 and +-2 at 3 - 2
    assert _codes([3, 2, 0, 2, 3], INF, 2, 1.0)[2] == 1
    # -1 when it is strictly better than +1, +2 when strictly better than both
    assert _codes([0, 0, 5], INF, 1, 1.0)[1] == -1
    assert _codes([9, 0, 0, 1], INF, 2, 1.0)[2] == 2
    # a move that ties JUMP keeps the move; JUMP when strictly better
    assert _codes([3, 0, 0], 1.0, 2, 1.0) == [0, 1, J]  # j = 1: +1 gives 2 = T; j = 2: +2 gives 1 < T = 2
    # STAY that ties JUMP stays ("ties stay", as split_model)
    assert _codes([3, 0], 3.0, 0, 0.0) == [0, 0]
    assert _codes([3, 0], 2.0, 0, 0.0) == [0, J]
    # step_cost = 0: the largest reachable neighbour, the nearest of equal ones
    assert _codes([0, 1, 2, 3], INF, 7, 0.0) == [-3, -2, -1, 0]
    assert _codes([0, 2, 2, 2], INF, 7, 0.0) == [-1, 0, 0, 0]
    assert _codes([2, 2, 0, 2, 2], INF, 7, 0.0)[2] == 1


def test_window_edges():
    # j - e outside [0, L) is no option: at j = 0 only negative e, at j = L-1 only positive
    assert _codes([0, 0, 9], INF, 7, 0.0) == [-2, -1, 0]
    assert _codes([9, 0, 0], INF, 7, 0.0) == [0, 1, 2]
    assert _codes([0, 9, 0], INF, 7, 0.0) == [-1, 0, 1]
    # max_step wider than the table, and one-lag tables
    assert _codes([4], 0.0, 7, 0.0) == [0]
    rng = np.random.RandomState(11)
    for _ in range(200):
        n_blocks, n_lags = int(rng.randint(2, 6)), int(rng.randint(1, 7))
        m = rng.randint(-4, 5, (n_blocks, n_lags)).astype(np.float64)
        s = int(rng.randint(0, 8))
        _, code, _ = dm.dp_tables(m, float(rng.choice([0.0, 2.0, INF])), s, float(rng.choice([0.0, 1.0, 3.0])))
        assert not code[0].any()
        for j in range(n_lags):
            for c in code[1:, j]:
                assert c == J or (abs(c) <= s and 0 <= j - c < n_lags)


def test_same_offsets_different_flags():
    """A jump and a step can produce the same offset difference: the flag is an output."""
    m = np.array([[3, 0, 0], [0, 0, 5]], dtype=np.float64)
    o, jump, total = dm.dp(m, 1.0, 2, 1.0)  # T = 2 beats the +2 step (3 - 2)
    assert o.tolist() == [0, 2] and jump.tolist() == [0, 1] and total == 7.0
    o, jump, total = dm.dp(m, 2.0, 2, 1.0)  # T = 1 ties the +2 step: the step stays
    assert o.tolist() == [0, 2] and jump.tolist() == [0, 0] and total == 6.0


def test_total_is_the_maximum_over_all_paths():
    rng = np.random.RandomState(3)
    for _ in range(120):
        n_blocks, n_lags = int(rng.randint(1, 6)), int(rng.randint(1, 7))
        m = rng.randint(-5, 6, (n_blocks, n_lags)).astype(np.float64)  # small integers: every sum is exact
        for p in (0.0, 2.0, 7.0, INF):
            for s, q in ((0, 1.0), (1, 0.0), (1, 1.0), (2, 0.5), (3, 2.0), (7, 1.0)):
                o, jump, total = dm.dp(m, p, s, q)
                assert total == dm.brute_force_total(m, p, s, q), (m, p, s, q)
                # and the path the backtrack returns costs what the total says
                cost = sum(p if jump[b] else q * abs(int(o[b]) - int(o[b - 1])) for b in range(1, n_blocks))
                assert all(jump[b] or abs(int(o[b]) - int(o[b - 1])) <= s for b in range(1, n_blocks))
                assert total == sum(m[b, o[b]] for b in range(n_blocks)) - cost


def test_argument_validation():
    for bad in (-1, 8, 1.5, "x", None, float("nan")):
        with pytest.raises(ValueError):
            da.validate_drift_args(bad, 1.0)
    for bad in (-1.0, float("nan"), INF, -INF):
        with pytest.raises(ValueError):
            da.validate_drift_args(2, bad)
    for s in range(8):
        da.validate_drift_args(s, 0.0)
    da.validate_drift_args(2.0, 1e300)
    # before any native call or look at the batch
    with pytest.raises(ValueError):
        da.drift_align_batch(None, 100, max_step=9)
    with pytest.raises(ValueError):
        da.drift_align_batch(None, 100, step_cost=-2.0)
    with pytest.raises(ValueError):
        da.drift_align_batch(None, 100, block_samples=100)
    with pytest.raises(ValueError):
        da.drift_sync([], step_cost=INF)
    assert 0 <= da.DEFAULT_MAX_STEP <= 7 and da.DEFAULT_STEP_COST >= 0
    with pytest.raises(ValueError):
        dm.dp(np.zeros((2, 2)), 1.0, 8, 1.0)


def test_segments_from_blocks():
    offs = np.array([10, 10, 11, 12, 40, 40, 39, 39, 39, 7], dtype=np.int32)
    jump = np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 1], dtype=np.uint8)
    scores = np.arange(10, dtype=np.float64) + 0.25
    segs = da.segments_from_blocks(offs, scores, jump, 256, 10 * 256 - 56)
    assert [(s.first_block, s.end_block, s.start_sample, s.end_sample, s.first_offset, s.last_offset) for s in segs] == \
        [(0, 4, 0, 1024, 10, 12), (4, 9, 1024, 2304, 40, 39), (9, 10, 2304, 2504, 7, 7)]
    assert [s.score for s in segs] == [0.25 + 1.25 + 2.25 + 3.25, 4.25 + 5.25 + 6.25 + 7.25 + 8.25, 9.25]
    assert [s.drift for s in segs] == [2 / (3 * 256.0), -1 / (4 * 256.0), 0.0]
    one = da.segments_from_blocks(offs[:1], scores[:1], jump[:1], 256, 100)
    assert [(s.first_block, s.end_block, s.end_sample, s.drift) for s in one] == [(0, 1, 100, 0.0)]
    # a change of offset without the flag is a step, not a boundary
    assert len(da.segments_from_blocks([5, 9], [1.0, 1.0], [0, 0], 256, 512)) == 1


def test_map_cues_drift_is_map_cues_over_the_block_runs():
    rng = np.random.RandomState(2)
    n_blocks, k = 40, 256
    offs = np.cumsum(rng.randint(-1, 2, n_blocks)).astype(np.int32) + 100
    jump = np.zeros(n_blocks, np.uint8)
    offs[25:] += 3000
    jump[25] = 1
    scores = rng.rand(n_blocks)
    sub_len = n_blocks * k - 17
    res = da.DriftResult(da.segments_from_blocks(offs, scores, jump, k, sub_len), 0.0, offs, scores, jump)
    start = np.sort(rng.randint(0, 110_000_000, 200)).astype(np.int64)  # some cues past the last block
    end = start + rng.randint(400_000, 3_000_000, 200)
    for ratio in (1.0, 24.0 / 25.0):
        got = da.map_cues_drift(start, end, ratio, res, k)
        want = sa.map_cues(start, end, ratio, sa.pieces_from_blocks(offs, scores, k, sub_len))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        sample = np.array([int(round(sa._scaled_us(u, ratio) / 1e6 * 100)) for u in start])
        block = np.minimum(sample // k, n_blocks - 1)
        assert np.array_equal(got[2], (block >= 25).astype(np.int64))
        assert np.array_equal(got[0] - np.array([sa._scaled_us(u, ratio) for u in start]), offs[block].astype(np.int64) * 10000)


def test_workload_truth_and_clean_pairs():
    from workloads import drift, synth

    spec = synth.make_pair_spec(4, 1800.0, max_true_offset_s=45.0)
    pr = drift.make_problem(4, 1800.0, clean=True)
    assert pr.eps == 0.0 and pr.wobble_s == 0.0 and pr.ratio_index == spec.true_ratio_index
    assert np.array_equal(pr.ref, synth.pair_arrays(spec)[0])
    assert np.allclose(pr.true_offset(np.arange(0, pr.sub.size, 5000)), spec.true_offset_samples, atol=1e-6)
    dr = drift.make_problem(4, 1800.0, eps=4e-4, wobble_s=0.0)
    i = np.array([0.0, 100000.0])
    assert np.allclose(np.diff(dr.true_offset(i)), 4e-4 * 100000.0)
    wb = drift.make_problem(4, 1800.0, eps=0.0, wobble_s=1.5)
    t = wb.true_offset(np.arange(0, wb.sub.size, 100)) - wb.offset_s * 100
    assert 140.0 < t.max() <= 150.0 and -150.0 <= t.min() < -140.0
    for seed in range(8):
        p = drift.make_problem(seed, 600.0)
        assert drift.MIN_EPS <= abs(p.eps) <= drift.MAX_EPS and 0.0 <= p.wobble_s <= drift.MAX_WOBBLE_S
        assert p.start_us.size == p.end_us.size == p.true_start_us.size and np.all(p.end_us > p.start_us)
    br = drift.make_problem(4, 1800.0, insert_break=True)
    assert br.ref.size == pr.ref.size + int(round(br.break_len_s * 100))
    late = br.true_offset(br.sub.size - 1.0) - drift.make_problem(4, 1800.0).true_offset(br.sub.size - 1.0)
    assert abs(late - br.break_len_s * 100) < 1e-6


def test_calibration_claims_at_the_committed_defaults():
    """Two-hour problems of workloads/drift.py, K = 1024, +-60 s, P = 8192, on the model (the device equals it bit for
    bit): every one of 16 clean pairs returns split_model's block offsets exactly, and on every one of 16 drifting pairs
    the mean block-offset error is at most half of split_model's."""
    from workloads import drift

    k, w, p = 1024, 6000, sa.DEFAULT_SPLIT_PENALTY
    rows = []
    for seed in range(16):
        for clean in (True, False):
            pr = drift.make_problem(seed, clean=clean)
            m = sm.block_scores(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), k, w)
            o, _ = sm.dp(m, p)
            split_off = o - (w - 1)
            off, _, jump, _ = dm.solve(None, None, None, None, k, w, p, da.DEFAULT_MAX_STEP, da.DEFAULT_STEP_COST, m=m)
            if clean:
                assert np.array_equal(off, split_off), (seed, int((off != split_off).sum()))
            else:
                rows.append((seed, drift.mean_block_error(pr, split_off, k), drift.mean_block_error(pr, off, k)))
    print("seed, split error, drift error (samples):", [(s, round(a, 2), round(b, 2)) for s, a, b in rows])
    assert all(b <= 0.5 * a for _, a, b in rows), rows
