"""Host-side tests of the lag-range drift aligner (no GPU): the numpy model tests/drift_range_model.py against
drift_model at [-W+1, W], against cut_model at max_step = 0, against an exhaustive maximum on tiny tables; the priority
order on exact ties; argument validation of ffsubsync_amd.drift_range; the workload's truth; one calibration claim."""
import json
import os

import numpy as np
import pytest

import cut_model as cm
import drift_model as dm
import drift_range_model as drm
from ffsubsync_amd import drift_range as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _vectors(seed):
    rng = np.random.RandomState(4400 + seed)
    R, S = int(rng.randint(700, 9000)), int(rng.randint(700, 9000))
    seg = np.maximum(1, rng.geometric(1.0 / 50.0, size=R // 20 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    i = np.arange(S)
    idx = i + int(rng.randint(-S // 2, R // 2)) + i // int(rng.randint(150, 900)) \
        + np.where(i < int(rng.randint(0, S + 1)), 0, int(rng.randint(-1500, 1501)))
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.08
    r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
    s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (-0.5, 1.25)][(seed // 3) % 3]
    return rng, rb, sb, r_lv, s_lv


def test_symmetric_range_is_the_windowed_drift_model_bit_for_bit():
    """[-W+1, W]: all four outputs of drift_model.solve, K in {256, 512, 1024}, max_step 0..7, costs with 0."""
    seen = set()
    for seed in range(24):
        rng, rb, sb, r_lv, s_lv = _vectors(seed)
        k = (256, 512, 1024)[seed % 3]
        w = int(rng.randint(2, 1500))
        s = seed % 8
        q = (0.0, 1.0, 16.0, 128.0)[(seed // 8 + seed) % 4]
        p = (0.0, 0.5, 60.0, 900.0, INF)[seed % 5]
        seen.add((s, q == 0.0))
        got = drm.solve(rb, sb, r_lv, s_lv, k, -w + 1, w, p, s, q)
        want = dm.solve(rb, sb, r_lv, s_lv, k, w, p, s, q)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), seed
        assert np.array_equal(got[2], want[2]) and _bits([got[3]])[0] == _bits([want[3]])[0], seed
    assert {s for s, _ in seen} == set(range(8)) and any(z for _, z in seen)


def _range_of_kind(kind, rng, R, S, seed):
    """The six kinds of lag range of tests/test_gpu_cut.py's small problems."""
    if kind == 0:
        return cm.full_range(R, S)
    if kind == 1:
        return -int(rng.randint(1, S)), int(rng.randint(0, 3 * R))
    if kind == 2:
        lo = int(rng.randint(1, R))
        return lo, lo + int(rng.randint(0, 4000))
    if kind == 3:
        lo = -S - int(rng.randint(0, 2000))
        return lo, lo + 262144 + int(rng.randint(1, 3000))
    if kind == 4:
        w = int(rng.randint(1, 5000))
        return -w + 1, w
    lo = R + int(rng.randint(0, 5000)) if seed % 2 else -S - int(rng.randint(5000, 9000))
    return lo, lo + int(rng.randint(0, 5000))


def test_max_step_zero_is_the_range_split_model_bit_for_bit():
    for seed in range(18):
        rng, rb, sb, r_lv, s_lv = _vectors(seed)
        if seed % 6 == 3:
            sb = sb[:700 + sb.size % 1800]  # few blocks under the 263 k-lag rows
        k = (256, 512, 1024)[(seed // 6) % 3]
        p = (0.0, 0.5, 60.0, 900.0, INF)[seed % 5]
        lo, hi = _range_of_kind(seed % 6, rng, rb.size, sb.size, seed)
        offs, scores, jump, total = drm.solve(rb, sb, r_lv, s_lv, k, lo, hi, p, 0, 3.0)
        w_offs, w_scores, w_total = cm.solve(rb, sb, r_lv, s_lv, k, lo, hi, p)
        assert np.array_equal(offs, w_offs) and np.array_equal(_bits(scores), _bits(w_scores)), seed
        assert _bits([total])[0] == _bits([w_total])[0], seed
        assert jump[0] == 0 and np.array_equal(jump[1:], (np.diff(offs) != 0).astype(np.uint8)), seed


def test_total_is_the_maximum_over_all_paths():
    """Tiny integer tables (exact arithmetic) through dp_rows, L = 1 and L <= max_step among them; the path's own sum
    reproduces the total and respects the moves."""
    rng = np.random.RandomState(5)
    for n_blocks, n_lags in ((4, 1), (4, 2), (3, 5), (4, 4), (5, 3), (3, 7)):
        for trial in range(6):
            m = rng.randint(-6, 7, size=(n_blocks, n_lags)).astype(np.float64)
            for s in (0, 1, 2, 5, 7):
                for p, q in ((3.0, 1.0), (9.0, 2.0), (2.0, 0.0), (INF, 1.0), (0.0, 4.0)):
                    o, jump, total = drm.dp_rows(m, p, s, q)
                    want = dm.brute_force_total(m, p, s, q)
                    assert total == want, (n_blocks, n_lags, trial, s, p, q)
                    o2, jump2, total2 = dm.dp(m, p, s, q)
                    assert np.array_equal(o, o2) and np.array_equal(jump, jump2) and total == total2
                    assert all(jump[b] or abs(int(o[b]) - int(o[b - 1])) <= s for b in range(1, n_blocks))
                    cost = sum(p if jump[b] else q * abs(int(o[b]) - int(o[b - 1])) for b in range(1, n_blocks))
                    assert total == sum(m[b, o[b]] for b in range(n_blocks)) - cost


def _codes(row0, p, s, q):
    """Codes of block 1 over the previous row ``row0`` (block 1 scores all zero), as the device numbers them."""
    dp = drm.RowDP(p, s, q)
    dp.push(np.asarray(row0, dtype=np.float64))
    dp.push(np.zeros(len(row0)))
    packed = dp.codes[0]
    return [(int(packed[j >> 1]) >> (4 * (j & 1))) & 15 for j in range(len(row0))]


def test_priority_order_on_exact_ties():
    # step_cost = 0: every neighbour within max_step ties with STAY on a flat row -> STAY everywhere; T ties too (P = 0)
    assert _codes([5, 5, 5, 5, 5], 0.0, 2, 0.0) == [0, 0, 0, 0, 0]
    # +a before -a: lag 1 sees 9 at both j - 1 and j + 1 -> +1 (code 1); the peaks themselves stay
    assert _codes([9, 0, 9], INF, 1, 0.0) == [0, 1, 0]
    # smaller moves first: lag 2 sees 9 at distance 1 (below) and at distance 2 (above) -> -1 (code 2)
    assert _codes([9, 0, 0, 9], INF, 2, 0.0)[2] == 2 and _codes([9, 0, 0, 9], INF, 2, 0.0)[1] == 1
    # a move that ties with JUMP keeps the move; STAY that ties with T stays (ties do not jump)
    s = 2
    assert _codes([9, 0, 0, 0, 0, 0], 0.0, s, 0.0) == [0, 1, 3, 2 * s + 1, 2 * s + 1, 2 * s + 1]
    # strictly better wins regardless of order: -2 over +1
    assert _codes([0, 1, 0, 7], INF, 2, 0.0)[1] == 4
    # out-of-range neighbours are not options: L = 2 <= max_step
    assert _codes([0, 9], INF, 7, 0.0) == [2, 0]
    # JUMP is code 2 s + 1 at every s
    for s in range(8):
        assert _codes([9] + [0] * 9, 1.0, s, 100.0)[9] == 2 * s + 1


def test_host_validation():
    for bad in (-1, 8, 1.5, "x", None):
        with pytest.raises(ValueError):
            dr.drift_align_range_batch(None, None, max_step=bad)
    for bad in (-1.0, float("nan"), INF):
        with pytest.raises(ValueError):
            dr.drift_align_range_batch(None, None, step_cost=bad)
        with pytest.raises(ValueError):
            dr.cut_drift_sync([], step_cost=bad)
    with pytest.raises(ValueError):
        dr.drift_align_range_batch(None, None, block_samples=100)
    with pytest.raises(ValueError):
        dr.drift_align_range_batch(None, None, split_penalty=-1.0)
    with pytest.raises(ValueError):
        dr.cut_drift_sync([], max_step=9)
    with pytest.raises(ValueError):
        dr.cut_drift_sync([], block_samples=1000)
    for bad in ((5, 4), (0.5, 3), (-2 ** 31, 0), (0, 2 ** 31), 7, (1, 2, 3)):
        with pytest.raises(ValueError):
            dr.cut_drift_sync([], lag_range=bad)
    assert 0 <= dr.DEFAULT_MAX_STEP <= 7 and dr.DEFAULT_RANGE_STEP_COST >= 0
    assert [dr.code_planes(s) for s in range(8)] == [1, 2, 3, 3, 4, 4, 4, 4]
    with pytest.raises(ValueError):
        drm.dp_rows(np.zeros((2, 2)), 1.0, 8, 1.0)


def test_workload_truth():
    from workloads import cut_drift, drift

    k = 1024
    for seed in (0, 1):
        pr = cut_drift.make_problem(seed, fixed=True)
        base = drift.make_problem(seed, cut_drift.DEFAULT_DURATION_S, eps=pr.eps, wobble_s=0.0,
                                  max_true_offset_s=cut_drift.MAX_BASE_OFFSET_S)
        assert abs(pr.eps) == cut_drift.FIXED_EPS and np.array_equal(pr.sub, base.sub)
        n_ins = pr.insert_len_s.size
        assert 2 <= n_ins <= 3 and cut_drift.MIN_TOTAL_S <= pr.insert_len_s.sum() <= cut_drift.MAX_TOTAL_S
        assert pr.ref.size == base.ref.size + int(round(pr.insert_len_s.sum() * 100))
        # outside the inserts the reference is the pair's own
        q = np.rint(pr.insert_ref_s * 100).astype(np.int64)
        assert np.array_equal(pr.ref[:q[0]], base.ref[:q[0]]) and np.array_equal(pr.ref[pr.ref.size - 1000:], base.ref[-1000:])
        # the truth: the pair's own offset plus the inserts passed so far; it passes 131 072 samples
        i = np.arange(0, pr.sub.size, 997, dtype=np.float64)
        passed = np.searchsorted(pr.break_samples(), i, side="right")
        want = base.true_offset(i) + np.concatenate([[0.0], np.cumsum(pr.insert_len_s)])[passed] * 100
        assert np.allclose(pr.true_offset(i), want, atol=1e-6)
        n_blocks = (pr.sub.size + k - 1) // k
        truth = cut_drift.block_truth(pr, n_blocks, k)
        assert np.abs(truth).max() > 131072
        # far from a break, the subtitle's speech meets the reference's speech at the true offset (15 % of the runs are
        # dropped and every edge jitters, so: the share of subtitle speech samples that land on reference speech)
        bb = cut_drift.break_blocks(pr, k)
        assert bb.size == n_ins and np.all(np.diff(bb) > 35) and bb.min() > 35 and bb.max() < n_blocks - 40
        for b0 in (3, int(bb[0]) + 5, n_blocks - 36):
            i = np.flatnonzero(pr.sub[b0 * k:(b0 + 30) * k]) + b0 * k
            d = int(round(truth[b0 + 15]))
            hit = [float(np.mean(pr.ref[i + d + x])) for x in (-300, 0, 300)]
            assert hit[1] > 0.8 and hit[1] > hit[0] + 0.2 and hit[1] > hit[2] + 0.2, (seed, b0, hit)
        # mean_block_error: zero for the truth, leaves out the blocks within `exclude` of a break
        assert cut_drift.mean_block_error(pr, truth, k) == 0.0
        off = truth.copy()
        off[bb[0] - 2:bb[0] + 3] += 70000.0
        assert cut_drift.mean_block_error(pr, off, k, exclude=2) == 0.0
        assert cut_drift.mean_block_error(pr, off, k, exclude=1) > 100.0
        clean = cut_drift.make_problem(seed, clean=True)
        assert clean.eps == 0.0 and clean.pair.wobble_s == 0.0 and np.array_equal(clean.insert_len_s, pr.insert_len_s)
        steps = np.diff(np.rint(cut_drift.block_truth(clean, n_blocks, k)))
        assert (steps != 0).sum() == n_ins


def test_steep_seeds_keep_their_nominal_ratio_nearest():
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import cut_drift

    ratios = list(candidate_ratios())
    seeds = cut_drift.steep_seeds(8)
    assert seeds == [0, 1, 2, 5, 6, 8, 14, 15]
    for seed in range(16):
        pr = cut_drift.make_problem(seed, fixed=True)
        clock = pr.ratio * (1.0 + pr.eps)
        nearest = min(range(len(ratios)), key=lambda i: abs(ratios[i] - clock))
        assert cut_drift.nominal_ratio_is_nearest(pr) == (nearest == pr.ratio_index) == (seed in seeds)
        if seed not in seeds:  # 6e-4 towards a neighbour 1e-3 away leaves 4e-4 to that neighbour
            assert abs(abs(ratios[nearest] / clock - 1.0) - 4e-4) < 2e-5


def test_one_calibration_claim_at_the_committed_default():
    """profiles/drift_range_calibration.json, recomputed on the model for one clean and one drifting problem over a lag
    range around the true offsets (the DP is the full range's; the rows are narrower so that the test stays quick):
    the clean problem returns the range split's block offsets exactly at the chosen step cost, and the steep problem's
    error is below the range split's."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    try:
        import drift_range_calibration as cal
    finally:
        sys.path.pop(0)
    from workloads import cut_drift

    with open(os.path.join(ROOT, "profiles", "drift_range_calibration.json")) as f:
        doc = json.load(f)
    cost = doc["chosen"]["step_cost"]
    assert cost == dr.DEFAULT_RANGE_STEP_COST and doc["chosen"]["max_step"] == dr.DEFAULT_MAX_STEP == cal.MAX_STEP
    line = {l["step_cost"]: l for l in doc["summary"]}
    assert line[cost]["clean_problems_differing"] == 0
    assert all(line[q]["clean_problems_differing"] == 0 for q in line if q >= cost)
    assert cost == min(line) or line[cost / 2]["clean_problems_differing"] > 0  # the smallest such power of two
    assert len([r for r in doc["problems"] if r["set"] == "clean"]) >= 16
    assert len([r for r in doc["problems"] if r["set"] != "clean"]) >= 16
    k = doc["block_samples"]
    for kw in (dict(clean=True), dict(fixed=True)):
        pr = cut_drift.make_problem(0, duration_s=1200.0, **kw)
        truth = cut_drift.block_truth(pr, (pr.sub.size + k - 1) // k, k)
        rng = (int(truth.min()) - 20000, int(truth.max()) + 20000)
        split_off, by_cost = cal.solve_costs(pr, step_costs=(cost,), lag_range=rng)
        off = by_cost[cost][0]
        if kw.get("clean"):
            assert np.array_equal(off, split_off)
        else:
            e_split, e_drift = cut_drift.mean_block_error(pr, split_off, k), cut_drift.mean_block_error(pr, off, k)
            print("20 min steep problem: split error %.2f, drift error %.2f samples" % (e_split, e_drift))
            assert e_drift < e_split
