"""tests/sweep_model.py against brute force on small random score tables: peaks under exclusion, ties, skipped points,
flat tables, G in {0, 1, 2}; the grid and the fine grid against their definitions."""
import math

import numpy as np
import pytest

import sweep_model as sm


def _brute_peaks(scores, offsets, flags, top_k, exclusion):
    live = [i for i in range(len(scores)) if math.isfinite(scores[i]) and not flags[i] & sm.FLAG_EMPTY_WINDOW]
    out = []
    for _ in range(top_k):
        best = None
        for i in live:  # ascending: a later equal score does not replace an earlier one
            if all(abs(i - p[2]) >= exclusion for p in out) and (best is None or scores[i] > scores[best]):
                best = i
        if best is None:
            break
        out.append((float(scores[best]), int(offsets[best]), best))
    return out


def _brute_moments(scores, flags):
    live = [float(scores[i]) for i in range(len(scores)) if math.isfinite(scores[i]) and not flags[i] & sm.FLAG_EMPTY_WINDOW]
    amb = sm.AMBIGUOUS if any(f & sm.FLAG_AMBIGUOUS for f in flags) else 0
    if not live:
        return 0.0, 0.0, amb | sm.FLAT | sm.EMPTY, len(scores)
    if all(x == live[0] for x in live):
        return live[0], 0.0, amb | sm.FLAT, len(scores) - len(live)
    mean = math.fsum(live) / len(live)
    return mean, math.sqrt(math.fsum((x - mean) ** 2 for x in live) / len(live)), amb, len(scores) - len(live)


def _table(rng, g, levels):
    scores = rng.randint(0, levels, g).astype(np.float64) * 0.5 - 3.0  # few levels: many ties
    flags = np.zeros(g, np.int32)
    kind = rng.rand(g)
    scores[kind < 0.08] = -np.inf
    flags[(kind >= 0.08) & (kind < 0.16)] |= sm.FLAG_EMPTY_WINDOW
    flags[rng.rand(g) < 0.05] |= sm.FLAG_AMBIGUOUS
    if g and rng.rand() < 0.1:
        scores[rng.randint(g)] = np.nan
    return scores, rng.randint(-6000, 6001, g).astype(np.int64), flags


@pytest.mark.parametrize("seed", range(6))
def test_peaks_and_moments_equal_brute_force(seed):
    rng = np.random.RandomState(seed)
    for g in [0, 1, 2, 3, 7, 33, 64, 129] * 4:
        scores, offsets, flags = _table(rng, g, levels=int(rng.choice([1, 2, 5, 50])))
        for top_k in (1, 3, 8):
            for exclusion in (1, 2, 5, g + 1):
                assert sm.peaks(scores, offsets, flags, top_k, exclusion) == _brute_peaks(scores, offsets, flags, top_k, exclusion)
        mean, std, fl, n_skip = sm.moments(scores, flags)
        b_mean, b_std, b_fl, b_skip = _brute_moments(scores, flags)
        assert (fl, n_skip) == (b_fl, b_skip)
        assert mean == pytest.approx(b_mean, rel=1e-12, abs=1e-12) and std == pytest.approx(b_std, rel=1e-12, abs=1e-12)
        if fl & sm.FLAT:
            assert std == 0.0 and (fl & sm.EMPTY or mean == b_mean)


def test_ties_go_to_the_smaller_index_and_exclusion_is_inclusive():
    scores = np.array([1.0, 5.0, 2.0, 5.0, 4.0, 5.0])
    off, fl = np.arange(6) * 10, np.zeros(6, np.int32)
    assert [p[2] for p in sm.peaks(scores, off, fl, 8, 1)] == [1, 3, 5, 4, 2, 0]
    assert [p[2] for p in sm.peaks(scores, off, fl, 8, 2)] == [1, 3, 5]  # |j - i| >= 2 is eligible
    assert [p[2] for p in sm.peaks(scores, off, fl, 8, 3)] == [1, 5]
    assert [p[2] for p in sm.peaks(scores, off, fl, 8, 7)] == [1]
    fl[1] = sm.FLAG_EMPTY_WINDOW  # the maximum's place is skipped: the next equal one wins
    scores[3] = -np.inf
    assert sm.peaks(scores, off, fl, 1, 1) == [(5.0, 50, 5)]
    rep = sm.report(scores, off, fl, 3, 1)
    assert (rep["n_points"], rep["n_skipped"], rep["flags"]) == (6, 2, 0)


def test_flat_and_tiny_tables():
    z = np.zeros(0)
    assert sm.report(z, z, z.astype(np.int32)) == dict(peaks=[], mean=0.0, std=0.0, n_points=0, n_skipped=0, flags=sm.FLAT | sm.EMPTY)
    one = sm.report(np.array([7.5]), np.array([3]), np.array([0], np.int32))
    assert one["peaks"] == [(7.5, 3, 0)] and (one["mean"], one["std"], one["flags"]) == (7.5, 0.0, sm.FLAT)
    same = sm.report(np.full(9, 0.1), np.arange(9), np.zeros(9, np.int32), 2, 4)
    assert (same["mean"], same["std"], same["flags"]) == (0.1, 0.0, sm.FLAT) and [p[2] for p in same["peaks"]] == [0, 4]
    gone = sm.report(np.array([-np.inf, 2.0]), np.array([1, 2]), np.array([0, sm.FLAG_EMPTY_WINDOW | sm.FLAG_AMBIGUOUS], np.int32))
    assert gone["peaks"] == [] and gone["flags"] == sm.FLAT | sm.EMPTY | sm.AMBIGUOUS and gone["n_skipped"] == 2
    assert sm.psr_margin(same) == (0.0, 0.0) and sm.psr_margin(one) == (0.0, 0.0)
    two = sm.report(np.array([1.0, 3.0]), np.array([5, 6]), np.zeros(2, np.int32), 3, 1)
    assert two["peaks"] == [(3.0, 6, 1), (1.0, 5, 0)] and (two["mean"], two["std"]) == (2.0, 1.0)
    assert sm.psr_margin(two) == (1.0, 2.0)


def test_grid_definition():
    for d, lo, hi, tol in [(59988, 0.9, 1.1, 25.0), (719990, 0.9, 1.1, 25.0), (1000, 0.95, 1.05, 1.0), (100, 1.0, 1.0, 60.0),
                           (30000, 0.9, 0.9 + 3 * 4 * 10.0 / 30000, 10.0)]:
        g, step = sm.grid(d, lo, hi, tol)
        assert step == 4.0 * tol / d and g[0] == lo and g[-1] <= hi < lo + step * g.size
        assert all(g[i] == lo + step * float(i) for i in range(g.size))
    assert sm.default_exclusion_steps(25.0) == 6 and sm.default_exclusion_steps(60.0) == 3 and sm.default_exclusion_steps(1000.0) == 1


def test_fine_grid_and_tie_rules():
    step = 1e-3
    fr, owner = sm.fine_ratios([1.0, 0.9003, 1.0999], step, 0.9, 1.1)
    assert fr.size == 3 * 33 + 7 and list(owner[:99]) == [0] * 33 + [1] * 33 + [2] * 33
    assert fr[16] == 1.0 and fr[0] == 1.0 - 16 * (step / 16) and fr[32] == 1.0 + 16 * (step / 16)
    assert fr[33:66].min() == 0.9 and fr[66:99].max() == 1.1  # clipped to [lo, hi]
    assert list(fr[99:]) == sm.SEVEN and list(owner[99:]) == [0] * 7
    assert list(sm.fine_ratios([0.95, 1.04], step, 0.9, 1.1)[1][66:]) == [1, 1, 1, 1, 1, 0, 0]  # the nearest coarse peak
    coarse = [1.0]
    r = np.array([0.5, 1.25, 0.75, 1.5])
    own = np.zeros(4, np.int64)
    none = np.zeros(4, np.int32)
    assert sm.pick(r, own, coarse, np.array([1.0, 3.0, 2.0, 3.0]), none) == 1  # nearest its coarse peak
    assert sm.pick(r, own, coarse, np.array([1.0, 3.0, 3.0, 0.0]), none) == 2  # equally near: the smaller ratio
    assert sm.pick(r, own, coarse, np.array([1.0, -np.inf, 3.0, 9.0]), np.array([0, 0, 0, sm.FLAG_EMPTY_WINDOW], np.int32)) == 2
    assert sm.pick(r, own, coarse, np.full(4, -np.inf), none) == -1
