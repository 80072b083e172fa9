"""The smooth drift fit on the CPU: the numpy model tests/drift_smooth_model.py (the contract of csrc/ffs_drift_smooth.h)
against its identities and slow references, knot placement, the lag window, the tie order, the Python layer's argument
checks, map_cues_smooth on hand-made results, and the defaults on two-hour problems."""
import itertools

import numpy as np
import pytest

import drift_model as dm
import drift_report_model as drm
import drift_smooth_model as dsm
import split_model as sm
from test_gpu_drift import _fuzz_problems


def _solved(pr):
    cnt = dsm.Counts(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"])
    m = sm.block_scores(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], n11=cnt.n11)
    off, scores, jump, _ = dm.solve(None, None, None, None, pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], m=m)
    return cnt, off, scores, jump


def _problems(n=24):
    return _fuzz_problems(n)


def test_one_block_knots_without_radius_return_the_path():
    """M = 1, R = 0: smooth_offset == block_offset and every block is a knot; with 0/1 levels the line scores are sums
    of integers, so line_score equals the segment's summed block scores."""
    checked = 0
    for pr in _problems():
        cnt, off, scores, jump = _solved(pr)
        smooth, knot, recs = dsm.fit(cnt, off, jump, 1, 0, 64.0)
        assert np.array_equal(smooth, off) and knot.all()
        segs = drm.segments_of(jump)
        assert [int(r["n_knots"]) for r in recs] == [e - f for f, e in segs]
        assert (recs["bend_total"] >= 0).all() and (recs["fit_total"] <= recs["line_score"]).all()  # the path bends
        free = dsm.fit(cnt, off, jump, 1, 0, 0.0)[2]
        assert np.array_equal(free["fit_total"], free["line_score"]) and not free["bend_total"].any()
        assert np.array_equal(free["line_score"], recs["line_score"])
        if pr["r_lv"] == (0.0, 1.0) and pr["s_lv"] == (0.0, 1.0):
            for (f, e), r in zip(segs, recs):
                if e - f > 1:
                    assert r["line_score"] == float(np.sum(scores[f:e])), (f, e)
                    checked += 1
    assert checked >= 5


def test_without_radius_the_knots_sit_on_the_path_and_lines_join_them():
    for pr in _problems():
        cnt, off, _, jump = _solved(pr)
        for m in (2, 3, 5, 16):
            smooth, knot, recs = dsm.fit(cnt, off, jump, m, 0, 8.0)
            ks = np.flatnonzero(knot)
            assert np.array_equal(smooth[ks], off[ks])
            for f, e in drm.segments_of(jump):
                kk = dsm.knots_of(f, e, m)
                assert list(ks[(ks >= f) & (ks < e)]) == kk
                for k0, k1 in zip(kk[:-1], kk[1:]):
                    lo, hi = sorted((int(off[k0]), int(off[k1])))
                    assert ((smooth[k0:k1 + 1] >= lo) & (smooth[k0:k1 + 1] <= hi)).all()
                    assert (np.diff(smooth[k0:k1 + 1]) * np.sign(int(off[k1]) - int(off[k0])) >= 0).all()  # monotone


@pytest.mark.parametrize("n,m", [(1, 8), (3, 8), (4, 8), (8, 8), (11, 8), (12, 8), (2, 5), (7, 5), (1, 1), (6, 1), (40, 256)])
def test_knot_placement_at_the_boundary_lengths(n, m):
    """n = 1, M/2 - 1, M/2, M, 3M/2 - 1, 3M/2: the last interval is the only one whose length differs from M and lies in
    [M/2, 3M/2) whenever there are two intervals or more."""
    f = 7
    ks = dsm.knots_of(f, f + n + 1, m)
    assert ks[0] == f and ks[-1] == f + n and len(ks) == max(1, (n + m // 2) // m) + 1
    gaps = np.diff(ks)
    assert (gaps[:-1] == m).all() and gaps.sum() == n and (gaps >= 1).all()
    if len(ks) > 2:
        assert m // 2 <= gaps[-1] and 2 * gaps[-1] < 3 * m
    expect = {(1, 8): 1, (3, 8): 1, (4, 8): 1, (8, 8): 1, (11, 8): 1, (12, 8): 2}
    if (n, m) in expect:
        assert len(ks) - 1 == expect[(n, m)]
    assert dsm.knots_of(f, f + 1, m) == [f]


def test_digital_line_is_monotone_ends_on_the_knots_and_floors_for_either_sign():
    for c0, c1, n in itertools.product((-7, 0, 5), (-9, 0, 4, 5, 30), (1, 2, 3, 8, 13)):
        j = np.arange(n + 1)
        d = dsm.digital_line(c0, c1, n, j)
        assert d[0] == c0 and d[-1] == c1
        assert (np.diff(d) * np.sign(c1 - c0) >= 0).all()
        exact = c0 + (c1 - c0) * j / n
        assert (np.abs(d - exact) <= 0.5).all()
        want = [c0 + int(np.floor((2 * (c1 - c0) * int(x) + n) / (2.0 * n))) for x in j]  # round half up, from a float
        assert list(d) == want
    assert dsm.digital_line(0, -1, 2, 1) == 0 and dsm.digital_line(0, 1, 2, 1) == 1  # halves go up for either sign


def test_line_table_equals_direct_counting():
    """Every line score of a two-knot segment against brute_line_score (no block counts, no prefix sums), levels other
    than 0/1 included."""
    done = 0
    for pr in _problems(21)[::3]:
        cnt, off, _, jump = _solved(pr)
        f, e = max(drm.segments_of(jump), key=lambda s: s[1] - s[0])
        if e - f < 2:
            continue
        r = 2
        n = e - 1 - f
        tab = dsm.line_table(cnt, off, f, n, True, r)
        for a, b in itertools.product(range(2 * r + 1), repeat=2):
            c0, c1 = int(off[f]) + a - r, int(off[e - 1]) + b - r
            if not (cnt.valid(c0) and cnt.valid(c1)):
                assert tab[a, b] == -np.inf
                continue
            lags = [int(x) for x in dsm.digital_line(c0, c1, n, np.arange(n + 1))]
            want = dsm.brute_line_score(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], range(f, e), lags)
            assert tab[a, b] == want, (a, b)
        done += 1
    assert done >= 4


def test_two_knot_segment_without_bend_cost_is_the_best_single_line():
    """lambda = 0, one interval: the result is the best of all (2R+1)^2 digital lines, the first in the tie order."""
    done = 0
    for pr in _problems():
        cnt, off, _, jump = _solved(pr)
        r = 3
        order = [u + r for u in dsm.tie_order(r)]
        for f, e in drm.segments_of(jump):
            n = e - 1 - f
            if n < 1:
                continue
            so, ks, lags, total, line, bend = dsm.fit_segment(cnt, off, f, e, dsm.MAX_KNOT_BLOCKS, r, 0.0)
            assert ks == [f, e - 1] and bend == 0.0 and total == line
            tab = dsm.line_table(cnt, off, f, n, True, r)
            best, arg = -np.inf, None
            for b in order:  # u_I outer, u_{I-1} inner
                for a in order:
                    if tab[a, b] > best:
                        best, arg = tab[a, b], (a, b)
            assert total == best and lags == [int(off[f]) + arg[0] - r, int(off[e - 1]) + arg[1] - r]
            assert list(so) == [int(x) for x in dsm.digital_line(lags[0], lags[1], n, np.arange(n + 1))]
            assert total >= tab[r, r]  # never below the line through the path's own ends
            done += 1
    assert done >= 20


def test_viterbi_total_equals_exhaustive_enumeration():
    """Small-integer line tables, power-of-two interval lengths and an integer bend cost: every sum is exact, so the
    Viterbi total must equal the maximum over all knot lags."""
    rng = np.random.RandomState(11)
    for trial in range(30):
        r = 1 + trial % 2
        s = 2 * r + 1
        n_int = 2 + trial % 3
        m = [2, 4, 8][trial % 3]
        ns = [m] * (n_int - 1) + [[m, m // 2][trial % 2]]  # powers of two: the division is exact
        ks = np.concatenate([[0], np.cumsum(ns)])
        off = np.cumsum(rng.randint(-2, 3, size=ks[-1] + 1)).astype(np.int64)
        tables = [rng.randint(-6, 7, size=(s, s)).astype(np.float64) * 4.0 for _ in range(n_int)]
        if trial % 5 == 0:
            tables[1][0, :] = -np.inf  # an invalid candidate
        lam = float([0.0, 1.0, 3.0, 8.0][trial % 4]) * 4.0
        bends = [dsm.bend_table(off, ks[i - 1], ns[i - 1], ns[i], m, r, lam) for i in range(1, n_int)]
        total, us = dsm.viterbi(tables, bends, r)
        assert total == dsm.brute_force_total(tables, bends, r), trial
        got = sum(tables[i][us[i] + r, us[i + 1] + r] for i in range(n_int)) - \
            sum(bends[i][us[i] + r, us[i + 1] + r, us[i + 2] + r] for i in range(n_int - 1))
        assert got == total and all(-r <= u <= r for u in us)


def test_straight_lines_cost_nothing_and_equal_intervals_cost_lambda_per_sample_of_slope_change():
    off = np.zeros(49, np.int64)
    b = dsm.bend_table(off, 0, 16, 16, 16, 2, 64.0)
    for a, m_, c in itertools.product(range(5), repeat=3):
        assert b[a, m_, c] == 64.0 * abs((c - m_) - (m_ - a))
    off = np.arange(49, dtype=np.int64) * 3  # a slope of 3 samples per block
    b = dsm.bend_table(off, 0, 16, 32, 16, 2, 64.0)
    assert b[2, 2, 2] == 0.0 and b[0, 1, 3] == 0.0  # (-2, -1, +1): 1 over 16 blocks, then 2 over 32
    assert b[2, 2, 3] == ((64.0 * 16.0) * 16.0) / 512.0


def test_ties_stay_on_the_path_and_follow_the_stated_order():
    r = 2
    s = 2 * r + 1
    flat = [np.zeros((s, s)) for _ in range(3)]
    none = [np.zeros((s, s, s))] * 2
    assert dsm.viterbi(flat, none, r) == (0.0, [0, 0, 0, 0])
    assert dsm.tie_order(3) == [0, 1, -1, 2, -2, 3, -3]
    # final state: u_I is the outer loop, so (u_{I-1}, u_I) = (-1, 0) is met before (0, +1)
    t = np.zeros((s, s))
    t[r - 1, r] = t[r, r + 1] = 5.0
    assert dsm.viterbi([t], [], r)[1] == [-1, 0]
    # and +1 before -1 on the inner loop
    t = np.zeros((s, s))
    t[r - 1, r] = t[r + 1, r] = 5.0
    assert dsm.viterbi([t], [], r)[1] == [1, 0]
    # predecessor: +1 before -1, 0 before both
    t0 = np.zeros((s, s))
    t0[r + 1, :] = t0[r - 1, :] = 3.0
    t1 = np.zeros((s, s))
    assert dsm.viterbi([t0, t1], none[:1], r)[1] == [1, 0, 0]
    t0[r, :] = 3.0
    assert dsm.viterbi([t0, t1], none[:1], r)[1] == [0, 0, 0]


def test_lines_are_clipped_by_the_lag_window():
    """A path on the window's edge: candidates outside [-W+1, W] score -inf, the fit never leaves the window, and blocks
    that overlap the reference only in part or not at all count what they overlap."""
    rng = np.random.RandomState(5)
    k, w, blocks = 256, 40, 9
    S = blocks * k - 7
    R = S + k
    seg = np.maximum(1, rng.geometric(1.0 / 8.0, size=R + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    sb = np.zeros(S, bool)
    i = np.arange(S)
    idx = i + w - np.rint(i * 6.0 / S).astype(np.int64)  # starts at lag +W, drifts down
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    cnt = dsm.Counts(rb, sb, (0.0, 1.0), (0.0, 1.0), k, w)
    m = sm.block_scores(rb, sb, (0.0, 1.0), (0.0, 1.0), k, w, n11=cnt.n11)
    off, _, jump, _ = dm.solve(None, None, None, None, k, w, np.inf, 2, 0.0, m=m)
    assert off.max() == w and not jump.any()
    tab = dsm.line_table(cnt, off, 0, 4, False, 4)
    u = np.arange(-4, 5)
    assert np.array_equal(np.isinf(tab), ((off[0] + u > w)[:, None] | (off[4] + u > w)[None, :]))
    for mk, r in ((4, 4), (2, 16), (8, 1)):
        smooth, knot, recs = dsm.fit(cnt, off, jump, mk, r, 1.0)
        assert smooth.max() <= w and smooth.min() >= -w + 1 and np.isfinite(recs["fit_total"]).all()
    # partial and empty overlaps: a reference so short that the last blocks hang over its end
    cnt2 = dsm.Counts(rb[:S - 2 * k], sb, (0.0, 1.0), (0.0, 0.75), k, w)
    t = dsm.line_table(cnt2, off, 4, 4, True, 2)
    for a, b in ((0, 0), (2, 2), (4, 1)):
        lags = [int(x) for x in dsm.digital_line(int(off[4]) + a - 2, int(off[8]) + b - 2, 4, np.arange(5))]
        if all(cnt2.valid(x) for x in (lags[0], lags[-1])):
            assert t[a, b] == dsm.brute_line_score(rb[:S - 2 * k], sb, (0.0, 1.0), (0.0, 0.75), k, range(4, 9), lags)


def test_argument_validation_of_the_python_layer():
    from ffsubsync_amd import drift_smooth as ds

    ds.validate_smooth_args(1, 0, 0.0)
    ds.validate_smooth_args(256, 16, 1e9)
    for bad in (0, 257, -1, 1.5, "x", None):
        with pytest.raises(ValueError):
            ds.validate_smooth_args(bad, 4, 1.0)
    for bad in (-1, 17, 0.5, None):
        with pytest.raises(ValueError):
            ds.validate_smooth_args(16, bad, 1.0)
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            ds.validate_smooth_args(16, 4, bad)
    # before any native call (no batch, no GPU needed to be refused)
    for kw in (dict(knot_blocks=0), dict(radius=17), dict(bend_cost=-1.0), dict(max_step=8), dict(block_samples=100)):
        with pytest.raises(ValueError):
            ds.smooth_align_batch(None, 100, **kw)
        with pytest.raises(ValueError):
            ds.smooth_sync([], **kw)
    for name in ("knot_blocks", "radius", "bend_cost"):
        with pytest.raises(ValueError):
            dsm.validate(**dict(dict(knot_blocks=16, radius=4, bend_cost=1.0), **{name: -1}))
    assert (dsm.MAX_KNOT_BLOCKS, dsm.MAX_RADIUS) == (ds._native.SMOOTH_MAX_KNOT_BLOCKS, ds._native.SMOOTH_MAX_RADIUS)


def _hand_made(segments):
    from ffsubsync_amd import drift_smooth as ds

    segs = []
    for first, end, knots in segments:
        ratios = [1.0 + (c1 - c0) / float((b1 - b0) * 1024) for (b0, c0), (b1, c1) in zip(knots[:-1], knots[1:])]
        segs.append(ds.SmoothSegment(first, end, knots, 0.0, 0.0, 0.0, ratios))
    return ds.SmoothResult(None, None, None, segs)


def test_map_cues_smooth_on_a_pure_slope_is_the_affine_map():
    from ffsubsync_amd import drift_smooth as ds

    k = 1024
    knots = [(16 * i, 100 + 3 * i) for i in range(44)] + [(703, 100 + 3 * 44)]  # the last interval has 15 blocks: bent there
    res = _hand_made([(0, 704, knots)])
    start = np.arange(0, 6_800_000_000, 7_654_321, dtype=np.int64)
    cs, ce, which = ds.map_cues_smooth(start, start + 1_500_000, 1.0, res, k, 100)
    sample = np.array([int(round(s / 1e6 * 100)) for s in start])
    inside = sample <= (16 * 43 + 0.5) * k
    want = (100.0 + 3.0 * (sample - 0.5 * k) / (16.0 * k)) * 1e4  # microseconds
    assert np.all(np.abs((cs - start)[inside] - want[inside]) <= 1.0) and inside.sum() > 800
    assert np.array_equal(ce - cs, np.full(start.size, 1_500_000)) and not which.any()
    assert ds.map_cues_smooth([0], [10], 1.0, res, k, 100)[0][0] == int(round((100.0 - 3.0 / 32.0) * 1e4))  # before the first centre
    assert res.segments[0].ratios[0] == 1.0 + 3.0 / (16 * k)


def test_map_cues_smooth_interpolates_a_staircase_between_block_centres_and_continues_the_end_slopes():
    from ffsubsync_amd import drift_smooth as ds

    k = 1024
    offs = [10, 10, 11, 13, 13, 12]
    res = _hand_made([(0, 6, list(enumerate(offs)))])  # R = 0, M = 1: every block a knot on the path

    def shift_at(sample):
        us = int(round(sample * 1e4))
        return int(ds.map_cues_smooth([us], [us + 1], 1.0, res, k, 100)[0][0]) - us

    for b, o in enumerate(offs):
        assert shift_at(b * k + k // 2) == o * 10_000  # at a block centre: the block's offset
    assert shift_at(2 * k) == 105_000 and shift_at(3 * k) == 120_000 and shift_at(5 * k) == 125_000  # boundaries: the mean
    assert shift_at(3 * k + k // 4) == int(round((11 + 2 * 0.75) * 1e4))
    assert shift_at(0) == 100_000  # before the first centre: the first interval's slope (0)
    assert shift_at(6 * k - 1) == int(round((12 - (k / 2 - 1) / k) * 1e4))  # after the last: the last interval's (-1 per block)
    assert shift_at(9 * k) == int(round((12 - 3.5) * 1e4))  # beyond the file: clamped to the last block's segment
    assert ds.polyline_shift(res.segments[0], 2.5 * k, k) == 11.0


def test_map_cues_smooth_picks_the_segment_by_block_and_one_block_segments_shift_by_their_offset():
    from ffsubsync_amd import drift_smooth as ds

    k = 1024
    res = _hand_made([(0, 4, [(0, 50), (3, 53)]), (4, 5, [(4, -200)]), (5, 9, [(5, 300), (8, 300)])])
    us = [int(round(s * 1e4)) for s in (10, 4 * k - 1, 4 * k, 5 * k - 1, 5 * k, 8 * k)]
    cs, ce, which = ds.map_cues_smooth(us, [u + 5 for u in us], 1.0, res, k, 100)
    assert list(which) == [0, 0, 1, 1, 2, 2]
    assert cs[2] - us[2] == cs[3] - us[3] == -2_000_000 and cs[4] - us[4] == cs[5] - us[5] == 3_000_000
    assert cs[1] - us[1] == int(round((53 + (k / 2 - 1) / k) * 1e4))  # past the last knot centre of segment 0: its slope
    assert np.array_equal(ce - cs, np.full(6, 5))
    with pytest.raises(ValueError):
        ds.map_cues_smooth(us, us, 1.0, ds.SmoothResult(None, None, None, []), k, 100)


def _two_hour(seed, clean):
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    pr = drift.make_problem(seed, clean=clean)
    drift_solve, smooth, knot, recs = dsm.solve(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), 1024, 6000,
                                                da.DEFAULT_SPLIT_PENALTY, da.DEFAULT_MAX_STEP, da.DEFAULT_STEP_COST,
                                                ds.DEFAULT_KNOT_BLOCKS, ds.DEFAULT_RADIUS, ds.DEFAULT_BEND_COST)
    return pr, drift_solve[0], smooth


@pytest.mark.parametrize("seed", range(8))
def test_defaults_beat_the_drift_path_on_every_drifting_problem(seed):
    from workloads import drift

    pr, off, smooth = _two_hour(seed, False)
    path, fitted = drift.mean_block_error(pr, off, 1024), drift.mean_block_error(pr, smooth, 1024)
    print("seed %d: path %.3f, fitted %.3f samples" % (seed, path, fitted))
    assert fitted < path, (seed, path, fitted)


@pytest.mark.parametrize("seed", range(8))
def test_defaults_leave_clean_problems_on_their_path(seed):
    _, off, smooth = _two_hour(seed, True)
    assert np.array_equal(off, smooth), seed
