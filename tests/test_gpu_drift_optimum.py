"""The drift aligners on the device against the independent lag-path reference (tests/drift_path_reference.py), not
against their step-for-step models: ffs_align_drift_batch (k_drift_dp) and ffs_align_drift_range_batch
(k_range_drift_step / k_range_drift_backtrack) reach the maximum over ALL lag paths, the returned path's objective is
the returned total, jumps move and unflagged steps stay within max_step, block scores and segments hold together, and
the documented edges hold -- P = DBL_MAX as P = inf, -0.0 as 0, max_step = 0 as the split aligners, U8 as U1, the range
aligner at [-W + 1, W] as the window aligner.  The shapes are the ones of tests/test_gpu_split_optimum.py, which no
other drift test reaches on the device: W = 1 and 2 (fewer lags than max_step), 2W = 262 144, K that are not powers of
two and K = 32 768, tail blocks of 1 to 33 samples, R < S, one-lag ranges, ranges without overlap, 282 999 lags on one
row, five lags under max_step = 7 and paths that step across a tile edge of the range step kernel.  The smooth fits
(k_drift_line_sums / k_drift_knot_dp and their range forms) are held to their definition in csrc/ffs_drift_smooth.h.

tests/test_drift_path_reference_host.py holds the models to the same reference on the same lists on the CPU."""
import functools

import numpy as np
import pytest

import drift_path_cases as cases
import drift_path_reference as dpr
import piecewise_reference as pw
from test_gpu_split_optimum import WINDOW_GROUPS, _device_pairs

pytestmark = pytest.mark.gpu

SETTINGS = cases.SETTINGS
N_RANGE_GROUPS = len(cases.all_range_groups())


def _drift_bytes(res):
    return (res.block_offsets.tobytes(), res.block_scores.tobytes(), res.block_jump.tobytes(),
            np.float64(res.total).tobytes())


def _split_bytes(res):
    return (res.block_offsets.tobytes(), res.block_scores.tobytes(), np.float64(res.total).tobytes())


def _segments(res):
    return [(g.first_block, g.end_block, g.first_offset, g.last_offset, g.score) for g in res.segments]


def _check_group(name, refs, by_setting, u8, split):
    """(problems, Tally, solutions checked) of one group: ``by_setting[si][i]`` the DriftResult of pair i at
    SETTINGS[si], ``u8`` the U8 call at SETTINGS[I_U8], ``split`` the split aligner's results at SETTINGS[I_SPLIT]."""
    bad, tally, checked = [], cases.Tally(), 0
    for si, setting in enumerate(SETTINGS):
        assert len(by_setting[si]) == len(refs)
        for i, (ref, res) in enumerate(zip(refs, by_setting[si])):
            probs = dpr.check_solution(ref, *setting, res.block_offsets, res.block_jump, res.total, res.block_scores,
                                       _segments(res))
            checked += 1
            if probs:
                bad.append((name, i, setting, probs[:3]))
            else:
                tally.add(ref, setting, res.block_offsets, res.block_jump)
    assert len(u8) == len(split) == len(refs)
    for i in range(len(refs)):
        if _drift_bytes(by_setting[cases.I_MAX][i]) != _drift_bytes(by_setting[cases.I_INF][i]):
            bad.append((name, i, "P = DBL_MAX differs from P = inf"))
        if _drift_bytes(by_setting[cases.I_NZERO][i]) != _drift_bytes(by_setting[cases.I_ZERO][i]):
            bad.append((name, i, "P = -0.0 differs from P = 0"))
        if _drift_bytes(u8[i]) != _drift_bytes(by_setting[cases.I_U8][i]):
            bad.append((name, i, "U8 records differ from U1"))
        zero = by_setting[cases.I_SPLIT][i]
        if _split_bytes(zero) != _split_bytes(split[i]):
            bad.append((name, i, "max_step = 0 differs from the split aligner"))
        if np.any(by_setting[cases.I_INF][i].block_jump):
            bad.append((name, i, "a jump at P = inf"))
    return bad, tally, checked


@functools.lru_cache(maxsize=None)
def _window_group(gi):
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import split_align as sa

    k, w, pif, _ = WINDOW_GROUPS[gi]
    pairs = cases.window_pairs(gi)
    refs = [cases.reference(pr) for pr in pairs]
    db = _device_pairs(pairs)
    by_setting = [da.drift_align_batch(db, w, k, p, s, q, pairs_in_flight=pif) for p, s, q in SETTINGS]
    u8 = da.drift_align_batch(_device_pairs(pairs, packed=False), w, k, *SETTINGS[cases.I_U8], pairs_in_flight=pif)
    split = sa.split_align_batch(db, w, k, SETTINGS[cases.I_SPLIT][0], pairs_in_flight=pif)
    da.clear_plan_cache()
    bad, tally, checked = _check_group("window K=%d W=%d" % (k, w), refs, by_setting, u8, split)
    return bad, tally, checked, len(pairs)


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr

    k, pif, _ = cases.all_range_groups()[gi]
    pairs = cases.range_pairs(gi)
    ranges = [(pr["lo"], pr["hi"]) for pr in pairs]
    refs = [cases.reference(pr) for pr in pairs]
    db = _device_pairs(pairs)
    by_setting = [dr.drift_align_range_batch(db, ranges, k, p, s, q, pairs_in_flight=pif) for p, s, q in SETTINGS]
    u8 = dr.drift_align_range_batch(_device_pairs(pairs, packed=False), ranges, k, *SETTINGS[cases.I_U8],
                                    pairs_in_flight=pif)
    split = ca.split_align_range_batch(db, ranges, k, SETTINGS[cases.I_SPLIT][0], pairs_in_flight=pif)
    dr.clear_plan_cache()
    ca.clear_plan_cache()
    bad, tally, checked = _check_group("range K=%d" % k, refs, by_setting, u8, split)
    return bad, tally, checked, len(pairs)


@pytest.mark.parametrize("gi", range(len(WINDOW_GROUPS)))
def test_window_aligner_reaches_the_optimum(gi):
    bad, _, checked, n_pairs = _window_group(gi)
    assert checked == n_pairs * len(SETTINGS) and n_pairs == len(WINDOW_GROUPS[gi][3])  # every pair, every setting
    assert not bad, bad[:5]


@pytest.mark.parametrize("gi", range(N_RANGE_GROUPS))
def test_range_aligner_reaches_the_optimum(gi):
    bad, _, checked, n_pairs = _range_group(gi)
    assert checked == n_pairs * len(SETTINGS) and n_pairs == len(cases.all_range_groups()[gi][2])
    assert not bad, bad[:5]


def test_the_problems_hold_moves_jumps_and_ties_on_the_device():
    """Counted on the device's solutions that passed every check (a group not run yet in this process runs here): at
    least 30 with a move, 30 with a jump, 10 with both, 5 with an exact tie on the optimal path -- per aligner; and
    the lists reach what the module's docstring says they reach."""
    for name, group, n in (("window", _window_group, len(WINDOW_GROUPS)), ("range", _range_group, N_RANGE_GROUPS)):
        tally = cases.Tally()
        for gi in range(n):
            tally.merge(group(gi)[1])
        print(name, "aligner on the device against the path reference:", tally.counts())
        assert tally.enough(), (name, tally.counts())
    shapes = [(k, w) for k, w, _, _ in WINDOW_GROUPS]
    assert {w for _, w in shapes} >= {1, 2, 131072} and {k for k, _ in shapes} >= {288, 800, 2080, 32768}
    lags = [pr["hi"] - pr["lo"] + 1 for gi in range(N_RANGE_GROUPS) for pr in cases.range_pairs(gi)]
    assert 1 in lags and 5 in lags and max(lags) > 262144


def test_range_aligner_over_the_window_equals_the_window_aligner():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_range as dr

    k, w, pif, _ = WINDOW_GROUPS[cases.PARITY_WINDOW_GROUP]
    pairs = cases.window_pairs(cases.PARITY_WINDOW_GROUP)
    db = _device_pairs(pairs)
    n = 0
    for p, s, q in SETTINGS:
        window = da.drift_align_batch(db, w, k, p, s, q, pairs_in_flight=pif)
        ranged = dr.drift_align_range_batch(db, (-w + 1, w), k, p, s, q, pairs_in_flight=pif)
        for i, (a, b) in enumerate(zip(window, ranged)):
            assert _drift_bytes(a) == _drift_bytes(b) and _segments(a) == _segments(b), (p, s, q, i)
            n += 1
    da.clear_plan_cache()
    dr.clear_plan_cache()
    assert n == len(pairs) * len(SETTINGS)


# ---- the smooth fits, by the definition in csrc/ffs_drift_smooth.h ---------------------------------------------------

def _check_fit(ref, res, m, radius, lam):
    segs = [(g.first_block, g.end_block, g.knots, g.fit_total, g.line_score, g.bend_total) for g in res.segments]
    d = res.drift
    return dpr.check_fit(ref, m, radius, lam, d.block_offsets, d.block_jump, res.smooth_offsets, res.knot, segs)


def _check_smooth_group(name, pairs, solve):
    exact = [pr for pr in pairs if pw.integer_levels(pr["r_lv"], pr["s_lv"])]
    assert len(exact) >= 2, name
    refs = [cases.reference(pr) for pr in exact]
    db = _device_pairs(exact)
    bad, n_fit, n_off, checked = [], 0, 0, 0
    for setting in cases.SMOOTH_DRIFT_SETTINGS:
        for m, radius, lam in cases.SMOOTH_SETTINGS:
            results = solve(db, exact, setting, m, radius, lam)
            assert len(results) == len(exact)
            for i, (ref, res) in enumerate(zip(refs, results)):
                d = res.drift
                probs = dpr.check_solution(ref, *setting, d.block_offsets, d.block_jump, d.total, d.block_scores)
                fit_probs, a, b = _check_fit(ref, res, m, radius, lam)
                checked += 1
                n_fit += a
                n_off += b
                if probs or fit_probs:
                    bad.append((name, i, setting, (m, radius, lam), (probs + fit_probs)[:3]))
    assert checked == len(exact) * len(cases.SMOOTH_DRIFT_SETTINGS) * len(cases.SMOOTH_SETTINGS)
    assert not bad, bad[:5]
    assert n_fit >= 6 and n_off >= 1, (n_fit, n_off)  # polylines were fitted, and some left the staircase


@pytest.mark.parametrize("gi", cases.SMOOTH_WINDOW_GROUPS)
def test_window_smooth_fit_holds_its_definition(gi):
    from ffsubsync_amd import drift_smooth as ds

    k, w, pif, _ = WINDOW_GROUPS[gi]

    def solve(db, pairs, setting, m, radius, lam):
        return ds.smooth_align_batch(db, w, k, *setting, m, radius, lam, pairs_in_flight=pif)

    _check_smooth_group("window K=%d W=%d" % (k, w), cases.window_pairs(gi), solve)
    ds.clear_plan_cache()


@pytest.mark.parametrize("gi", cases.SMOOTH_RANGE_GROUPS)
def test_range_smooth_fit_holds_its_definition(gi):
    from ffsubsync_amd import drift_range_smooth as drs

    k, pif, _ = cases.all_range_groups()[gi]

    def solve(db, pairs, setting, m, radius, lam):
        return drs.smooth_align_range_batch(db, [(pr["lo"], pr["hi"]) for pr in pairs], k, *setting, m, radius, lam,
                                            pairs_in_flight=pif)

    _check_smooth_group("range K=%d" % k, cases.range_pairs(gi), solve)
    drs.clear_plan_cache()
