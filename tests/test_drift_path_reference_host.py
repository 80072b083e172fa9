"""The independent drift reference (tests/drift_path_reference.py) on the CPU: its two backward passes against the
enumeration of every lag path on tiny tables, and the drift models (drift_model, drift_range_model) held to it on the
exact shape and setting lists of tests/test_gpu_drift_optimum.py -- so the models themselves reach the optimum at the
new shapes, and the problems are shown to hold moves, jumps and exact ties before any device runs them."""
import functools
import math

import numpy as np

import cut_model as cm
import drift_model as dm
import drift_path_cases as cases
import drift_path_reference as dpr
import drift_range_model as drm
import drift_range_smooth_model as drsm
import drift_smooth_model as dsm
import piecewise_reference as pw
import split_model as sm
from test_gpu_split_optimum import WINDOW_GROUPS


def test_backward_passes_equal_the_enumeration_of_all_paths():
    """Integer tables, dyadic P and Q: dense == banded == enumerator, exactly; B <= 5, L <= 6, s in 0..7 (L <= s
    occurs)."""
    rng = np.random.RandomState(4100)
    penalties = [0.0, 0.5, 3.0, 8.0, math.inf]
    step_costs = [0.0, 0.25, 1.0, 4.0, 16.0]
    n, small = 0, 0
    for i in range(400):
        B, L = int(rng.randint(1, 6)), int(rng.randint(1, 7))
        s = int(rng.randint(0, 8))
        P, Q = penalties[i % 5], step_costs[(i // 5) % 5]
        rows = rng.randint(-6, 7, size=(B, L)).astype(np.float64)
        want = dpr.enumerate_optimum(rows, P, s, Q)
        dense, banded = dpr.dense_optimum(rows, P, s, Q)[0], dpr.banded_optimum(rows, P, s, Q)[0]
        assert dense == banded == want, (i, B, L, s, P, Q, dense, banded, want)
        n += 1
        small += L <= s
    assert n == 400 and small >= 50, (n, small)
    assert dpr.banded_optimum(np.array([[1.0, 0.0], [0.0, 5.0]]), dpr.DBL_MAX, 0, 0.0)[0] == 5.0  # DBL_MAX is "never"


def test_objective_reports_the_defects():
    rows = np.array([[5.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 5.0], [0.0, 0.0, 0.0, 5.0]])
    assert dpr.objective(rows, [0, 3, 3], [0, 1, 0], 2.0, 1, 1.0) == (13.0, [])
    assert dpr.objective(rows, [0, 3, 3], [0, 0, 0], 2.0, 1, 1.0)[1] == [("unflagged move beyond max_step", 1, 3)]
    assert dpr.objective(rows, [0, 3, 3], [0, 1, 1], 0.0, 1, 1.0)[1] == [("jump that does not move", 2)]
    assert dpr.objective(rows, [0, 1, 3], [0, 0, 1], math.inf, 1, 1.0)[0] == -math.inf


@functools.lru_cache(maxsize=None)
def _window_group(gi):
    """(problems, Tally) of the window model on one group at every setting."""
    k, w, _, _ = WINDOW_GROUPS[gi]
    bad, tally = [], cases.Tally()
    for i, pr in enumerate(cases.window_pairs(gi)):
        ref = cases.reference(pr)
        m = sm.block_scores(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, w)
        for setting in cases.SETTINGS:
            offs, scores, jump, total = dm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, w, *setting, m=m)
            probs = dpr.check_solution(ref, *setting, offs, jump, total, scores)
            if probs:
                bad.append((k, w, i, setting, probs[:3]))
            else:
                tally.add(ref, setting, offs, jump)
    return bad, tally


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    k, _, _ = cases.all_range_groups()[gi]
    bad, tally = [], cases.Tally()
    for i, pr in enumerate(cases.range_pairs(gi)):
        ref = cases.reference(pr)
        pair = cm._Pair(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])
        rows = [pair.scores(b) for b in range(pair.n_blocks)]
        for si, setting in enumerate(cases.SETTINGS):
            o, jump, total = drm.dp_rows(rows, *setting)  # what drift_range_model.solve does, the rows computed once
            offs = o + pair.lo
            scores = np.array([rows[b][int(o[b])] for b in range(pair.n_blocks)])
            if si == 0:
                whole = drm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], *setting)
                assert np.array_equal(whole[0], offs) and np.array_equal(whole[1], scores) and \
                    np.array_equal(whole[2], jump) and whole[3] == float(total), (k, i)
            probs = dpr.check_solution(ref, *setting, offs, jump, float(total), scores)
            if probs:
                bad.append((k, i, (pr["lo"], pr["hi"]), setting, probs[:3]))
            else:
                tally.add(ref, setting, offs, jump)
    return bad, tally


def test_models_reach_the_optimum_and_the_problems_are_not_vacuous():
    """Every (problem, setting) of the device tests' lists: the window and the range model pass ``check_solution``; at
    least 30 solutions hold a move, 30 a jump, 10 both, and 5 an exact tie on the optimal path -- per aligner."""
    for name, group, n_groups in (("window", _window_group, len(WINDOW_GROUPS)),
                                  ("range", _range_group, len(cases.all_range_groups()))):
        bad, tally = [], cases.Tally()
        for gi in range(n_groups):
            b, t = group(gi)
            bad += b
            tally.merge(t)
        print(name, "model against the path reference:", tally.counts())
        assert not bad, bad[:5]
        assert tally.enough(), tally.counts()


def test_tile_edge_problems_cross_the_edge():
    """The extra range problems' optimal paths sit on both sides of a tile edge of the step kernel."""
    gi = len(cases.all_range_groups()) - 1
    k = cases.all_range_groups()[gi][0]
    crossed = 0
    for pr in cases.range_pairs(gi):
        if pr["hi"] - pr["lo"] + 1 <= cases.TILE:
            continue
        o = drm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], 60.0, 2, 1.0)[0] - pr["lo"]
        crossed += any(a // cases.TILE != b // cases.TILE and abs(a - b) <= 2 for a, b in zip(o[:-1], o[1:]))
    assert crossed >= 3, crossed


def _fit_problems(ref, fit, m, radius, lam):
    """``check_fit`` of a smooth model's (drift, smooth offsets, knot flags, records)."""
    drift, smooth, knot, recs = fit
    segs = [(f, e, [(b, int(smooth[b])) for b in range(f, e) if knot[b]], float(rec["fit_total"]),
             float(rec["line_score"]), float(rec["bend_total"]))
            for (f, e), rec in zip(dpr.segments_of(drift[2]), recs)]
    return dpr.check_fit(ref, m, radius, lam, drift[0], drift[2], smooth, knot, segs)


def test_smooth_models_hold_the_definition_on_the_device_tests_lists():
    """The definition check of the smooth fits (``check_fit``) on the models' fits of the groups and settings the device
    runs: no problems, polylines are fitted in every group and some of them leave the staircase."""
    for window, groups in ((True, cases.SMOOTH_WINDOW_GROUPS), (False, cases.SMOOTH_RANGE_GROUPS)):
        for gi in groups:
            pairs = cases.window_pairs(gi) if window else cases.range_pairs(gi)
            pairs = [pr for pr in pairs if pw.integer_levels(pr["r_lv"], pr["s_lv"])]
            assert len(pairs) >= 2
            bad, n_fit, n_off = [], 0, 0
            for i, pr in enumerate(pairs):
                ref = cases.reference(pr)
                for setting in cases.SMOOTH_DRIFT_SETTINGS:
                    for m, radius, lam in cases.SMOOTH_SETTINGS:
                        args = (pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"])
                        if window:
                            fit = dsm.solve(*args, pr["hi"], *setting, m, radius, lam)
                        else:
                            fit = drsm.solve(*args, pr["lo"], pr["hi"], *setting, m, radius, lam)
                        probs, a, b = _fit_problems(ref, fit, m, radius, lam)
                        n_fit += a
                        n_off += b
                        if probs:
                            bad.append((window, gi, i, setting, (m, radius, lam), probs[:3]))
            assert not bad, bad[:5]
            assert n_fit >= 6 and n_off >= 1, (window, gi, n_fit, n_off)
