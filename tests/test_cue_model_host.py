"""The numpy model of the per-cue evidence report (tests/cue_model.py) against a per-sample loop written
from the contract, independently: every field and flag, on vectors of a few hundred samples.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cue_model as cm  # noqa: E402

FIELDS = ("start", "end", "lo", "hi", "lag", "own", "best", "own_score", "best_score", "best_delta", "n_best",
          "cue_own_n11", "cue_own_ov", "cue_max_n11", "cue_max_delta", "flags", "reserved")


def brute(r, s, start, end, lag, radius, context, ref_levels, sub_levels):
    """One cue by the contract's words: a dict of the record's fields."""
    R, S = len(r), len(s)
    out = dict.fromkeys(FIELDS, 0)
    out.update(start=start, end=end, lag=lag, own=[0] * 4, best=[0] * 4, own_score=0.0, best_score=0.0)
    a, e = min(max(start, 0), S), min(max(end, 0), S)
    flags = 0
    if e <= a:
        flags |= 1
    if abs(lag) > 2 ** 31:
        flags |= 2
    if flags:
        out["flags"] = flags
        return out
    L, U = max(0, a - context), min(S, e + context)
    sv = [2.0 * sub_levels[0] - 1.0, 2.0 * sub_levels[1] - 1.0]
    rv = [2.0 * ref_levels[0] - 1.0, 2.0 * ref_levels[1] - 1.0]
    per = {}
    for delta in range(-radius, radius + 1):
        d = lag + delta
        n = [[0, 0], [0, 0]]
        for i in range(L, U):
            if 0 <= i + d < R:
                n[int(s[i])][int(r[i + d])] += 1
        cov = c11 = 0
        for i in range(a, e):
            if 0 <= i + d < R:
                cov += 1
                c11 += int(r[i + d])
        score = ((n[0][0] * (sv[0] * rv[0]) + n[0][1] * (sv[0] * rv[1])) + n[1][0] * (sv[1] * rv[0])) + n[1][1] * (sv[1] * rv[1])
        ov = n[0][0] + n[0][1] + n[1][0] + n[1][1]
        per[delta] = (score, [ov, n[1][1], n[1][0] + n[1][1], n[0][1] + n[1][1]], cov, c11)
    order = sorted(per, key=lambda x: (abs(x), -x))  # stay, +1, -1, +2, ...
    bd = order[0]
    md = order[0]
    for x in order[1:]:
        if per[x][0] > per[bd][0]:
            bd = x
        if per[x][3] > per[md][3]:
            md = x
    n_best = sum(1 for x in per if per[x][0] == per[bd][0])
    if per[0][1][0] == 0:
        flags |= 4
    if radius > 0 and abs(bd) == radius:
        flags |= 8
    if radius > 0 and n_best == 2 * radius + 1:
        flags |= 16
    if per[md][3] == 0:
        flags |= 32
    out.update(lo=L, hi=U, own=per[0][1], best=per[bd][1], own_score=per[0][0], best_score=per[bd][0], best_delta=bd,
               n_best=n_best, cue_own_n11=per[0][3], cue_own_ov=per[0][2], cue_max_n11=per[md][3], cue_max_delta=md,
               flags=flags)
    return out


def check(r, s, cues, radius, context, ref_levels=(0.0, 1.0), sub_levels=(0.0, 1.0)):
    got = cm.cue_report(r, s, cues, radius, context, ref_levels, sub_levels)
    for k in range(len(cues[0])):
        want = brute(r, s, int(cues[0][k]), int(cues[1][k]), int(cues[2][k]), radius, context, ref_levels, sub_levels)
        for f in FIELDS:
            g = got[k][f]
            if f in ("own_score", "best_score"):
                assert np.float64(g).tobytes() == np.float64(want[f]).tobytes(), (k, f, g, want[f])
            else:
                assert np.array_equal(np.asarray(g), np.asarray(want[f])), (k, f, g, want[f])
    return got


def speechy(rng, n, mean_run=12):
    seg = np.maximum(1, rng.geometric(1.0 / mean_run, size=n))
    vals = (np.arange(seg.size) + rng.randint(2)) % 2
    return np.repeat(vals, seg)[:n].astype(np.uint8)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("radius, context", [(0, 0), (5, 0), (0, 7), (9, 20), (40, 300)])
def test_model_against_per_sample_loop(seed, radius, context):
    rng = np.random.RandomState(1000 + seed)
    R, S = int(rng.randint(150, 400)), int(rng.randint(150, 400))
    r, s = speechy(rng, R), speechy(rng, S)
    start = rng.randint(-30, S + 10, 14)
    end = start + rng.randint(-3, 60, 14)
    lag = rng.randint(-R - 40, R + 40, 14)
    # windows over both ends of s; partners wholly before, wholly behind and partly outside r
    start = np.concatenate([start, [0, S - 5, -20, S - 3, 10, 10, 50]])
    end = np.concatenate([end, [S, S + 40, 15, S, 11, 40, 90]])
    lag = np.concatenate([lag, [0, 3, -2, R + 500, -S - R - 9, -25, R - 60]])
    lv = ((0.0, 1.0), (0.0, 1.0)) if seed % 2 == 0 else ((0.25, 1.0), (0.0, 1.0 / 1.001))
    check(r, s, (start, end, lag), radius, context, *lv)


def test_empty_and_invalid_records_hold_the_inputs_only():
    r, s = np.ones(100, np.uint8), np.ones(80, np.uint8)
    got = check(r, s, ([10, 90, -5, 10, 30], [10, 200, 0, 5, 40], [0, 0, 0, 7, 2 ** 31 + 1]), 3, 4)
    assert list(got["flags"]) == [cm.EMPTY, cm.EMPTY, cm.EMPTY, cm.EMPTY, cm.INVALID]
    assert not got["own"].any() and not got["lo"].any() and not got["hi"].any() and not got["n_best"].any()
    ok = check(r, s, ([30, 30], [40, 40], [2 ** 31, -2 ** 31]), 3, 4)  # the limit itself is valid: no overlap at all
    assert list(ok["flags"] & cm.INVALID) == [0, 0] and all(ok["flags"] & cm.NO_OVERLAP)


def test_all_ones_reference_is_flat_and_all_zeros_is_silent():
    rng = np.random.RandomState(5)
    s = speechy(rng, 300)
    flat = check(np.ones(400, np.uint8), s, ([100], [130], [20]), 10, 15)
    assert flat["flags"][0] == cm.FLAT and flat["best_delta"][0] == 0 and flat["n_best"][0] == 21
    assert flat["cue_max_delta"][0] == 0 and flat["cue_max_n11"][0] == 30
    silent = check(np.zeros(400, np.uint8), s, ([100], [130], [20]), 10, 15)
    assert silent["flags"][0] == cm.FLAT | cm.SILENT and silent["best_delta"][0] == 0
    # silent around the cue only: speech elsewhere in the reference, none within the radius of the cue
    r = np.ones(400, np.uint8)
    r[100:180] = 0
    near = check(r, s, ([120], [140], [10]), 10, 0)
    assert near["flags"][0] & cm.SILENT and near["cue_max_n11"][0] == 0


def test_symmetric_tie_goes_to_plus_delta():
    # s: one run [50, 60); r: runs at -16 and +16 of it, symmetric about the cue and inside the symmetric window
    s = np.zeros(120, np.uint8)
    s[50:60] = 1
    r = np.zeros(120, np.uint8)
    r[34:44] = 1
    r[66:76] = 1
    got = check(r, s, ([50], [60], [0]), 20, 30)
    assert got["best_delta"][0] == 16 and got["cue_max_delta"][0] == 16 and got["n_best"][0] == 2
    assert got["best_score"][0] > got["own_score"][0]


def test_option_order():
    d = np.arange(-3, 4)
    assert cm.first_in_option_order(np.zeros(7), d) == 3  # stay
    assert d[cm.first_in_option_order(np.array([1, 0, 0, 0, 0, 0, 1.0]), d)] == 3  # +3 over -3
    assert d[cm.first_in_option_order(np.array([1, 0, 1, 0, 0, 0, 1.0]), d)] == -1  # the smaller |delta| first
