"""Break refinement on the host (no GPU): the numpy model tests/split_refine_model.py against a brute-force search over
every (t1, t2), window clipping between close breaks and at the file ends, map_cues_refined on hand-built cases, and
argument validation."""
import math

import numpy as np
import pytest

import split_refine_model as rm
from ffsubsync_amd import split_align, split_refine
from ffsubsync_amd.split_align import Piece
from ffsubsync_amd.split_refine import RefinedBreak


def _problem(seed):
    """A small pair with two or three true offsets and block offsets that break at (or near) the true changes."""
    rng = np.random.RandomState(300 + seed)
    k = 256
    S = int(rng.randint(3 * k, 5 * k))
    R = S + 200
    rb = rng.rand(R) < 0.45
    n_b = -(-S // k)
    true = sorted(rng.choice(np.arange(1, n_b), size=min(2, n_b - 1), replace=False))
    offs = np.zeros(n_b, np.int64)
    lags = [int(rng.randint(-40, 41)) for _ in range(len(true) + 1)]
    for i, b in enumerate(true):
        offs[b:] = lags[i + 1] if lags[i + 1] != lags[i] else lags[i] + 7
    offs[:true[0]] = lags[0]
    idx = np.arange(S) + np.repeat(offs, k)[:S] + rng.randint(-30, 31)  # the true change is off the block grid
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.1
    lv = [((0.0, 1.0), (0.0, 1.0)), ((-1.0, 2.5), (0.0, 24.0 / 25.0)), ((0.3, 0.8), (-0.5, 1.25))][seed % 3]
    return rb, sb, lv[0], lv[1], offs, k


@pytest.mark.parametrize("beta", [None, 0.0, 0.25, 1.0])
def test_model_equals_brute_force(beta):
    seen_unmatched = 0
    for seed in range(6):
        rb, sb, r_lv, s_lv, offs, k = _problem(seed)
        recs = rm.refine(rb, sb, r_lv, s_lv, offs, k, 70, beta)
        assert len(recs) == len(rm.breaks_of(offs)) >= 1
        for rec in recs:
            t1, t2, v = rm.brute(rb, sb, r_lv, s_lv, int(rec["lo"]), int(rec["hi"]), int(rec["offset_prev"]),
                                 int(rec["offset_next"]), beta)
            assert (int(rec["t1"]), int(rec["t2"])) == (t1, t2), (seed, rec, t1, t2)
            assert np.float64(rec["refined_score"]).tobytes() == np.float64(v).tobytes()
            assert rec["lo"] <= rec["t1"] <= rec["t2"] <= rec["hi"]
            seen_unmatched += int(rec["t1"] < rec["t2"])
            if beta is None:
                assert rec["t1"] == rec["t2"] and not rec["flags"] & rm.UNMATCHED
    if beta is not None and beta > 0:
        assert seen_unmatched >= 1  # the margin does open unmatched stretches on noise-flipped data


def test_refined_score_is_never_below_the_coarse_cut():
    """(c, c) is one of the candidates, so the refined objective is at least the coarse cut's score when beta = None;
    with beta the coarse cut costs N(c) - N(c) = 0 for the stretch, the same value."""
    for seed in range(6):
        rb, sb, r_lv, s_lv, offs, k = _problem(seed)
        for beta in (None, 0.25):
            for rec in rm.refine(rb, sb, r_lv, s_lv, offs, k, 200, beta):
                assert rec["refined_score"] >= rec["coarse_score"] - 1e-9 * abs(rec["coarse_score"])


def test_windows_clip_between_close_breaks_and_at_the_ends():
    # radius 1000: the first window starts at 0, the last ends at S, close neighbours meet at their midpoints
    assert rm.windows([512, 1024, 4096], 5000, 1000) == [(0, 768, True), (768, 2024, True), (3096, 5000, False)]
    assert rm.windows([300], 400, 1000) == [(0, 400, False)]
    assert rm.windows([2048, 6144], 10000, 100) == [(1948, 2148, False), (6044, 6244, False)]
    assert rm.windows([257, 258], 1000, 50) == [(207, 257, True), (257, 308, True)]  # floor((257 + 258) / 2) = 257


def test_windows_in_model_records_and_flags():
    rng = np.random.RandomState(9)
    rb, sb = rng.rand(3000) < 0.5, rng.rand(2900) < 0.5
    offs = np.array([0, 0, 5, -3, -3, -3, 8, 8, 8, 8, 8, 8], np.int64)[: -(-2900 // 256)]
    recs = rm.refine(rb, sb, (0.0, 1.0), (0.0, 1.0), offs, 256, 400, 0.25)
    assert list(recs["block"]) == [2, 3, 6] and list(recs["cut"]) == [512, 768, 1536]
    assert list(recs["lo"]) == [112, 640, 1152] and list(recs["hi"]) == [640, 1152, 1936]
    assert [bool(f & rm.CLIPPED) for f in recs["flags"]] == [True, True, True]
    assert list(recs["offset_prev"]) == [0, 5, -3] and list(recs["offset_next"]) == [5, -3, 8]
    assert not (recs["reserved"]).any()


def test_window_at_file_ends_and_absent_partners():
    """A break in the first block's reach: the window starts at 0 and the lags send samples past both reference ends."""
    rng = np.random.RandomState(4)
    rb, sb = rng.rand(700) < 0.5, rng.rand(900) < 0.5
    offs = np.array([-500, 450, 450, 450], np.int64)
    for beta in (None, 0.4):
        rec = rm.refine(rb, sb, (0.0, 1.0), (0.0, 1.0), offs, 256, 5000, beta)[0]
        assert (rec["lo"], rec["hi"]) == (0, 900)
        t1, t2, v = rm.brute(rb, sb, (0.0, 1.0), (0.0, 1.0), 0, 900, -500, 450, beta) if beta is None else \
            (None, None, None)
        if beta is None:
            assert (rec["t1"], rec["t2"]) == (t1, t2)


def _pieces(*spec):
    return [Piece(0, 0, a, b, o, 0.0) for a, b, o in spec]


def _brk(t1, t2, c=None):
    c = t1 if c is None else c
    return RefinedBreak(0, c, 0, 0, t1, t2, 0, 0, 0.0, 0.0, 0)


def test_map_cues_refined_hand_built():
    pieces = _pieces((0, 1024, 100), (1024, 2048, 300), (2048, 3000, -50))
    breaks = [_brk(1000, 1000, 1024), _brk(2100, 2300, 2048)]
    # cue start samples (ratio 1, 100 Hz: 10 000 us per sample)
    starts = np.array([0, 999, 1000, 1023, 2099, 2100, 2299, 2300, 2999], np.int64)
    s_us, e_us = starts * 10000, starts * 10000 + 5000
    cs, ce, which, um = split_refine.map_cues_refined(s_us, e_us, 1.0, pieces, breaks)
    assert list(which) == [0, 0, 1, 1, 1, -2, -2, 2, 2]
    assert list(um) == [False, False, False, False, False, True, True, False, False]
    want_off = np.array([100, 100, 300, 300, 300, 300, 300, -50, -50]) * 10000  # unmatched: the earlier piece's offset
    assert np.array_equal(cs, s_us + want_off) and np.array_equal(ce, e_us + want_off)


def test_map_cues_refined_at_the_coarse_cuts_is_map_cues():
    pieces = _pieces((0, 1024, 100), (1024, 2048, 300), (2048, 3000, -50))
    rng = np.random.RandomState(1)
    s_us = np.sort(rng.randint(-20000, 3100 * 10000, 200)).astype(np.int64)
    e_us = s_us + rng.randint(1, 500000, 200)
    for ratio in (1.0, 24.0 / 25.0, 25.0 / 24.0):
        want = split_align.map_cues(s_us, e_us, ratio, pieces)
        got = split_refine.map_cues_refined(s_us, e_us, ratio, pieces, [_brk(1024, 1024), _brk(2048, 2048)])
        for a, b in zip(want, got[:3]):
            assert np.array_equal(a, b)
        assert not got[3].any()


def test_map_cues_refined_checks_its_arguments():
    pieces = _pieces((0, 1024, 100), (1024, 2048, 300))
    with pytest.raises(ValueError):
        split_refine.map_cues_refined([0], [1], 1.0, pieces, [])
    with pytest.raises(ValueError):
        split_refine.map_cues_refined([0], [1], 1.0, [], [])


@pytest.mark.parametrize("args", [
    (500, 27000, 0.25), (1024.5, 27000, 0.25), (128, 27000, 0.25), (1024, 0, 0.25), (1024, 131073, 0.25),
    (1024, 27000.5, 0.25), (1024, 27000, -0.1), (1024, 27000, math.inf), (1024, 27000, math.nan),
])
def test_argument_validation(args):
    with pytest.raises(ValueError):
        split_refine.validate_args(*args)


def test_valid_arguments_pass():
    for args in ((256, 1, None), (32768, 131072, 0.0), (1024, 27000, 0.25)):
        split_refine.validate_args(*args)
