"""The split DP's optimum pinned without a GPU: the piece-structure reference (tests/piecewise_reference.py) against an
enumeration of every lag path, then the numpy models of the window aligner (split_model) and the range aligner
(cut_model) against the reference -- the total, the path's own objective and every piece's slice maximum."""
import math

import numpy as np

import cut_model as cm
import piecewise_reference as pw
import split_model as sm

INT_LEVELS = [(0.0, 1.0), (-1.0, 2.5)]  # mapped to (-1, 1) and (-3, 4)
FRACTION_LEVELS = (0.0, 24.0 / 25.0)  # mapped to (-1, 0.92): the tolerance path


def test_mapped_levels_and_slice_correlation_by_definition():
    rng = np.random.RandomState(5)
    for lv in INT_LEVELS + [FRACTION_LEVELS]:
        bits = rng.rand(50) < 0.5
        m = pw.mapped(bits, lv)
        assert np.array_equal(m, np.where(bits, 2 * lv[1] - 1, 2 * lv[0] - 1))
    assert pw.integer_levels(*INT_LEVELS) and not pw.integer_levels(INT_LEVELS[0], FRACTION_LEVELS)
    for seed in range(20):
        rng = np.random.RandomState(seed)
        R, S = int(rng.randint(1, 60)), int(rng.randint(1, 60))
        r = pw.mapped(rng.rand(R) < 0.5, INT_LEVELS[seed % 2])
        s = pw.mapped(rng.rand(S) < 0.5, INT_LEVELS[(seed // 2) % 2])
        a = int(rng.randint(0, S))
        e = int(rng.randint(a, S + 1))
        lo = int(rng.randint(-S - 10, R + 10))
        hi = lo + int(rng.randint(0, 80))
        want = [sum(s[i] * r[i + d] for i in range(a, e) if 0 <= i + d < R) for d in range(lo, hi + 1)]
        assert np.array_equal(pw.slice_corr(s, r, a, e, lo, hi), np.array(want, dtype=np.float64))


def test_fft_slice_correlation_equals_direct_sums():
    rng = np.random.RandomState(11)
    r = pw.mapped(rng.rand(40000) < 0.4, (-1.0, 2.5))
    s = pw.mapped(rng.rand(3000) < 0.5, (0.0, 1.0))
    big = pw.slice_corr(s, r, 100, 2900, -2500, 30000)  # 2800 x 32501 cells: the FFT path
    saved = pw.DIRECT_CELLS
    try:
        pw.DIRECT_CELLS = 1 << 40
        direct = pw.slice_corr(s, r, 100, 2900, -2500, 30000)
    finally:
        pw.DIRECT_CELLS = saved
    assert np.array_equal(big, direct)


def _tiny_rows(seed):
    """Block rows of a tiny problem: real bit vectors at K = 256 (2 to 5 blocks, L^B <= 50 000), or a small random
    integer table, whose many ties are where a DP's tie handling goes wrong."""
    rng = np.random.RandomState(300 + seed)
    if seed % 3 == 2:
        B = int(rng.randint(1, 7))
        L = int(rng.randint(1, max(2, int(50000 ** (1.0 / B)) + 1)))
        L = min(L, 12)
        return rng.randint(-3, 4, size=(B, L)).astype(np.float64), None
    B = int(rng.randint(1, 6))
    L = int(rng.randint(1, max(2, min(41, int(50000 ** (1.0 / B))) + 1)))
    S = (B - 1) * 256 + int(rng.randint(1, 257))
    R = int(rng.randint(100, S + 600))
    lo = int(rng.randint(-300, 300))
    rb, sb = pw.two_offset_bits(rng, R, S, (lo + int(rng.randint(0, L)), lo + int(rng.randint(0, L))), flip=0.05)
    ref = pw.Reference(rb, sb, INT_LEVELS[seed % 2], INT_LEVELS[(seed // 2) % 2], 256, lo, lo + L - 1)
    return ref.rows, ref


PENALTIES = [0.0, 0.5, 1.0, 3.0, 60.0, 1000.0, math.inf]


def test_enumerator_equals_segment_dp():
    """>= 200 tiny problems x 7 penalties: the maximum over all L^B lag paths == best[B] exactly, and the segment DP's
    own structure reaches it."""
    n = 0
    for seed in range(210):
        rows, ref = _tiny_rows(seed)
        B, L = rows.shape
        M = np.full((B + 1, B + 1), -np.inf)
        for a in range(B):
            for c in range(a + 1, B + 1):
                M[a, c] = rows[a:c].sum(axis=0).max()
        if ref is not None:
            assert np.array_equal(M, ref.M)
        for p in PENALTIES:
            top, paths = pw.enumerate_optimum(rows, p)
            best, pieces = pw.segment_dp(M, B, p)
            assert best[B] == top, (seed, p, best[B], top)
            # every piece at its slice's argmax: an optimal path (adjacent pieces at one lag would only save penalty)
            path = tuple(int(np.argmax(rows[a:c].sum(axis=0))) for a, c in pieces for _ in range(a, c))
            assert pw.path_objective(rows, path, p) == top and path in paths, (seed, p, pieces)
            n += 1
    assert n >= 200 * len(PENALTIES)


def _model_cases(n, seed0):
    """Seeded problems over the shapes the kernels meet: K in {256, 288, 800} (not only powers of two), S < K, S = nK,
    nK + 1, + 31, + 33 and free; R < S, R >> S and R shorter than one block; W in {1, 2, 31, 32, 33, 300}; integer
    levels with dyadic penalties, and every eighth problem on the tolerance path."""
    out = []
    for i in range(n):
        rng = np.random.RandomState(seed0 + i)
        k = [256, 288, 800][i % 3]
        nb = int(rng.randint(1, 8))
        S = [k // 2 + int(rng.randint(0, k // 2)), nb * k, nb * k + 1, nb * k + 31, nb * k + 33,
             int(rng.randint(k, 8 * k))][(i // 3) % 6]
        R = [max(40, S // 2), S * 3 + 500, int(rng.randint(40, k)), max(40, S + int(rng.randint(-200, 200)))][i % 4]
        w = [1, 2, 31, 32, 33, 300][int(rng.randint(0, 6))]
        d0 = int(rng.randint(-w + 1, w + 1))
        d1 = d0 + int(rng.randint(-min(w, 200), min(w, 200) + 1))
        rb, sb = pw.two_offset_bits(rng, R, S, (d0, d1))
        r_lv = INT_LEVELS[i % 2]
        s_lv = FRACTION_LEVELS if i % 8 == 7 else INT_LEVELS[(i // 2) % 2]
        p = [0.0, 0.5, 3.0, 60.0, 8192.0, math.inf][int(rng.randint(0, 6))]
        out.append(dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, k=k, w=w, p=p, rng=rng))
    return out


def test_split_model_reaches_the_optimum():
    cases = _model_cases(120, 4100)
    bad, multi, exact = [], 0, 0
    for i, c in enumerate(cases):
        offs, scores, total, pieces = sm.solve(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], c["w"], c["p"])
        ref = pw.Reference(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], -c["w"] + 1, c["w"])
        probs = pw.check_solution(ref, c["p"], offs, total, scores, [(p[0], p[1], p[4], p[5]) for p in pieces])
        multi += len(pieces) > 1
        exact += ref.exact
        if probs:
            bad.append((i, c["k"], c["w"], c["p"], probs[:3]))
    assert not bad, bad[:5]
    assert multi >= 20 and exact >= 100, (multi, exact)


def _range_cases(n, seed0):
    """Lag ranges of every kind over the same shapes: one lag (lo == hi), lo > 0, hi < 0, the full overlap range,
    ranges that reach past both overlap edges, and ranges without any overlap."""
    out = []
    for i, c in enumerate(_model_cases(n, seed0)):
        rng = c.pop("rng")
        R, S = c["rb"].size, c["sb"].size
        kind = i % 6
        if kind == 0:
            lo = hi = int(rng.randint(-S + 1, R))
        elif kind == 1:
            lo = int(rng.randint(1, R + 1))
            hi = lo + int(rng.randint(0, 400))
        elif kind == 2:
            hi = -int(rng.randint(1, S + 1))
            lo = hi - int(rng.randint(0, 400))
        elif kind == 3:
            lo, hi = cm.full_range(R, S)
        elif kind == 4:
            lo, hi = -S - int(rng.randint(0, 300)), R + int(rng.randint(0, 300))
        else:
            lo = R + int(rng.randint(0, 50))
            hi = lo + int(rng.randint(0, 300))
        out.append(dict(c, lo=lo, hi=hi))
    return out


def test_cut_model_reaches_the_optimum():
    cases = _range_cases(120, 5200)
    bad, multi, exact = [], 0, 0
    for i, c in enumerate(cases):
        offs, scores, total = cm.solve(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], c["lo"], c["hi"], c["p"])
        pieces = cm.pieces(offs, scores, c["k"], c["sb"].size)
        ref = pw.Reference(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], c["lo"], c["hi"])
        probs = pw.check_solution(ref, c["p"], offs, total, scores, [(p[0], p[1], p[4], p[5]) for p in pieces])
        multi += len(pieces) > 1
        exact += ref.exact
        if probs:
            bad.append((i, c["k"], c["lo"], c["hi"], c["p"], probs[:3]))
    assert not bad, bad[:5]
    assert multi >= 15 and exact >= 100, (multi, exact)


def test_models_at_the_exact_tie_penalty():
    """P = the exact gain of the best split over one piece: stay and switch tie, and the models still reach best[B]."""
    n = 0
    for i, c in enumerate(_model_cases(60, 6300)):
        if not pw.integer_levels(c["r_lv"], c["s_lv"]):
            continue
        ref = pw.Reference(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], -c["w"] + 1, c["w"])
        p = pw.tie_penalty(ref)
        if p is None:
            continue
        offs, scores, total, pieces = sm.solve(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], c["w"], p)
        assert not pw.check_solution(ref, p, offs, total, scores, [(q[0], q[1], q[4], q[5]) for q in pieces]), (i, p)
        offs, scores, total = cm.solve(c["rb"], c["sb"], c["r_lv"], c["s_lv"], c["k"], -c["w"] + 1, c["w"], p)
        assert not pw.check_solution(ref, p, offs, total, scores), (i, p)
        n += 1
    assert n >= 10, n


def test_check_solution_rejects_wrong_answers():
    """The checker itself: a total one off, a piece moved off its slice's maximum and a wrong block score are caught."""
    rng = np.random.RandomState(77)
    rb, sb = pw.two_offset_bits(rng, 3000, 2048, (40, 140), flip=0.02)
    ref = pw.Reference(rb, sb, (0.0, 1.0), (0.0, 1.0), 256, -299, 300)
    offs, scores, total, pieces = sm.solve(rb, sb, (0.0, 1.0), (0.0, 1.0), 256, 300, 3.0)
    assert len(pieces) == 2 and not pw.check_solution(ref, 3.0, offs, total, scores)
    assert pw.check_solution(ref, 3.0, offs, total - 1.0, scores)
    moved = offs.copy()
    moved[: pieces[0][1]] += 1
    assert pw.check_solution(ref, 3.0, moved, total, scores)
    wrong = scores.copy()
    wrong[0] += 1.0
    assert pw.check_solution(ref, 3.0, offs, total, wrong)
