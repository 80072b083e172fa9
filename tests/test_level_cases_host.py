"""What tests/level_cases.py claims about its own cases, asserted with the exact reference on the CPU, so that no test
of tests/test_gpu_levels_exact.py can pass vacuously: the (q, m) of every level set, the tied lags of every tie
family, where the partial-overlap winners lie, the histogram-cell values at the guard, the lists' lengths."""
import numpy as np
import pytest

import exact_reference as er
import level_cases as lc
from oracle import runs_model as rm

F64 = np.float64
SET_IDS = [ls.name for ls in lc.ACCEPTED]


def _solve(p, max_off):
    return er.solve(np.asarray(p[1], F64), p[2], None, p[3], max_off, max_off)


def _planes(ref):
    lam, q, m = er.level_info(ref)
    return [np.asarray(ref, F64) >= x for x in lam[1:]], m


def test_accepted_sets_return_their_q_and_m_and_rejected_sets_none():
    for ls in lc.ACCEPTED:
        lam, q, m = er.level_info(ls.levels)
        assert lam == [float(x) for x in ls.levels] and m == ls.m and q == ls.q, (ls, lam, q, m)
        # a vector in the set's own type holds the levels exactly and decomposes into its planes
        rng = np.random.RandomState(1)
        planes = lc._nest(ls, *(lc._noise(rng, 500, 5, 0.5) for _ in range(3)))
        ref = lc.make(ls, planes)
        assert ref.dtype == ls.dtype and np.array_equal(np.unique(ref), ls.levels)
        M = er.multilevel_weights(ref, lam, m)
        assert np.array_equal(M, sum(mk * pl for mk, pl in zip(m, planes)))
    for ls in lc.REJECTED:
        assert er.level_info(ls.levels) is None, ls
    # the float32 `weighted` set is refused only because of its rounding: the same levels in float64 are accepted
    assert er.level_info(lc.BY_NAME["weighted_rounded_f32"].levels.astype(F64).round(6)) is not None
    assert {ls.name for ls in lc.ACCEPTED} >= set(lc.PARTIAL_SETS) >= {"steps_8_1_8", "base_zero"} and len(lc.PARTIAL_SETS) >= 4


def test_the_largest_reachable_sum_of_multiplicities():
    """Every triple of integer steps up to 8 (and beyond: 9 is refused) through the level analysis."""
    best = 0
    for a in range(1, 10):
        for b in range(1, 10):
            for c in range(1, 10):
                info = er.level_info(np.cumsum([0, a, b, c]) / float(a + b + c))
                if info is not None:
                    best = max(best, sum(info[2]))
    assert best == lc.SUM_M_MAX == sum(lc.BY_NAME["steps_3_8_8"].m)


@pytest.mark.parametrize("ls", lc.ACCEPTED, ids=SET_IDS)
def test_tie_families_hold_their_ties(ls):
    total = 0
    for max_off in (None, 6000, 3):
        periodic, flat = lc.periodic_ties(ls, max_off), lc.flat_tops(ls)
        ties = 0
        for p in periodic + flat:
            assert np.array_equal(np.unique(p[1]), ls.levels), p[0]  # every level present: the set the test names
            recs, _ = _solve(p, max_off)
            ties += sum(r["n_at_max"] >= 2 for r in recs)
            n0 = recs[0]["n_at_max"]
            if max_off != 3 and p[0].startswith("periodic"):
                assert n0 >= (16 if max_off is None else 3), (p[0], max_off, n0)
                assert recs[2]["n_at_max"] == n0  # (the amplitude candidate ties on the same lags)
                d_lo, d_top = lc.window(lc.TIE_R, lc.TIE_S, max_off)
                at = {"periodic_tile_last": d_lo + lc.RUNS_T - 1, "periodic_tile_first": d_lo, "periodic_window_top": d_top}[p[0]]
                assert (recs[0]["offset"] - at) % lc.TIE_P == 0, (p[0], recs[0]["offset"], at)
            if max_off != 3 and p[0].startswith("flat") and ls.name != "base_zero":
                assert n0 >= int(p[0].rsplit("_", 1)[1]) >= 41, (p[0], max_off, n0)
        assert ties >= lc.min_tie_records(ls, max_off), (max_off, ties)
        total += lc.min_tie_records(ls, max_off)
    assert total * len(lc.ACCEPTED) >= 40  # tie records over the GPU test's parameters
    assert int(lc.flat_tops(ls)[1][0].rsplit("_", 1)[1]) >= 300


@pytest.mark.parametrize("max_off", [None, 6000])
def test_broken_ties_have_one_winner_below_the_largest_tied_lag(max_off):
    for ls in lc.ACCEPTED:
        broken, unbroken, d0 = lc.broken_tie(ls, max_off)
        assert int((broken[1] != unbroken[1]).sum()) == 1 and np.array_equal(np.unique(broken[1]), ls.levels)
        x = int(np.flatnonzero(broken[1] != unbroken[1])[0])
        pl_b, m = _planes(broken[1])
        pl_u, _ = _planes(unbroken[1])
        changed = [k for k in range(len(m)) if pl_b[k][x] != pl_u[k][x]]
        assert changed == [int(np.argmin(m))], (ls, changed)  # one plane, the one with the smallest m_k
        rb, ru = _solve(broken, max_off)[0], _solve(unbroken, max_off)[0]
        for b, u in zip(rb, ru):
            assert u["n_at_max"] >= (16 if max_off is None else 4) and b["n_at_max"] == 1, (ls, b, u)
            assert b["offset"] == d0 < u["offset"], (ls, b, u)


def test_zero_rule_relatives():
    ls = lc.BY_NAME["base_zero"]
    lam, q, m = er.level_info(ls.levels)
    assert 2.0 * lam[0] - 1.0 == 0.0
    all_zero, equal, equal_amp = lc.zero_rule()
    for p in (all_zero, equal, equal_amp):
        assert all(er.pm1(lv[0]) == 0.0 for lv in p[3])  # k0 = k1x = kx1 = 0
    for max_off in (None, 6000, 3):
        recs, win = _solve(all_zero, max_off)
        n_lags = er.qm.lag_set(lc.ZERO_R, lc.ZERO_S, max_off).size
        assert recs[0]["score"] == 0.0 and recs[0]["n_at_max"] == n_lags and recs[2]["n_at_max"] == n_lags
        for p in (equal, equal_amp):
            recs, win = _solve(p, max_off)
            if max_off != 3:
                assert recs[0]["score"] == recs[1]["score"] == recs[2]["score"] > 0 and win["best_cand"] == 0
                assert abs(recs[0]["offset"] - recs[1]["offset"]) == 300


@pytest.mark.parametrize("name", lc.PARTIAL_SETS)
def test_partial_overlap_winners_lie_at_partial_overlap(name):
    probs = lc.partial_overlap(lc.BY_NAME[name])
    assert len(probs) == 64
    partial, shorter = 0, 0
    for p in probs:
        R, S = p[1].size, p[2][0].size
        assert 2100 <= R <= 12000 and 2100 <= S <= 12000  # (transform length >= 4096: not the direct kernel)
        recs, win = _solve(p, None)
        d = win["offset"]
        partial += min(S, R - d) - max(0, -d) < S
        shorter += R < S
    assert partial >= 24 and 8 <= shorter <= 56, (partial, shorter)
    assert {p[3][0] for p in probs} == {(0.0, 1.0), (0.0, 1.0 / 1.001), (-0.5, 1.25)}


def test_negative_slice_windows_leave_a_few_lags():
    probs, windows = lc.negative_slice(lc.BY_NAME["weighted_label_0"])
    n = er.orc.fft_length(lc.NEG_R, lc.NEG_S)
    assert n >= 4096
    for w, count in zip(windows, (1, 8, 30)):
        assert w > n - 1 - lc.NEG_S
        lags = er.qm.lag_set(lc.NEG_R, lc.NEG_S, w)
        assert lags.size == count and lags.min() == -lc.NEG_S, (w, lags)
    assert any(r["score"] != 0.0 for p in probs for r in _solve(p, windows[-1])[0])


def test_cell_guard_values():
    ls = lc.BY_NAME["steps_1_8"]
    for n, cell in ((3640, 32760), (3642, 32778)):
        name, ref, cands, _ = lc.cell_guard(n)
        planes, m = _planes(ref)
        assert m == [1, 8] and [rm.boundaries(p)[0].size for p in planes] == [n + 2, n] and rm.boundaries(cands[0])[0].size == n
        assert lc.cell_bound(ls, ref, cands[0]) == cell
        assert er.qm.lag_set(ref.size, cands[0].size, None).size <= lc.RUNS_T  # one tile
        assert n < lc.STRIDE0  # (no stride retry involved)
    assert 32760 <= 32767 < 32768 <= 32778 and 9 * 3641 > 32767  # the largest even count below the guard, the first at or above it


def test_plane_tail_lengths_and_end_samples():
    want = {16384 * k + e for k in (1, 2) for e in (-1, 0, 1)}
    assert want <= set(lc.TAIL_LENGTHS)
    assert any(abs(R - 1024 * round(R / 1024)) == 1 and R not in want and abs(R - 16384) < 2048 for R in lc.TAIL_LENGTHS)
    assert any(abs(R - 128 * round(R / 128)) == 1 and abs(R - 1024 * round(R / 1024)) > 1 for R in lc.TAIL_LENGTHS)
    for name in ("weighted_label_0", "dyadic_f32_1_1_2"):
        ls = lc.BY_NAME[name]
        probs = lc.plane_tails(ls)
        assert [p[1].size for p in probs] == lc.TAIL_LENGTHS and max(lc.TAIL_LENGTHS) <= 40000
        for p in probs:
            ref = p[1]
            assert ref[0] == ref[-1] == ls.levels[-1] and ref[-2] == ls.levels[0] and np.array_equal(np.unique(ref), ls.levels)
            assert abs(p[2][0].size - ref.size / 3.0) < 1.0


def test_stride_cases_are_dense_and_sparse_where_they_claim():
    for p in lc.dense_planes():
        planes, m = _planes(p[1])
        n_q = [rm.boundaries(pl)[0].size for pl in planes]
        assert len(planes) == 3 and min(n_q) > lc.STRIDE0 and max(n_q) < 16384, n_q  # one growth (x 4) suffices
        assert lc.cell_bound(lc.BY_NAME["weighted_label_0"], p[1], p[2][0]) < 32768
    for p in lc.long_candidate_lists():
        planes, m = _planes(p[1])
        assert max(rm.boundaries(pl)[0].size for pl in planes) < lc.STRIDE0 // 4
        for c in p[2]:
            assert lc.STRIDE0 < rm.boundaries(c)[0].size < 32768
            assert lc.cell_bound(lc.BY_NAME["weighted_label_0"], p[1], c) < 32768
    alt = lc.alternating_list_candidate(lc.BY_NAME["weighted_label_0"])
    pos = rm.boundaries(alt[2][0])[0]
    assert np.all(np.diff(pos) == 1) and pos.size > 8 * lc.RUNS_EDGE  # every 32-sample window holds 32 entries


def test_neighbour_problems_stay_inside_the_coincidence_budget():
    """"auto" sends a sub-batch through the transforms when sum_k n_p n_q (W / R) exceeds 12 N (n_cand + 1) / (2 n_cand)
    (csrc/ffsalign.hip); N >= 8192 for these lengths, three candidates: 65 536.  The neighbours' problems stay below
    half of it, so only the odd pairs' sub-batches take the transforms."""
    for k, ls in enumerate(lc.ACCEPTED):
        name, ref, cands, _ = lc.small_problem(ls, k)
        planes, m = _planes(ref)
        assert m == ls.m
        n_q = sum(rm.boundaries(pl)[0].size for pl in planes)
        for c in cands:
            assert rm.boundaries(c)[0].size * n_q * 6001 // ref.size < 65536 // 2, (ls, n_q)
    for name in ("five_levels", "weighted_rounded_f32"):
        p = lc.odd_pair(lc.BY_NAME[name], 0)
        assert er.level_info(p[1]) is None and 0.0 <= p[1].min() and p[1].max() <= 1.0


def test_transform_rule_accepts_the_exact_winner_and_refuses_its_neighbour():
    p = lc.small_problem(lc.BY_NAME["weighted_label_0"], 3)
    recs, _ = _solve(p, 3000)
    d = recs[1]["offset"]
    assert lc.transform_rule_bad(p[1], p[2][1], p[3][1], 3000, d) is None
    assert lc.transform_rule_bad(p[1], p[2][1], p[3][1], 3000, d + 1) is not None
    assert lc.transform_rule_bad(p[1], p[2][1], p[3][1], 3000, 3001) is not None
