"""The exact reference (tests/exact_reference.py) against brute force and against the reference aligner's restatement,
and the committed tests/golden/exact_golden.npz against the reference itself.  CPU only."""
import os
import sys

import numpy as np
import pytest

import exact_reference as er
import golden_cases
from oracle import aligners_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


def _levels(x):
    """(0/1 vector, (lo, hi)) of a two-level array or '0101' string; None for more than two levels."""
    x = np.array([int(ch) for ch in x], dtype=float) if isinstance(x, str) else np.asarray(x, dtype=float)
    u = np.unique(x)
    if u.size > 2:
        return None
    lo, hi = float(u.min()), float(u.max())
    return (x == hi).astype(np.uint8) if hi != lo else np.zeros(x.size, np.uint8), (lo, hi)


def _brute(ref01, sub01, ref_levels, sub_levels, max_off, M=None, info=None):
    """Every lag of the window counted by np.dot, scored by the device's chain, the maximum taken by hand."""
    R, S = ref01.size if M is None else M.size, sub01.size
    n = orc.fft_length(R, S)
    ks = np.flatnonzero(np.isfinite(orc.mask_extreme_offsets(np.zeros(n), S, max_off)))
    s = sub01.astype(np.int64)
    r = (ref01.astype(np.int64) if M is None else M)
    found = []
    for k in ks:
        d = n - 1 - S - k
        i0, i1 = max(0, -d), min(S, R - d)
        if i1 <= i0:
            sc = 0.0
        else:
            seg_s, seg_r = s[i0:i1], r[i0 + d:i1 + d]
            n11, n1x, nx1, ov = int(np.dot(seg_s, seg_r)), int(seg_s.sum()), int(seg_r.sum()), i1 - i0
            if M is None:
                c00, c01, c10, c11 = er.two_level_coefficients(ref_levels, sub_levels)
                n10, n01 = n1x - n11, nx1 - n11
                sc = er._chain((ov - n11 - n10 - n01, c00), [(n01, c01), (n10, c10), (n11, c11)])
            else:
                lam, q, _ = info
                s0, s1 = er.pm1(sub_levels[0]), er.pm1(sub_levels[1])
                base = 2.0 * lam[0] - 1.0
                sc = er._chain((ov, base * s0), [(n1x, base * (s1 - s0)), (nx1, 2.0 * q * s0), (n11, 2.0 * q * (s1 - s0))])
        found.append((sc, d))
    if not found:
        return dict(score=float("-inf"), offset=n - 1 - S, flags=1, n_at_max=0)
    top = max(sc for sc, _ in found)
    at = [d for sc, d in found if sc == top]
    return dict(score=top, offset=max(at), flags=0, n_at_max=len(at))


def _runs(rng, n, mean):
    seg = np.maximum(1, rng.geometric(1.0 / mean, size=n))
    return np.repeat(rng.rand(seg.size) < 0.45, seg)[:n].astype(np.uint8)


LEVELS = [((0.0, 1.0), (0.0, 1.0)), ((0.0, 1.0), (0.0, 0.96)), ((0.25, 1.0), (0.0, 1.0 / 1.001)), ((-1.0, 1.0), (0.1, 0.7))]


@pytest.mark.parametrize("R,S", [(97, 181), (190, 67), (129, 129), (64, 33), (5, 3)])
@pytest.mark.parametrize("max_off", [None, 0, 7, 40, 500])
def test_reference_equals_brute_force_counting(R, S, max_off):
    """R < S, R > S, lengths not multiples of 32; windows: none, a window that masks every lag (0 -- the negative
    slice), narrow, wider than the data; (0, 1), amplitude and odd levels; periodic vectors for exact ties."""
    rng = np.random.RandomState(R * 1000 + S + (max_off or 0))
    for trial, (rl, sl) in enumerate(LEVELS):
        if trial % 2:
            ref01, sub01 = _runs(rng, R, 4), _runs(rng, S, 3)
        else:  # a period shared by both: exact ties at every multiple of it
            ref01 = np.resize(np.array([1, 1, 0, 0, 0, 1, 0], np.uint8), R)
            sub01 = np.resize(np.array([1, 1, 0, 0, 0, 1, 0], np.uint8), S)
        got = er.candidate(ref01, sub01, rl, sl, max_off)
        want = _brute(ref01, sub01, rl, sl, max_off)
        assert got == want or (got["score"] == want["score"] == 0.0 and got["offset"] == want["offset"]
                               and got["n_at_max"] == want["n_at_max"]), (trial, got, want)


@pytest.mark.parametrize("max_off", [None, 30])
def test_multilevel_reference_equals_brute_force_counting(max_off):
    rng = np.random.RandomState(17)
    for R, S in [(211, 150), (150, 211)]:
        a, b = _runs(rng, R, 6), _runs(rng, R, 5)
        ref = 0.6 * a + 0.4 * b
        info = er.level_info(ref)
        assert info is not None and info[2] == [2, 1, 2]
        M = er.multilevel_weights(ref, info[0], info[2])
        assert np.array_equal(M, np.rint((ref - info[0][0]) / info[1]).astype(np.int64))  # r = lam0 + q M
        sub01 = _runs(rng, S, 4)
        for sl in [(0.0, 1.0), (0.0, 0.96)]:
            got = er.candidate_multilevel(ref, sub01, sl, max_off)
            assert got == _brute(None, sub01, None, sl, max_off, M=M, info=info)


@pytest.mark.parametrize("max_off", [None, 30])
def test_multilevel_reference_equals_brute_force_counting_on_every_level_set(max_off):
    """Every level set the run path accepts (tests/level_cases.py: divisors 1 .. 4, multiplicities up to 8, a vanishing
    base, levels outside [0, 1], float32 values), references built from nested planes; R < S and R > S."""
    import level_cases as lc

    for n, ls in enumerate(lc.ACCEPTED):
        rng = np.random.RandomState(40 + n)
        for R, S in [(397, 150), (150, 211)]:
            planes = lc._nest(ls, *(_runs(rng, R, k) != 0 for k in (6, 5, 4)))
            ref = lc.make(ls, planes)
            info = er.level_info(ref)
            assert info is not None and info[2] == ls.m and info[1] == ls.q
            M = er.multilevel_weights(ref, info[0], info[2])
            assert np.array_equal(M, sum(mk * pl for mk, pl in zip(ls.m, planes)))
            sub01 = _runs(rng, S, 4)
            for sl in [(0.0, 1.0), (0.0, 1.0 / 1.001), (-0.5, 1.25), (0.5, 1.0)]:
                got = er.candidate_multilevel(np.asarray(ref, np.float64), sub01, sl, max_off)
                want = _brute(None, sub01, None, sl, max_off, M=M, info=info)
                assert got == want or (got["score"] == want["score"] == 0.0 and got["offset"] == want["offset"]
                                       and got["n_at_max"] == want["n_at_max"]), (ls, R, S, sl, got, want)


def test_fma_emulation_rounds_once():
    eps = 2.0 ** -30
    # a*b = 1 - 2^-60 exactly: unfused rounds the product to 1.0 first
    assert (1.0 + eps) * (1.0 - eps) - 1.0 == 0.0
    assert er.fma(1.0 + eps, 1.0 - eps, -1.0) == -(2.0 ** -60)
    assert 0.1 * 10.0 - 1.0 == 0.0 and er.fma(0.1, 10.0, -1.0) == 2.0 ** -54
    # an ordinary case and the signs of exact zeros (round to nearest: +0 unless both addends are -0)
    assert er.fma(3.0, 7.0, 0.5) == 21.5
    assert np.signbit(er.fma(-0.0, 5.0, -0.0)) and not np.signbit(er.fma(0.0, 5.0, -0.0))
    assert not np.signbit(er.fma(2.0, 3.0, -6.0)) and not np.signbit(er.fma(-0.0, 5.0, 0.0))
    # the two-level chain differs from the unfused sum on amplitude levels
    c00, c01, c10, c11 = er.two_level_coefficients((0.0, 1.0), (0.0, 1.0 / 1.001))
    rng = np.random.RandomState(3)
    differ = 0
    for _ in range(200):
        n = rng.randint(0, 400000, 4)
        plain = n[0] * c00 + n[1] * c01 + n[2] * c10 + n[3] * c11
        differ += er._chain((n[0], c00), [(n[1], c01), (n[2], c10), (n[3], c11)]) != plain
    assert differ > 20


def _oracle_check(ref_levels, rec, ref_x, cand_x, max_off, tag):
    conv, S = orc.convolve_full(ref_x, cand_x)
    m = orc.mask_extreme_offsets(conv, S, max_off)
    k = int(np.argmax(m))
    s_o, o_o = m[k], len(m) - 1 - k - S
    if not np.isfinite(s_o):
        assert (rec["score"], rec["offset"], rec["flags"] & 1) == (-np.inf, o_o, 1), tag
        return
    assert rec["score"] == pytest.approx(s_o, rel=1e-6, abs=1e-6), tag
    fin = np.sort(m[np.isfinite(m)])
    if fin.size < 2 or fin[-1] - fin[-2] > 0.5:
        assert rec["offset"] == o_o, tag
    else:  # the oracle's own pick is FFT noise among tied lags: the reference's lag is one of the exact maxima
        assert rec["n_at_max"] >= 1
        assert abs(m[len(m) - 1 - S - rec["offset"]] - rec["score"]) <= 1e-6 * max(1.0, abs(rec["score"])), tag


def test_reference_against_the_oracle_on_golden_cases():
    for name, c in golden_cases.build_cases(include_large=False).items():
        r = _levels(c["ref"])
        cands = [_levels(x) for x in c["cands"]]
        if any(x is None for x in cands):
            continue  # multi-level candidates: the transform path's float products, not an exact count
        ref_x = np.array([int(ch) for ch in c["ref"]], float) if isinstance(c["ref"], str) else np.asarray(c["ref"], float)
        if r is None:
            recs, win = er.solve(ref_x, [x[0] for x in cands], None, [x[1] for x in cands], c["max_offset"], c["max_offset"])
        else:
            recs, win = er.solve(r[0], [x[0] for x in cands], r[1], [x[1] for x in cands], c["max_offset"], c["max_offset"])
        for j, (rec, cx) in enumerate(zip(recs, c["cands"])):
            _oracle_check(r, rec, ref_x, np.array([int(ch) for ch in cx], float) if isinstance(cx, str) else cx, c["max_offset"],
                          (name, j))
        try:
            (s_o, o_o), i_o = orc.max_score_align(ref_x, [np.array([int(ch) for ch in x], float) if isinstance(x, str) else x
                                                          for x in c["cands"]], c["max_offset"])
        except orc.OracleAlignmentError:
            assert win["best_cand"] == -1, name
            continue
        assert win["best_cand"] == i_o and win["score"] == pytest.approx(s_o, rel=1e-6, abs=1e-6), name


def test_reference_against_the_oracle_on_seeded_problems():
    rng = np.random.RandomState(2024)
    for trial in range(24):
        R = int(rng.randint(300, 5000))
        S = int(max(50, R * rng.uniform(0.3, 1.6)))
        ref01, sub01 = _runs(rng, R, int(rng.choice([3, 40, 300]))), _runs(rng, S, int(rng.choice([3, 40, 300])))
        if trial % 3 == 0:  # a shifted copy: a clear peak
            sub01 = np.roll(np.resize(ref01, S), int(rng.randint(-50, 50)))
        rl, sl = LEVELS[trial % len(LEVELS)]
        mo = [None, 6000, int(rng.randint(0, 3 * R)), int(rng.randint(1, 60))][trial % 4]
        rec = er.candidate(ref01, sub01, rl, sl, mo)
        ref_x = np.where(ref01 != 0, rl[1], rl[0])
        sub_x = np.where(sub01 != 0, sl[1], sl[0])
        _oracle_check(rl, rec, ref_x, sub_x, mo, (trial, R, S, mo))


def _fixture():
    return er.load_golden(os.path.join(HERE, "golden", "exact_golden.npz"))


def test_fixture_honesty_regenerated_seeds_are_bit_identical():
    import make_exact_golden as mk

    gold = _fixture()
    for kind, idx in (("headline", 0), ("headline", 517), ("windowless", 101)):
        g = gold[kind][idx]
        assert g["seed"] == idx
        new = mk.solve_seed(kind, idx)
        bits = lambda r: [[c[0].hex()] + c[1:] for c in r["cand"]] + [r["winner"][:2] + [r["winner"][2].hex()]]
        assert new["seed"] == g["seed"] and bits(new) == bits(g), (kind, idx)


def test_fixture_covers_many_exact_ties():
    gold = _fixture()
    assert [g["seed"] for g in gold["headline"]] == list(range(1024))
    assert [g["seed"] for g in gold["windowless"]] == list(range(128))
    ties = sum(c[2] >= 2 for kind in ("headline", "windowless") for g in gold[kind] for c in g["cand"])
    assert ties >= 700, ties
    for g in gold["headline"]:  # the winner is the first maximal candidate that passes the filter
        ok = [j for j, c in enumerate(g["cand"]) if not c[3] & 4]
        best = max(g["cand"][j][0] for j in ok)
        assert g["winner"][0] == next(j for j in ok if g["cand"][j][0] == best)
        assert g["winner"][1:] == [g["cand"][g["winner"][0]][1], g["cand"][g["winner"][0]][0]]
