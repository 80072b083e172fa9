"""The numpy model of the joint cue retiming (tests/retime_model.py) against the enumeration of every path
(tests/retime_reference.py), its invariants and limiting cases, and its fast evaluation against the plain one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cue_model as cm  # noqa: E402
import retime_model as rm  # noqa: E402
import retime_reference as rr  # noqa: E402

PENALTIES = (0, 1, 64, 1000)


def _tiny(rng, max_cues=7):
    """A tiny case: vectors of 20-80 samples, cues that overlap, repeat, go out of order and are skipped in the middle."""
    R, S = int(rng.randint(20, 81)), int(rng.randint(20, 81))
    r, s = (rng.rand(R) < 0.5).astype(np.uint8), (rng.rand(S) < 0.5).astype(np.uint8)
    K = int(rng.randint(1, max_cues + 1))
    st = rng.randint(-3, S, K)
    if rng.rand() < 0.5:
        st = np.sort(st)
    en, lag = st + rng.randint(0, 14, K), rng.randint(-6, 7, K)
    if K >= 3 and rng.rand() < 0.5:  # a repeated cue and a skipped one in the middle
        st[1], en[1], lag[1] = st[0], en[0], lag[0]
        en[K // 2] = st[K // 2] if rng.rand() < 0.5 else en[K // 2]
        lag[K // 2] = 2 ** 31 + 5 if rng.rand() < 0.3 else lag[K // 2]
    return r, s, (st.astype(np.int64), en.astype(np.int64), lag.astype(np.int64))


def _invariants(recs, summ, radius, penalty_q, jump_q):
    live = recs[(recs["flags"] & 3) == 0]
    skipped = recs[(recs["flags"] & 3) != 0]
    assert summ["own_total"] <= summ["total"] <= summ["best_total"]
    assert summ["total"] == 64 * int(live["at"].astype(np.int64).sum()) - int(live["link"].sum())
    assert summ["n_live"] == live.size and summ["n_moved"] == (live["delta"] != 0).sum()
    assert summ["n_jumps"] == ((live["flags"] & rm.JUMP) != 0).sum() and (jump_q >= 0 or summ["n_jumps"] == 0)
    assert (np.abs(live["delta"]) <= radius).all() and (live["at"] <= live["best"]).all() and (live["own"] <= live["best"]).all()
    for f in ("delta", "own", "at", "best", "best_delta", "link"):
        assert not skipped[f].any()
    if live.size:
        assert live["link"][0] == 0
        want = penalty_q * np.abs(np.diff(live["delta"].astype(np.int64)))
        assert np.array_equal(live["link"][1:], np.minimum(want, jump_q) if jump_q >= 0 else want)


@pytest.mark.parametrize("jump", [False, True])
@pytest.mark.parametrize("keep_order", [True, False])
def test_the_model_reaches_the_enumerated_optimum(keep_order, jump):
    rng = np.random.RandomState(31 + 2 * keep_order + jump)
    n, seen_skip, seen_unordered = 0, 0, 0
    while n < 64:  # 4 x 64 = 256 cases
        r, s, cues = _tiny(rng)
        if len(rr.live_cues(s.size, cues)) > rr.MAX_LIVE:
            continue
        radius, context = n % 4, int(rng.randint(0, 6))
        pq = PENALTIES[(n // 4) % 4]
        jq = (0, 70, 900, 1 << 40)[(n // 16) % 4] if jump else -1
        recs, summ = rm.retime(r, s, cues, radius, context, pq, jq, keep_order)
        ref = rr.Reference(r, s, cues, radius, context, pq, jq, keep_order)
        live = recs[(recs["flags"] & 3) == 0]
        assert [k for k, *_ in ref.live] == np.flatnonzero((recs["flags"] & 3) == 0).tolist()
        assert int(summ["total"]) == ref.optimum(), (n, summ)
        assert ref.value([int(x) for x in live["delta"]]) == ref.optimum()  # the path is admissible and attains it
        assert [int(x) for x in live["own"]] == [a[0] for a in ref.A]
        _invariants(recs, summ, radius, pq, jq)
        seen_skip += int(0 < live.size < recs.size)
        seen_unordered += int(((recs["flags"] & rm.UNORDERED) != 0).any())
        n += 1
    assert seen_skip >= 5 and (seen_unordered >= 5) == keep_order


def test_the_fast_evaluation_equals_the_plain_one():
    rng = np.random.RandomState(4)
    for n in range(120):
        r, s, cues = _tiny(rng, max_cues=12)
        radius, context = int(rng.randint(0, 13)), int(rng.randint(0, 9))
        pq, jq, keep = PENALTIES[n % 4], (-1, 0, 70, 900, 1 << 40)[n % 5], n % 3 != 0
        a, sa = rm.retime(r, s, cues, radius, context, pq, jq, keep)
        b, sb = rm.retime_fast(r, s, cues, radius, context, pq, jq, keep)
        assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes(), n
        _invariants(a, sa, radius, pq, jq)
    # the largest penalty and radius, and many settings at once
    r, s = (rng.rand(400) < 0.5).astype(np.uint8), (rng.rand(380) < 0.5).astype(np.uint8)
    st = np.sort(rng.randint(0, 340, 9)).astype(np.int64)
    cues = (st, st + 20, rng.randint(-3, 4, 9).astype(np.int64))
    settings = [(0, -1), (1 << 20, -1), (1 << 20, 1 << 40), (3, 50), (64, 0)]
    flags, pos, A = rm.profiles(cm.Pair(r, s), cues, 40, 5)
    paths, totals = rm.retime_paths(flags, pos, A, 40, settings, True)
    for (pq, jq), path, total in zip(settings, paths, totals):
        recs, summ = rm.retime(r, s, cues, 40, 5, pq, jq, True)
        assert recs["delta"].tolist() == path.tolist() and int(summ["total"]) == int(total)


def test_limiting_cases():
    rng = np.random.RandomState(12)
    for n in range(40):
        r, s, cues = _tiny(rng, max_cues=9)
        radius, context = int(rng.randint(0, 6)), int(rng.randint(0, 6))
        # no penalty, order off: every live cue sits at the cue report's own best shift at unit levels
        recs, _ = rm.retime(r, s, cues, radius, context, 0, -1, False)
        rep = cm.cue_report(r, s, cues, radius, context)
        live = (recs["flags"] & 3) == 0
        assert np.array_equal(live, (rep["flags"] & 3) == 0)
        assert np.array_equal(recs["delta"][live], rep["best_delta"][live])
        assert np.array_equal(recs["best_delta"][live], rep["best_delta"][live])
        assert np.array_equal(recs["own"][live].astype(np.float64), rep["own_score"][live])  # A(0) = c(0) at unit levels
        # a huge penalty without a cap, order off: one shift for all
        recs, summ = rm.retime(r, s, cues, radius, context, 1 << 20, -1, False)
        assert np.unique(recs["delta"][live]).size <= 1 and not recs["link"].any()
        # order kept: no consecutive pair that was in order ends reversed
        for pq, jq in ((0, -1), (1, 30), (64, 0)):
            recs, _ = rm.retime(r, s, cues, radius, context, pq, jq, True)
            k = np.flatnonzero(live)
            pos = np.clip(recs["start"], 0, s.size) + recs["lag"]
            a, b = k[:-1], k[1:]
            was = pos[b] >= pos[a]
            assert not (was & (pos[b] + recs["delta"][b] < pos[a] + recs["delta"][a])).any()
            assert np.array_equal((recs["flags"][b] & rm.UNORDERED) != 0, ~was)


def test_ties_go_to_the_option_order():
    s = np.zeros(400, np.uint8)
    s[200:210] = 1
    r = np.zeros(400, np.uint8)
    r[160:170] = 1
    r[240:250] = 1
    cues = (np.array([200, 200]), np.array([210, 210]), np.array([0, 0]))
    recs, _ = rm.retime(r, s, cues, 45, 100, 0, -1, True)
    assert recs["delta"].tolist() == [40, 40] and recs["best_delta"].tolist() == [40, 40]
    recs, summ = rm.retime(np.ones(500, np.uint8), s, cues, 6, 100, 3, 10, True)  # constant profiles
    assert not recs["delta"].any() and summ["total"] == summ["own_total"] == summ["best_total"]
    assert recs["flags"].tolist() == [0, rm.ORDER_TIGHT]  # the two cues start together: g = 0 and equal shifts
    with pytest.raises(ValueError):
        rm.retime(r, s, cues, 1025, 0, 0, -1)
    with pytest.raises(ValueError):
        rm.retime(r, s, cues, 5, 0, 0, -2)
