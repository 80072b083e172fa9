"""The numpy statement of the sampled alignment (tests/sampled_model.py) against definitions: the counts against a
brute-force triple loop at tiny sizes, the scores against the unmodified reference aligner on the 0.5-filled vector,
order / cutting independence (S2) and the prefix case (S3) in the model, the schedule, and what tests/sampled_cases.py
claims to cover.  No device."""
import numpy as np
import pytest

import progressive_cases as pc
import progressive_model as pm
import quality_model as qm
import sampled_cases as sc
import sampled_model as sm
from oracle import aligners_oracle as ao


def _feed(slot, ref, script, top_k=3, e=300):
    out = None
    for a, n, *_ in script:
        out = slot.append_at(a, ref[a:a + n], top_k, e)
    return out


@pytest.mark.parametrize("S,W,T,segs", [(1, 1, 5, [(2, 1)]), (7, 3, 20, [(0, 4), (10, 3), (4, 2)]),
                                        (33, 16, 50, [(49, 1), (0, 33), (40, 5), (33, 7)]), (40, 33, 10, [(3, 4)]),
                                        (5, 40, 200, [(100, 100), (0, 3)]), (64, 2, 64, [(31, 2), (33, 31), (0, 31)]),
                                        (200, 8, 200, [(64, 32), (0, 64), (190, 10), (96, 1)])])
def test_counts_equal_the_brute_force_triple_loop(S, W, T, segs):
    rng = np.random.RandomState(S * 1000 + W * 10 + T)
    s, r = rng.rand(S) < 0.5, rng.rand(T) < 0.5
    slot = sm.Slot([(s, (0.0, 1.0))], (0.0, 1.0), W, T)
    for a, n in segs:
        slot.append_at(a, r[a:a + n], 1, 1)
        want = sm.counts_brute(r, slot.known, s, W)
        assert (slot.counts[0] == want).all(), (a, n)
        assert (sm.counts_direct(r, slot.known, s, W) == want).all(), (a, n)  # what the larger shapes are held to
    assert slot.intervals == sm.merge([(a, a + n) for a, n in segs]) and int(slot.known.sum()) == sum(n for _, n in segs)
    assert slot.records(1, 1)[0][0] == sm.report(r, slot.known, s, (0.0, 1.0), (0.0, 1.0), W, 1, 1)


def _oracle_scores(slot, c, W):
    """The unmodified reference aligner's masked `convolve` entries of the window on the 0.5-filled vector."""
    s, lv = slot.cands[c]
    conv, n_sub = ao.convolve_full(slot.filled(0.5), np.where(s, lv[1], lv[0]))
    masked = ao.mask_extreme_offsets(conv, n_sub, W)
    lags = len(masked) - 1 - np.arange(len(masked)) - n_sub
    keep = np.isfinite(masked)
    order = np.argsort(lags[keep])
    return lags[keep][order], masked[keep][order]


def test_scores_equal_the_reference_aligner_on_the_half_filled_vector():
    """Small shapes where the reference's lag mask is the window, several known sets; then the S4 case of the GPU test
    after every append, with the gap assertion that lets it demand the decision exactly."""
    rng = np.random.RandomState(5)
    for S, W, T, segs in [(700, 33, 800, [(100, 50), (0, 7), (600, 200)]), (300, 16, 310, [(5, 300)]),
                          (64, 8, 100, [(30, 1), (90, 10)])]:
        assert pm.window_is_reference_mask(T, S, W)
        s, r = pc.speech(rng, S), pc.speech(rng, T)
        slot = sm.Slot([(s, (0.0, 24 / 25))], (0.0, 1.0), W, T)
        for a, n in segs:
            slot.append_at(a, r[a:a + n], 1, 1)
            lags, want = _oracle_scores(slot, 0, W)
            n11, n1x, nx1, ov = slot.counts[0]
            got_lags, got, _, slack = sm.scores_from_counts(n11, n1x, nx1, ov, (0.0, 1.0), (0.0, 24 / 25), W)
            assert (lags == got_lags).all()
            assert np.abs(got - want).max() <= slack, (S, W, T, a)
    case, script = sc.s4_case()
    assert case["ref_levels"] == (0.0, 1.0)
    assert all(pm.window_is_reference_mask(case["T"], len(s), case["W"]) for s, _ in case["cands"])
    slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
    for a, n, _ in script:
        _, st = slot.append_at(a, case["ref"][a:a + n], case["top_k"], case["e"])
        gap, (cand, off) = sm.decision_gap(slot)
        assert gap > 0.5, (a, gap)  # no S4 case may be skipped for a tie
        assert (st["best_cand"], st["offset"]) == (cand, off)
        (score, offset), index = ao.max_score_align(slot.filled(0.5), [np.where(s, lv[1], lv[0]) for s, lv in slot.cands],
                                                    case["W"])
        assert (index, offset) == (cand, off) and abs(score - st["score"]) <= slot.slack(cand)


def test_records_do_not_depend_on_order_or_cutting_in_the_model():
    case, segs = sc.s2_case()
    scripts = sc.s2_scripts()
    assert len(scripts) == 6 and len({tuple(s) for s in scripts}) == 6
    seen = []
    for script in scripts:
        slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        reps, st = _feed(slot, case["ref"], script, case["top_k"], case["e"])
        assert slot.intervals == sm.merge(segs)
        seen.append((reps, st, [c.tobytes() for c in slot.counts]))
    assert all(x == seen[0] for x in seen[1:])
    assert sm.merge(segs) == [(0, 130), (500, 640), (1000, 1001), (4000, 5000)]


def test_a_prefix_equals_the_progressive_model():
    case, cuts = sc.s3_case()
    a_slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
    p_slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])
    o = 0
    for n in cuts:
        chunk = case["ref"][o:o + n]
        got, want = a_slot.append_at(o, chunk, case["top_k"], case["e"]), p_slot.append(chunk, case["top_k"], case["e"])
        o += n
        assert got == want, o
    assert o == case["T"] and a_slot.intervals == [(0, o)]


def test_nothing_known_and_nothing_reachable_are_flat_zero():
    case, script = sc.edge_case()
    slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
    reps, st = slot.records(case["top_k"], case["e"])
    assert st["ref_len"] == 0 and all(rep["flags"] == qm.FLAT for rep in reps)
    a, n, _ = script[0]
    assert a >= max(len(s) for s, _ in case["cands"]) + case["W"]  # beyond every subtitle's reach
    reps, st = slot.append_at(a, case["ref"][a:a + n], case["top_k"], case["e"])
    assert case["ref"][a:a + n].any() and st["ref_len"] == n
    for c, rep in enumerate(reps):
        assert not slot.counts[c][3].any() and rep["flags"] == qm.FLAT and (rep["mean"], rep["std"]) == (0.0, 0.0)
        assert all(p[0] == 0.0 for p in rep["peaks"]) and rep["peaks"][0][1] == case["W"]


def test_the_schedule_is_a_spread_permutation_that_tiles_the_reference():
    for total, seg in [(1, 1), (5, 10), (25, 10), (60000, 6000), (360000, 6000), (360001, 6000), (719999, 6000), (64, 1),
                       (1000, 7)]:
        sched = sm.segment_schedule(total, seg)
        flat = sorted(sched)
        assert flat[0][0] == 0 and flat[-1][1] == total and all(x[1] == y[0] for x, y in zip(flat, flat[1:]))
        assert all(b - a == seg for a, b in flat[:-1]) and 0 < flat[-1][1] - flat[-1][0] <= seg
        assert sorted(a // seg for a, _ in sched) == list(range(len(sched)))  # a permutation of the grid
        k = 0
        while 2 ** k <= len(sched):
            head = sorted(sched[:2 ** k])
            edges = [0] + [x for ab in head for x in ab] + [total]
            gaps = [edges[i + 1] - edges[i] for i in range(0, len(edges), 2)]
            assert max(gaps) <= total / 2 ** k + seg, (total, seg, k, max(gaps))
            k += 1
    assert [a // 10 for a, _ in sm.segment_schedule(80, 10)] == [0, 4, 2, 6, 1, 5, 3, 7]  # bit-reversed where n = 2^k
    assert sm.segment_schedule(25, 10)[-1] == (20, 25) or (20, 25) in sm.segment_schedule(25, 10)
    from ffsubsync_amd import sampled

    for total, seg in [(25, 10), (360001, 6000), (64, 1)]:
        assert sampled.segment_schedule(total, seg) == sm.segment_schedule(total, seg)
        assert sampled.prefix_schedule(total, seg) == sorted(sm.segment_schedule(total, seg))
    for bad in [(0, 10), (10, 0), (2.5, 1), (10, 1.5)]:
        with pytest.raises(ValueError):
            sampled.segment_schedule(*bad)


def test_what_the_model_refuses():
    slot = sm.Slot([(np.ones(5, bool), (0.0, 1.0))], (0.0, 1.0), 4, 600)
    slot.append_at(10, np.ones(10, bool))
    assert slot.check(-1, 2) and slot.check(595, 6) and slot.check(19, 1) and slot.check(5, 6) and slot.check(0, 600)
    assert slot.check(20, 5) is None and slot.check(0, 10) is None and slot.check(600, 0) is None and slot.check(15, 0) is None
    lim = sm.Slot([(np.ones(5, bool), (0.0, 1.0))], (0.0, 1.0), 4, 600)
    for k in range(sm.MAX_INTERVALS):
        lim.known[2 * k] = True
        lim.intervals.append((2 * k, 2 * k + 1))
    assert lim.check(512, 1) == "intervals" and lim.check(1, 1) is None and lim.check(511, 1) is None


def test_the_case_lists_cover_what_they_claim():
    shapes = sc.shape_cases()
    assert {2 * c["W"] for _, c, _ in shapes} == set(sc.LAG_COUNTS)
    assert all(3000 <= c["T"] <= 40000 for _, c, _ in shapes)
    assert {fb for _, _, script in shapes for _, _, fb in script} == set(sc.FIRST_BITS)
    for name, case, script in shapes + [("s4", *sc.s4_case()), ("queue", *sc.queue_case())]:
        slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        for a, n, fb in script:
            assert slot.check(a, n) is None, (name, a, n)
            slot.known[a:a + n] = True
            slot.intervals = sm.merge(slot.intervals + [(a, a + n)])
    case, script = sc.edge_case()
    sizes = [n for _, n, _ in script]
    assert {1, 31, 32, 33, 0} <= set(sizes) and script[1][:2] == (0, 1) and script[-1][0] + script[-1][1] == case["T"]
    assert (40, 5) in [x[:2] for x in script] and 40 // 32 == 44 // 32  # inside one word
    at = [x[:2] for x in script]
    assert at.index((10, 30)) > at.index((40, 5)) and (10 + 30 - 1) // 32 == 40 // 32  # in front, sharing its last word
    assert at.index((45, 10)) > at.index((40, 5))  # directly behind
    assert at.index((360, 5)) > max(at.index((355, 5)), at.index((365, 5))) and 355 // 32 == 369 // 32  # fills the hole
    assert case["ref"][401:463].all() and not case["ref"][500:564].any()
    assert len({len(s) for s, _ in case["cands"]}) == 3
    case, script = sc.piece_case()
    assert script[0][1] == sc.PIECE + 1 and script[1][0] + script[1][1] == script[0][0] and script[-1][0] + script[-1][1] == case["T"]
    cases, rounds = sc.slot_cases()
    counts = []
    for i, case in enumerate(cases):
        slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        for rnd in rounds:
            assert slot.check(*rnd[i]) is None
            slot.append_at(rnd[i][0], case["ref"][rnd[i][0]:rnd[i][0] + rnd[i][1]], 1, 1)
        counts.append(len(slot.intervals))
    assert len(set(counts)) == 3, counts
    case, cuts = sc.s3_case()
    assert sum(cuts) == case["T"] and 0 in cuts
    import progressive_model

    for seed in sc.SYNC_SEEDS[:2]:
        ref, _, cands, _ = pc.sync_problem(seed)
        assert ref.size == 60000 and len(sm.segment_schedule(ref.size, sc.SYNC_SEGMENT)) == 10
        assert all(progressive_model.window_is_reference_mask(ref.size, len(s), sc.SYNC_W) for s, _ in cands)


def test_all_eight_sync_seeds_keep_their_distance_from_every_threshold():
    """What lets tests/test_gpu_sampled_sync.py demand the model's stop update exactly (as
    tests/test_progressive_model_host.py argues for the prefix schedule)."""
    stops = []
    for seed in sc.SYNC_SEEDS:
        full = sc.sync_model_run(seed, None)
        assert full["updates"] == 10 and not full["settled"] and full["state"]["ref_len"] == 60000
        for i, rule in enumerate(sc.SYNC_RULES):
            assert pm.decision_distance(full["history"], rule) >= 1e-6, (seed, i)
            stops.append(sc.sync_model_run(seed, i)["updates"])
    assert min(stops) < 10  # some file stops early


# ---- the tile, tie, limit and row-end lists (tests/test_gpu_sampled.py) ------------------------------------------------
TILE_CASES = sc.tile_cases()


def _assert_direct(slot, case, where):
    for c, (s, _) in enumerate(slot.cands):
        assert (slot.counts[c] == sm.counts_direct(case["ref"], slot.known, s, slot.W)).all(), (where, c)


@pytest.mark.parametrize("name,case,script", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_the_incremental_model_equals_the_direct_counts_on_the_tile_lists(name, case, script):
    """``Slot`` adds per interval as the device does; ``counts_direct`` does not.  After every append (the limit window:
    after the last), and the ov curve says which tiles each append reached."""
    W = case["W"]
    slot = sm.Slot(case["cands"], case["ref_levels"], W, case["T"])
    limit = 2 * W == pc.MAX_LAGS
    for a, n, fb in script:
        assert n <= 2000 and slot.check(a, n) is None
        before = [c[3].copy() for c in slot.counts]
        slot.known[a:a + n] = True  # (the counts alone: no records at this size)
        slot.ref[a:a + n] = case["ref"][a:a + n]
        slot.intervals = sm.merge(slot.intervals + [(a, a + n)])
        for c, (s, _) in enumerate(slot.cands):
            slot.counts[c][0] += pm.n11_increment(case["ref"][a:a + n], a, s, W)
            ov, n1x, nx1 = sm.side_increment(a, a + n, slot.ref, s, W)
            slot.counts[c][1:] += np.stack([n1x, nx1, ov])
            grew = np.flatnonzero(slot.counts[c][3] != before[c])  # the lag indices this append touched
            tiles = sorted({pc.tile_of(W, int(d)) for d in pm.window_lags(W)[grew][[0, -1]]}) if grew.size else []
            want = sc.reach_tiles(a, n, len(s), W)
            assert ([] if not want else [want[0], want[-1]] if len(want) > 1 else want) == tiles, (name, a, c)
            r = sc.reach(a, n, len(s), W)
            assert grew.size == (0 if r is None else r[1] - r[0] + 1)
        if not limit:
            _assert_direct(slot, case, (name, a))
    _assert_direct(slot, case, name)
    assert {fb for _, _, fb in script} <= set(sc.FIRST_BITS)


def test_the_tile_lists_cover_what_they_claim():
    cases = {name: (case, script) for name, case, script in TILE_CASES}
    assert len(cases) == 8 and TILE_CASES[-1][0] == "W%d-limit" % pc.LIMIT_W
    assert sorted({2 * c["W"] for c, _ in cases.values()}) == [4096, 4098, 8192, pc.MAX_LAGS]
    planted = {W: set() for W in pc.TILE_WINDOWS}
    for W in pc.TILE_WINDOWS:
        for j in range(2):
            case, script = cases["W%d-%s" % (W, "ab"[j])]
            assert case["T"] == sc.TILE_T and [len(s) for s, _ in case["cands"]] == [33, 5000, case["T"]]
            planted[W] |= set(sc.TILE_PLANTS[W][j])
            assert sc.TILE_PLANTS[W][j][0] >= 0  # the short candidate meets the reference where it is planted
        # every planted lag is the first or the last lag of a tile, and every such lag of the window is planted
        edges = {d for d in range(-W + 1, W + 1)
                 if d in (W, -W + 1) or pc.tile_of(W, d) != pc.tile_of(W, d + 1) or pc.tile_of(W, d) != pc.tile_of(W, d - 1)}
        assert planted[W] == edges, (W, planted[W], edges)
        named = {W, -W + 1} | {d for d in (W - 4095, W - 4096, W - 8191, W - 8192) if -W < d <= W}
        assert edges == named
        script = cases["W%d-a" % W][1]
        segs = [(a, n) for a, n, _ in script]
        reaches = [[sc.reach_tiles(a, n, S, W) for S in sc.TILE_SUB_LENGTHS] for a, n in segs]
        n_tiles = (2 * W + sc.TILE - 1) // sc.TILE
        if 2 * W == 8192:
            assert segs[0] == (0, 1) and all(t == [1] for t in reaches[0])  # 1.: wholly inside tile 1, every candidate
            assert segs[2][0] == 1 and segs[2][0] // 32 == 0  # 3.: abuts it inside word 0
        else:
            assert reaches[0][0] == [] and reaches[0][1] == [0]  # beyond the short subtitle's reach
            assert segs[2][0] == 0  # 3.: at 0
            # no segment can lie wholly in tile 1: it is met at d = b - 1 >= 0, and d >= 0 is tile 0
            assert n_tiles == 1 or pc.tile_of(W, 0) == 0
        a, n = segs[1]
        for S, tiles in zip(sc.TILE_SUB_LENGTHS, reaches[1]):
            if S >= 5000:
                lo, hi = sc.reach(a, n, S, W)
                assert tiles == list(range(n_tiles))  # 2.: straddles e = 4096 where there is one
                assert lo == -W + 1 if W < 4096 else lo <= W - 4096 < W - 4095 <= hi
            else:
                assert tiles == ([0] if 2 * W == 8192 else [])  # (beyond the short subtitle's reach in the narrow windows)
        assert segs[3][0] == a + n and (a + n) % 32 != 0  # 4.: abuts 2. inside a word
        assert segs[4][0] + segs[4][1] == sc.TILE_T  # 5.: the tail
    # the tie case
    case, script = cases["ties-4098"]
    W = case["W"]
    assert (2 * W, case["T"], [len(s) for s, _ in case["cands"]], case["top_k"], case["e"]) == (4098, 9000, [4000], 8, 200)
    assert [(a, a + n) for a, n, _ in script][0] == (5900, 5950) and len(script) == 2
    slot = sm.Slot(case["cands"], case["ref_levels"], W, case["T"])
    a, n, _ = script[0]
    reps, _ = slot.append_at(a, case["ref"][a:a + n], case["top_k"], case["e"])
    lags = pm.window_lags(W)
    assert list(lags[slot.counts[0][3] > 0]) == list(range(sc.TIE_ISLAND[0], sc.TIE_ISLAND[1] + 1))
    peaks = reps[0]["peaks"]
    assert len(peaks) == 8 and peaks[0][0] > 0.0 and sc.TIE_ISLAND[0] <= peaks[0][1] <= sc.TIE_ISLAND[1]
    assert all(p[0] == 0.0 for p in peaks[1:])  # every later peak is picked from the run of exact 0.0 scores
    open_lags = lags[(slot.counts[0][3] == 0) & (np.abs(lags - peaks[0][1]) >= case["e"])]  # the ties of the second pick
    assert (W - open_lags < sc.TILE).any() and (W - open_lags >= sc.TILE).any()  # on both sides of e = 4096
    assert peaks[1][1] == int(open_lags.max())  # ties go to the largest lag
    a, n, _ = script[1]
    reps, _ = slot.append_at(a, case["ref"][a:a + n], case["top_k"], case["e"])
    got = lags[slot.counts[0][3] > 0]
    assert list(got) == list(range(-W + 1, 50)) + list(range(sc.TIE_ISLAND[0], sc.TIE_ISLAND[1] + 1))  # a second island
    assert any(p[1] < 50 for p in reps[0]["peaks"])  # and a peak is taken from it
    # the limit
    case, script = cases["W%d-limit" % pc.LIMIT_W]
    W = case["W"]
    assert 2 * W == pc.MAX_LAGS and case["T"] == 3000 and [len(s) for s, _ in case["cands"]] == list(pc.LIMIT_SUB_LENGTHS)
    assert sorted(n for _, n, _ in script) == sorted(pc.LIMIT_CUTS) and [a for a, _, _ in script] != sorted(a for a, _, _ in script)
    assert sm.merge([(a, a + n) for a, n, _ in script]) == [(0, 3000)]
    first = min(min(sc.reach_tiles(a, n, 200000, W)) for a, n, _ in script)
    reached = set().union(*[sc.reach_tiles(a, n, 200000, W) for a, n, _ in script])
    assert first == 31 and len(reached) >= 30 and max(reached) == 63
    known = np.ones(3000, bool)
    ov = sm.counts_direct(case["ref"], known, case["cands"][1][0], W)[3]
    e = W - pm.window_lags(W)
    assert not ov[e < first * sc.TILE].any() and all(ov[e // sc.TILE == k].any() for k in reached)


def test_the_row_end_and_the_three_window_lists_cover_what_they_claim():
    assert [T % 32 for T in sc.ROW_END_TOTALS] == [0, 1, 31] and all((T // 32 + 2) % 16 == 0 for T in sc.ROW_END_TOTALS)
    for T, cases, steps in sc.row_end_cases():
        assert all(c["T"] == T for c in cases)
        slots = [sm.Slot(c["cands"], c["ref_levels"], c["W"], T) for c in cases]
        for s, a, n, fb in steps:
            assert slots[s].check(a, n) is None
            slots[s].known[a:a + n] = True
            slots[s].intervals = sm.merge(slots[s].intervals + [(a, a + n)])
        order = [(s, a, a + n) for s, a, n, _ in steps]
        zero = [i for i, x in enumerate(order) if x[0] == 0]
        assert order[zero[0]][2] == T and order[zero[1]][1] == 0 and cases[0]["ref"][T - 40:].all()
        one = [i for i, x in enumerate(order) if x[0] == 1]
        assert one[0] < zero[0] and one[-1] > zero[-1] and slots[1].intervals == [(0, 100), (T - 1, T)]
    cases, rounds = sc.tile_slot_cases()
    assert [k["W"] for k in cases] == [2048, 4096, 16]
    for i, case in enumerate(cases):
        slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
        for rnd in rounds:
            assert slot.check(*rnd[i]) is None
            slot.known[rnd[i][0]:sum(rnd[i])] = True
    assert sc.reach_tiles(1, 300, 5000, 4096) == [0, 1]  # the widest slot works in both tiles in one call


# ---- the stream sequences (tests/test_gpu_sampled_streams.py) ----------------------------------------------------------
def _reports(slot, a, chunk):
    """The candidate reports alone: the state's ref_len would tell two calls apart whatever they fed."""
    return slot.append_at(a, chunk, 3, 40)[0]


def _calls_of_slot(case, segs):
    """The reports after each segment of ``segs`` fed in order."""
    slot = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"])
    return [_reports(slot, a, case["ref"][a:a + n]) for a, n in segs]


def _every_call_is_visible(case, segs, where):
    """Every non-empty call changes the reports; swapping two adjacent calls changes the reports of one of the two."""
    seen = _calls_of_slot(case, segs)
    start = sm.Slot(case["cands"], case["ref_levels"], case["W"], case["T"]).records(3, 40)[0]
    for k, (a, n) in enumerate(segs):
        prev = seen[k - 1] if k else start
        assert (seen[k] != prev) == (n > 0), (where, k, a, n)
    for k in range(len(segs) - 1):
        if segs[k][1] == 0 and segs[k + 1][1] == 0:
            continue
        swapped = list(segs)
        swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
        other = _calls_of_slot(case, swapped)
        assert other[k] != seen[k] or other[k + 1] != seen[k + 1], (where, "swap", k)
        assert other[k + 1] == seen[k + 1]  # (the pair's union is the same: order-independent)


def test_every_call_of_the_stream_sequences_is_visible_in_the_records():
    cases = sc.queue_cases()
    assert len(cases) == 3 and len(sc.QUEUE_CALLS) == 8 and 2 * cases[1]["W"] == 4098
    per_slot = {0: [], 1: [], 2: []}
    for slots, segs, fb in sc.QUEUE_CALLS:
        assert len(set(slots)) == len(slots) == len(segs) and 0 <= fb < 32
        for s, seg in zip(slots, segs):
            per_slot[s].append(seg)
    assert len({tuple(slots) for slots, _, _ in sc.QUEUE_CALLS}) == 8  # another subset or order each call
    lengths = [n for segs in per_slot.values() for _, n in segs]
    assert set(lengths) == set(sc.QUEUE_LENGTHS) and lengths.count(0) == 2
    for s, segs in per_slot.items():
        fed = [x for x in segs if x[1]]
        assert all(a + n == prev for (a, n), (prev, _) in zip(fed[1:], fed))  # back to front, each abutting the last
        _every_call_is_visible(cases[s], segs, ("queue", s))
    assert sum(per_slot[1][0]) == cases[1]["T"]
    assert all(sc.reach_tiles(a, n, 5000, cases[1]["W"]) == [0, 1] for a, n in per_slot[1] if n)  # a queued call runs two tiles
    case = sc.two_stream_case()
    assert len(sc.TWO_STREAM_SEGMENTS) == 10 and all(n > 0 for _, n in sc.TWO_STREAM_SEGMENTS)
    assert [a for a, _ in sc.TWO_STREAM_SEGMENTS] != sorted(a for a, _ in sc.TWO_STREAM_SEGMENTS)
    _every_call_is_visible(case, list(sc.TWO_STREAM_SEGMENTS), "two streams")
    prefix, sampled = sc.mixed_case()
    assert len(sc.MIXED_LENGTHS) == len(sc.MIXED_SEGMENTS) == 6 and sum(sc.MIXED_LENGTHS) <= prefix["ref"].size
    assert prefix["W"] == sampled["W"] and [len(s) for s, _ in prefix["cands"]] == [len(s) for s, _ in sampled["cands"]]
    _every_call_is_visible(sampled, list(sc.MIXED_SEGMENTS), "mixed")
    slot, seen = pm.Slot(prefix["cands"], prefix["ref_levels"], prefix["W"]), []
    o = 0
    for n in sc.MIXED_LENGTHS:
        seen.append(slot.append(prefix["ref"][o:o + n], 3, 40)[0])
        o += n
    assert all(x != y for x, y in zip(seen, seen[1:]))
    chain = sc.reopen_chain()
    assert [k for k, _, _ in chain] == ["sampled", "prefix", "sampled", "sampled"]
    (_, c, _), (_, d, _) = chain[2:]
    assert d["T"] < c["T"] and d["W"] < c["W"] and len(d["cands"]) < len(c["cands"])
    for kind, case, appends in chain:
        if kind == "sampled":
            _every_call_is_visible(case, appends, ("chain", case["T"]))
        else:
            assert sum(appends) == case["ref"].size
    case, segs = sc.late_case()
    _every_call_is_visible(case, segs, "late")
