"""The numpy statement of the progressive alignment (tests/progressive_model.py) against definitions: the incremental n11
against brute force at tiny sizes, the reports against quality_model.report where the lag sets coincide, the stop rule's
restatement, and what tests/progressive_cases.py claims to cover.  No device."""
import math

import numpy as np
import pytest

import progressive_cases as pc
import progressive_model as pm
import quality_model as qm


@pytest.mark.parametrize("S,W,L", [(1, 1, 5), (7, 3, 20), (33, 16, 50), (40, 33, 10), (5, 40, 3), (64, 2, 64)])
def test_incremental_counts_equal_brute_force_however_cut(S, W, L):
    rng = np.random.RandomState(S * 1000 + W * 10 + L)
    s, r = rng.rand(S) < 0.5, rng.rand(L) < 0.5
    for kind in ("once", "ones", "random"):
        slot = pm.Slot([(s, (0.0, 1.0))], (0.0, 1.0), W)
        o = 0
        for n in pc.cut(L, kind, seed=S) if kind != "random" else [0, 1, 0] + [1] * (L - 1):
            slot.append(r[o:o + n])
            o += n
        assert o == L and (slot.n11[0] == pm.n11_brute(r, s, W)).all(), kind
        assert slot.records()[0][0] == pm.report(r, s, (0.0, 1.0), (0.0, 1.0), W)


def test_reports_equal_the_quality_model_where_the_lag_sets_coincide():
    rng = np.random.RandomState(11)
    hits = 0
    for S, W, L in [(700, 33, 100), (700, 33, 34), (33, 33, 900), (32, 33, 900), (5000, 600, 700), (700, 600, 601)]:
        s, r = pc.speech(rng, S), pc.speech(rng, L)
        if not pm.window_is_reference_mask(L, S, W):
            continue
        hits += 1
        for lv_r, lv_s in (((0.0, 1.0), (0.0, 1.0)), ((0.1, 1.0), (0.0, 24 / 25))):
            got, want = pm.report(r, s, lv_r, lv_s, W, 3, 40), qm.report(r, s, lv_r, lv_s, W, 3, 40)
            assert got["n_lags"] == want["n_lags"] == 2 * W and got["flags"] == want["flags"]
            assert got["mean"] == want["mean"] and got["std"] == want["std"]
            for (a, da), (b, db) in zip(got["peaks"], want["peaks"]):
                assert abs(a - b) <= 4 * np.spacing(max(S, L)) and (da == db or lv_s != (0.0, 1.0))
            if lv_s == (0.0, 1.0) and lv_r == (0.0, 1.0):
                assert {k: v for k, v in got.items() if k != "sum_bound"} == want
    assert hits >= 4
    # the sufficient condition of DESIGN 3.22, and two places where the masks differ
    assert all(pm.window_is_reference_mask(L, S, W) for S, W, L in [(700, 33, 34), (32, 33, 40), (5000, 600, 601)])
    assert not pm.window_is_reference_mask(20, 31, 33) and not pm.window_is_reference_mask(0, 700, 33)
    assert not pm.window_is_reference_mask(900, 20, 33)  # (W > S + 1: the reference's slice wraps)


def test_an_empty_prefix_is_flat_zero():
    slot = pm.Slot([(np.ones(5, bool), (0.0, 1.0)), (np.zeros(9, bool), (0.0, 0.96))], (0.1, 1.0), 4)
    reps, st = slot.append(np.zeros(0, bool), 3, 2)
    assert all(rep["flags"] == qm.FLAT and rep["mean"] == 0.0 and rep["std"] == 0.0 and rep["n_lags"] == 8 for rep in reps)
    assert reps[0]["peaks"] == [(0.0, 4), (0.0, 2), (0.0, 0)]  # largest lag on ties, E apart
    assert (st["best_cand"], st["offset"], st["score"], st["other_best"]) == (0, 4, 0.0, 0.0)
    assert pm.derived(st) == (0.0, 0.0, 0.0)
    one = pm.Slot([(np.ones(5, bool), (0.0, 1.0))], (0.0, 1.0), 4).append(np.ones(3, bool), 1, 1)[1]
    assert math.isnan(one["other_best"]) and math.isnan(one["runner_up"]) and pm.derived(one)[1] == math.inf


def _state(cand=2, offset=100, score=10.0, mean=0.0, std=1.0, runner_up=5.0, other_best=9.0, ref_len=1000, flags=0):
    return dict(best_cand=cand, offset=offset, score=score, mean=mean, std=std, runner_up=runner_up, other_best=other_best,
                ref_len=ref_len, flags=flags)


def test_settled_restated_with_each_clause_failing_alone():
    rule = dict(min_psr=5.0, min_margin=3.0, min_ratio_margin=0.5, stable_updates=3, offset_tolerance=2, min_samples=500)
    good = [_state(), _state(offset=102), _state(offset=101)]
    assert pm.settled(good, **rule) and not pm.settled(good[:2], **rule)
    assert not pm.settled(good, **dict(rule, stable_updates=None))
    for bad in (_state(cand=1), _state(offset=98), _state(score=4.9, runner_up=0.0, other_best=0.0), _state(runner_up=7.5),
                _state(other_best=9.6), _state(ref_len=499), _state(flags=qm.FLAT), _state(std=0.0)):
        for at in range(3):
            assert not pm.settled(good[:at] + [bad] + good[at + 1:], **rule), (bad, at)
        assert pm.settled([bad] + good, **rule)  # older than the last three: not looked at
    assert pm.settled([_state(other_best=math.nan, runner_up=math.nan)] * 3, **rule)  # one candidate, one peak


def test_all_eight_sync_seeds_keep_their_distance_from_every_threshold():
    """What lets tests/test_gpu_progressive_sync.py demand the model's stop update exactly: the device's moments differ
    from numpy's by rounding (1e-9 relative at most, as tested), and no decision statistic of any state of these files
    lies within 1e-6 relative of a threshold."""
    assert pc.SYNC_SEEDS == tuple(range(8))
    stops = []
    for seed in pc.SYNC_SEEDS:
        full = pc.sync_model_run(seed, None)
        assert full["updates"] == 6 and not full["settled"] and full["state"]["ref_len"] == 60000
        for i, rule in enumerate(pc.SYNC_RULES):
            assert pm.decision_distance(full["history"], rule) >= 1e-6, (seed, i)
            stops.append(pc.sync_model_run(seed, i)["updates"])
        ref, _, cands, ratios = pc.sync_problem(seed)
        assert len(cands) == len(ratios) == 7 and all(pm.window_is_reference_mask(60000, len(s), pc.SYNC_W) for s, _ in cands)
    assert min(stops) < 6  # some file stops early


def test_the_case_list_covers_what_it_claims():
    cases = pc.total_cases()
    assert {c[1]["ref"].size for c in cases} == set(pc.TOTALS)
    for total in pc.TOTALS:
        kinds = {c[2] for c in cases if c[1]["ref"].size == total}
        assert kinds == (set(pc.CUTS) if total <= 95 else set(pc.CUTS) - {"ones"})
    for name, case, kind, fb in cases:
        cuts = pc.cut(case["ref"].size, kind, seed=len(name))
        assert sum(cuts) == case["ref"].size and min(cuts) >= 0
    assert any(0 in pc.cut(1000, "random", seed=s) for s in range(4))
    both = cases + pc.window_cases()
    assert {c[3] for c in both} == set(pc.FIRST_BITS)
    assert {len(s) for c in both for s, _ in c[1]["cands"]} == set(pc.SUB_LENGTHS)
    assert {c[1]["W"] for c in both} == set(pc.WINDOWS) and {len(c[1]["cands"]) for c in cases} == set(pc.N_CANDS)
    assert {c[1]["ref_levels"] for c in both} == {(0.0, 1.0), (0.1, 1.0)}
    assert {(c[1]["W"], len(c[1]["cands"][0][0])) for c in pc.window_cases()} == {(w, s) for w in pc.WINDOWS for s in pc.SUB_LENGTHS}
    his = {lv[1] for c in both for _, lv in c[1]["cands"]}
    assert 1.0 in his and any(h < 1.0 for h in his)
    assert any(c[1]["W"] > len(c[1]["cands"][0][0]) for c in both) and any(c[1]["W"] > c[1]["ref"].size for c in both)
    assert 2 * max(pc.WINDOWS) > 4096  # crosses a lag tile of k_prog_counts


def _peak_tiles(case, cuts):
    """The tiles of k_prog_counts that hold a model peak of any candidate after the last append."""
    slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])
    o = 0
    for n in cuts:
        reps, _ = slot.append(case["ref"][o:o + n], case["top_k"], case["e"])
        o += n
    return {pc.tile_of(case["W"], lag) for rep in reps for _, lag in rep["peaks"]}


def test_the_tile_cases_cover_what_they_claim():
    cases = pc.tile_cases()
    by_w = {}
    for name, case, cuts, fb in cases:
        assert sum(cuts) == case["ref"].size and min(cuts) >= 0 and case["top_k"] == 8 and fb in pc.FIRST_BITS
        by_w.setdefault(case["W"], []).append((name, case, cuts))
    full = [W for W in by_w if (2 * W) % pc.TILE == 0 and 2 * W < pc.MAX_LAGS]
    plus_two = [W for W in by_w if (2 * W) % pc.TILE == 2]
    assert sorted(by_w) == [2048, 2049, 4096, pc.LIMIT_W] and 2 * pc.LIMIT_W == pc.MAX_LAGS == 64 * pc.TILE
    assert sorted(full) == [2048, 4096] and plus_two == [2049]  # one full tile, two full tiles; a tile and two lags
    for W in pc.TILE_WINDOWS:
        got = {(len(c["cands"][0][0]), c["ref"].size, len(cuts) == 1) for _, c, cuts in by_w[W]}
        assert got == {(S, total, once) for S in pc.TILE_SUB_LENGTHS for total in pc.TILE_TOTALS for once in (True, False)}
    assert {fb for _, _, _, fb in cases} == set(pc.FIRST_BITS)
    name, limit, cuts = by_w[pc.LIMIT_W][0]
    assert cuts == [1000, 1, 1999] and [len(s) for s, _ in limit["cands"]] == [5000, 200000]
    assert limit["ref_levels"] == (0.1, 1.0) and limit["e"] == pc.LIMIT_W // 8
    # for a window of two full tiles, for the one of a tile and two lags and for the limit: a case whose model peaks lie
    # in at least two tiles (2W = 4096 is one tile).  The planted lag is peak 1 and lies where tile_shift says.
    for W, S in ((4096, 5000), (2049, 5000)):
        name, case, cuts = next(x for x in by_w[W] if len(x[1]["cands"][0][0]) == S and len(x[2]) == 1)
        tiles = _peak_tiles(case, cuts)
        assert len(tiles) >= 2 and pc.tile_of(W, pc.tile_shift(W, S, case["ref"].size)) in tiles, (name, tiles)
    assert pc.tile_of(2049, pc.tile_shift(2049, 5000, 1000)) == 1 and pc.tile_of(2049, -2048) == 1 and pc.tile_of(2049, -2046) == 0
    assert pc.tile_of(2048, -2047) == 0 and pc.tile_of(4096, 0) == 1 and pc.tile_of(4096, 1) == 0
    tiles = _peak_tiles(limit, cuts)
    assert len(tiles) >= 2 and max(tiles) >= 33, tiles
    slot_cases, rounds = pc.tile_slot_cases()
    assert [c["W"] for c in slot_cases] == [2048, 4096, 16]
    assert all(sum(r[i] for r in rounds) <= c["ref"].size for i, c in enumerate(slot_cases))
    e2, cuts = pc.tile_e2_case()
    assert e2["W"] == 2048 and sum(cuts) == 2100 == len(e2["cands"][0][0]) and pm.window_is_reference_mask(2100, 2100, 2048)


def test_incremental_counts_equal_brute_force_at_a_full_tile():
    """W = 2048 (2W = one tile of k_prog_counts) at tiny S and L, in three appends."""
    rng = np.random.RandomState(2048)
    s, r = rng.rand(70) < 0.5, rng.rand(90) < 0.5
    slot = pm.Slot([(s, (0.0, 1.0))], (0.0, 1.0), 2048)
    for lo, hi in ((0, 33), (33, 34), (34, 90)):
        slot.append(r[lo:hi], 1, 1)
    assert slot.n11[0].size == 4096 and (slot.n11[0] == pm.n11_brute(r, s, 2048)).all() and slot.n11[0].any()


def _queue_fits():
    cases = pc.queue_cases()
    fed = [0] * len(cases)
    for slots, ns, fb in pc.QUEUE_CALLS:
        assert len(set(slots)) == len(slots) == len(ns) and 0 <= fb < 32
        for s, n in zip(slots, ns):
            fed[s] += n
    return cases, fed


def test_the_queued_sequences_cover_what_they_claim():
    cases, fed = _queue_fits()
    assert len(pc.QUEUE_CALLS) == 8 and len(cases) == 3 and all(f <= c["ref"].size for f, c in zip(fed, cases))
    assert {n for _, ns, _ in pc.QUEUE_CALLS for n in ns} == set(pc.QUEUE_LENGTHS)
    assert len({fb for _, _, fb in pc.QUEUE_CALLS}) == 8  # a different first_bit per call
    orders = {tuple(slots) for slots, _, _ in pc.QUEUE_CALLS}
    assert any(list(o) != sorted(o) for o in orders) and {len(o) for o in orders} == {1, 2, 3}
    assert all(c["W"] <= 600 and c["ref"].size <= 1000 for c in cases + list(pc.reopen_cases()) + [pc.two_stream_case()])
    long, short, _ = pc.reopen_cases()
    assert (len(long["cands"][0][0]), long["W"]) == (5000, 600) and (len(short["cands"][0][0]), short["W"]) == (33, 16)


def test_every_append_of_the_two_stream_sequence_changes_the_answer():
    """Appends k and k + 1 of tests/test_gpu_progressive_streams.py's two-stream test come from different streams with
    nothing but the plan to order them.  If they ran swapped, record k would be the model's of the prefix plus chunk
    k + 1: that differs from the model's record k only if consecutive chunks and consecutive answers differ."""
    case = pc.two_stream_case()
    assert len(pc.TWO_STREAM_LENGTHS) == 10 and sum(pc.TWO_STREAM_LENGTHS) <= case["ref"].size
    slot = pm.Slot(case["cands"], case["ref_levels"], case["W"])

    def answer(reps, st):
        return ([(rep["peaks"], rep["mean"], rep["std"]) for rep in reps],
                {k: repr(v) for k, v in st.items() if k != "ref_len"})

    o, chunks, seen = 0, [], []
    for n in pc.TWO_STREAM_LENGTHS:
        chunks.append(case["ref"][o:o + n])
        seen.append(answer(*slot.append(chunks[-1], case["top_k"], case["e"])))
        o += n
    for k in range(9):
        assert seen[k] != seen[k + 1] and seen[k][0] != seen[k + 1][0], k
        assert chunks[k].tobytes() != chunks[k + 1].tobytes(), k
        # what a swapped pair would leave in record k: the prefix and chunk k + 1
        swapped = pm.Slot(case["cands"], case["ref_levels"], case["W"])
        swapped.append(case["ref"][:sum(pc.TWO_STREAM_LENGTHS[:k])], case["top_k"], case["e"])
        assert answer(*swapped.append(chunks[k + 1], case["top_k"], case["e"])) != seen[k], k
