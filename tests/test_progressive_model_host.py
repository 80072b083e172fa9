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
