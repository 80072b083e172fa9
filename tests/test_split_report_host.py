"""Per-piece quality report of a split solve without a GPU: the numpy model's piece curves against brute-force
correlation of each piece's slice, its moments, the host-side derivation and decision rules, the separation of the
synthetic classes at the default thresholds, and host-side validation."""
import json
import math
import os

import numpy as np
import pytest

import split_model as sm
import split_report_model as srm
from ffsubsync_amd import _native
from ffsubsync_amd import split_report as sr
from workloads import splits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(seed, R, S, shifts, noise=0.08):
    """0/1 vectors: the subtitle follows the reference at shifts[0] up to a cut, then at shifts[1]."""
    rng = np.random.RandomState(seed)
    seg = np.maximum(1, rng.geometric(1.0 / 40.0, size=R // 10 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    cut = S // 2
    idx = np.arange(S) + np.where(np.arange(S) < cut, shifts[0], shifts[1])
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < noise
    return rb, sb


CASES = [  # (seed, R, S, shifts, K, W, P, levels ref, levels sub)
    (1, 3000, 4100, (150, -90), 256, 400, 300.0, (0.0, 1.0), (0.0, 1.0)),          # R < S, S not a multiple of K
    (2, 5200, 2900, (-60, 60), 512, 700, 100.0, (-1.0, 2.5), (0.0, 24.0 / 25.0)),  # R > S, non-default levels
    (3, 1500, 1700, (30, 30), 256, 2500, 50.0, (0.3, 0.8), (-0.5, 1.25)),          # window past both ends
    (4, 2600, 2300, (10, 200), 256, 300, 0.0, (0.0, 1.0), (0.0, 1.0)),             # P = 0
    (5, 2600, 2300, (10, 200), 256, 300, math.inf, (0.0, 1.0), (0.0, 1.0)),        # P = inf: one piece
    (6, 2000, 2050, (-5, -5), 1024, 1, 10.0, (0.0, 1.0), (0.0, 1.0)),              # W = 1
]


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_piece_curves_equal_brute_force_correlation(case):
    seed, R, S, shifts, k, w, p, r_lv, s_lv = case
    rb, sb = _problem(seed, R, S, shifts, noise=0.3 if p == 0.0 else 0.08)
    (offs, _, _, pieces), recs, curves = srm.report(rb, sb, r_lv, s_lv, k, w, p, 3, 50)
    if p == math.inf:
        assert len(pieces) == 1
    if p == 0.0:
        assert len(pieces) >= 3
    assert len(curves) == len(pieces) == recs.size
    for (f, e, lo, hi, off, _), c, rec in zip(pieces, curves, recs):
        want = srm.brute_curve(rb, sb, r_lv, s_lv, w, lo, hi)
        assert c.tobytes() == want.tobytes(), (f, e)
        assert rec["own_score"] == c[off + w - 1]
    # one piece spanning everything: the n11 sum of every block is the whole-vector correlation
    n11 = sm.block_counts(rb, sb, k, w).sum(axis=0)
    whole = srm.piece_curve(rb, sb, r_lv, s_lv, k, w, 0, S, n11)
    assert whole.tobytes() == srm.brute_curve(rb, sb, r_lv, s_lv, w, 0, S).tobytes()


def test_neighbour_scores_and_flags():
    rb, sb = _problem(11, 6000, 5000, (100, -250))
    (offs, _, _, pieces), recs, curves = srm.report(rb, sb, (0.0, 1.0), (0.0, 1.0), 512, 600, 200.0, 4, 100)
    assert len(pieces) >= 2
    assert math.isnan(recs[0]["prev_score"]) and math.isnan(recs[-1]["next_score"])
    for i in range(len(pieces) - 1):
        assert recs[i]["next_score"] == curves[i][pieces[i + 1][4] + 599]
        assert recs[i + 1]["prev_score"] == curves[i + 1][pieces[i][4] + 599]
    for rec in recs:
        assert bool(rec["flags"] & srm.OWN_NOT_PEAK) == (rec["peak_offset"][0] != rec["offset"])


def test_model_moments_are_the_population_moments():
    rng = np.random.RandomState(2)
    for n in (2, 63, 1024, 1025, 5000, 120000):
        c = rng.randn(n) * 300 + 17
        mean, std, flags = srm.moments(c)
        assert flags == 0
        assert abs(mean - c.mean()) <= 1e-12 * abs(c).max() and abs(std - c.std()) <= 1e-12 * c.std()
    mean, std, flags = srm.moments(np.full(10, 2.5))
    assert (mean, std, flags) == (2.5, 0.0, srm.FLAT)


def _rec(**kw):
    r = np.zeros(1, dtype=_native.PIECE_REPORT_DTYPE)[0]
    r["n_lags"], r["n_peaks"] = 100, 2
    r["prev_score"] = r["next_score"] = np.nan
    for k, v in kw.items():
        r[k] = v
    return r


def test_host_derivation_and_decision_rules():
    a = sr.from_record(_rec(offset=5, own_score=100.0, next_score=20.0, mean=10.0, std=5.0,
                            peak_score=[100.0, 60.0] + [0.0] * 6, peak_offset=[5, 90] + [0] * 6))
    b = sr.from_record(_rec(offset=90, own_score=80.0, prev_score=50.0, mean=0.0, std=2.0,
                            peak_score=[80.0, 10.0] + [0.0] * 6, peak_offset=[90, 5] + [0] * 6))
    assert (a.psr, a.margin, a.gain_next) == (18.0, 8.0, 16.0) and math.isnan(a.gain_prev)
    assert (b.psr, b.gain_prev) == (40.0, 15.0) and math.isnan(b.gain_next)
    assert a.own_is_peak and b.own_is_peak
    assert sr.break_support([a, b], 15.0) == [True] and sr.break_support([a, b], 15.5) == [False]
    assert sr.assess_split([a, b], 8.0, 8.0) == []
    reasons = sr.assess_split([a, b], 20.0, 16.0)
    assert reasons == ["piece 0: psr 18.0 < 20.0", "break 0 (block 0): gain 16.0 / 15.0 < 16.0"]
    flat = sr.from_record(_rec(offset=0, own_score=3.0, mean=3.0, std=0.0, flags=srm.FLAT))
    assert flat.flat and flat.psr == 0.0 and sr.assess_split([flat]) == ["piece 0: flat correlation (std 0)"]


def test_calibration_separates_the_classes_at_the_defaults():
    """The committed calibration run (profiles/split_report_calibration.py): every recovered true break supported and
    every piece of those problems above min_piece_psr; no spurious break of a clean problem at P = 1000, no piece more
    than 10 samples off its true offset above min_piece_psr, and no break or
    piece of a wrong pair passes.  The one split problem the DP does not recover (a spurious extra piece at the default
    penalty) is flagged too."""
    d = json.load(open(os.path.join(ROOT, "profiles", "split_report_calibration.json")))
    g, t = sr.DEFAULT_MIN_GAIN, sr.DEFAULT_MIN_PIECE_PSR
    rows = d["rows"]
    assert len([r for r in rows if r["cls"] == "split"]) == 64
    for r in rows:
        ok = all(x >= t for x in r["psr"]) and all(x >= g for x in r["break_gain"])
        if r["cls"] == "split":
            assert ok == r["recovered"], r["seed"]
        elif r["cls"] == "clean_lowP":
            assert not any(x >= g for x in r["break_gain"]), r["seed"]
            spurious = [p for p, o in zip(r["psr"], r["offsets"]) if abs(o - r["truth_offsets"][0]) > 10]
            assert all(p < t for p in spurious), r["seed"]
        else:
            assert not ok and not any(x >= g for x in r["break_gain"]), (r["duration_s"], r["seed"])


def test_separation_on_a_few_live_problems():
    """The same verdicts recomputed on the model: 10 min clean problems at P = 1000 and wrong pairs at the defaults."""
    w, k = 60000, 1024
    for seed in (0, 49, 57):
        pr = splits.make_problem(seed, duration_s=600.0, clean=True)
        _, recs, _ = srm.report(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), k, w, 1000.0)
        pq = [sr.from_record(x) for x in recs]
        assert not any(sr.break_support(pq))
        assert all(q.psr < sr.DEFAULT_MIN_PIECE_PSR for q in pq if abs(q.offset - pr.offsets[0]) > 10)
    for seed in (0, 1):
        a = splits.make_problem(seed, duration_s=600.0, clean=True)
        b = splits.make_problem(seed + 1, duration_s=600.0, clean=True)
        _, recs, _ = srm.report(b.ref, a.sub, (0.0, 1.0), (0.0, a.sub_hi), k, w, sr.DEFAULT_SPLIT_PENALTY)
        assert sr.assess_split([sr.from_record(x) for x in recs])


def test_host_side_checks_raise_before_any_native_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native call")

    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    monkeypatch.setattr(sr, "solve_ratios", boom)
    bad = [dict(block_samples=300), dict(max_offset_samples=0), dict(split_penalty=-1.0), dict(split_penalty=math.nan),
           dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0), dict(top_k=2.5)]
    for kw in bad:
        args = dict(max_offset_samples=100, block_samples=1024, split_penalty=10.0, top_k=3, exclusion_samples=300)
        args.update(kw)
        with pytest.raises(ValueError):
            sr.split_report_batch(object(), **args)
        sync = dict(args)
        sync.pop("max_offset_samples")
        if "max_offset_samples" not in kw:
            with pytest.raises(ValueError):
                sr.checked_split_sync([], **sync)
    with pytest.raises(ValueError):
        sr.checked_split_sync([], max_offset_seconds=0.0)
