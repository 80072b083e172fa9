"""Per-piece quality report over a lag range without a GPU: the numpy model tests/cut_report_model.py against brute-force
correlation of every piece at every lag, its records against split_report_model's at [-W+1, W], and the host-side cut
decision (ffsubsync_amd.cut_report) on hand-built piece reports."""
import math

import numpy as np
import pytest

import cut_report_model as crm
import split_report_model as srm
from ffsubsync_amd import _native
from ffsubsync_amd import cut_report as cr
from ffsubsync_amd.split_report import PieceQuality


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


def _offsets(S, k, shifts):
    b = -(-S // k)
    return np.where(np.arange(b) < b // 2, shifts[0], shifts[1]).astype(np.int64)


CASES = [  # (seed, R, S, shifts, K, lag range, levels ref, levels sub)
    (1, 3000, 4096 + 1, (150, -90), 256, (-500, 1200), (0.0, 1.0), (0.0, 1.0)),           # asymmetric; tail of 1 sample
    (2, 2600, 2048 + 33, (-60, 60), 512, (-2081 - 300, 2599 + 400), (-1.0, 2.5), (0.0, 24.0 / 25.0)),  # past both ends
    (3, 1500, 1024 + 17, (30, 30), 256, (30, 30), (0.3, 0.8), (-0.5, 1.25)),              # a one-lag range
    (4, 2000, 1536 + 31, (-700, -650), 512, (-900, -400), (0.0, 1.0), (0.0, 1.0)),        # only negative lags
    (5, 1800, 2048 + 32, (40, 900), 1024, (0, 1799), (0.0, 1.0), (0.0, 1.0)),             # lag_lo = 0, tail of 32
]


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_model_equals_brute_force_at_every_lag_and_piece(case):
    seed, R, S, shifts, k, (lo, hi), r_lv, s_lv = case
    rb, sb = _problem(seed, R, S, shifts)
    offs = np.clip(_offsets(S, k, shifts), lo, hi)
    recs, curves = crm.report(rb, sb, r_lv, s_lv, k, lo, hi, offs, 3, 50)
    assert recs.size == len(crm.pieces_of(offs, k, S)) == len(curves)
    for i, rec in enumerate(recs):
        c = curves[i]
        want = crm.brute_curve(rb, sb, r_lv, s_lv, int(rec["start_sample"]), int(rec["end_sample"]), lo, hi)
        assert c.tobytes() == want.tobytes(), i
        assert rec["n_lags"] == hi - lo + 1
        assert rec["own_score"] == c[int(rec["offset"]) - lo]
        assert bool(rec["flags"] & srm.OWN_NOT_PEAK) == (rec["n_peaks"] == 0 or rec["peak_offset"][0] != rec["offset"])
    assert int(recs[-1]["end_sample"]) == S
    # the run-based n11 of the whole subtitle is the direct count
    n11 = crm.piece_n11(rb, sb, 0, S, lo, hi)
    direct = [int(np.sum(sb[max(0, -d):min(S, R - d)] & rb[max(0, -d) + d:min(S, R - d) + d])) if min(S, R - d) > max(0, -d)
              else 0 for d in range(lo, hi + 1)]
    assert n11.tolist() == direct


@pytest.mark.parametrize("seed,w,p", [(11, 300, 200.0), (12, 700, 0.0), (13, 2500, math.inf), (14, 1, 10.0)])
def test_symmetric_range_equals_the_windowed_report(seed, w, p):
    """At [-W+1, W], given the windowed split's block offsets, every record equals split_report_model's bit for bit."""
    rb, sb = _problem(seed, 4100, 3900, (120, -200), noise=0.3 if p == 0.0 else 0.08)
    k = 256
    (offs, _, _, pieces), want, _ = srm.report(rb, sb, (0.0, 1.0), (0.0, 24.0 / 25.0), k, w, p, 4, 100)
    got, _ = crm.report(rb, sb, (0.0, 1.0), (0.0, 24.0 / 25.0), k, -w + 1, w, offs, 4, 100)
    assert got.tobytes() == want.tobytes()
    if p == 0.0:
        assert len(pieces) >= 3


def test_offsets_outside_the_range_are_refused():
    rb, sb = _problem(3, 1000, 900, (5, 5))
    with pytest.raises(ValueError):
        crm.report(rb, sb, (0.0, 1.0), (0.0, 1.0), 256, 10, 20, np.full(4, 5, np.int64))


def _pq(start, end, psr=20.0, gain_prev=20.0, gain_next=20.0, flat=False, first_block=0):
    flags = _native.QUALITY_FLAT if flat else 0
    std = 0.0 if flat else 1.0
    return PieceQuality(first_block, first_block + 1, start, end, 0, 0.0, 0.0, 0.0, [(psr, 0)], 0.0, std, 100,
                        0.0 if flat else psr, 1.0, gain_prev, gain_next, flags)


def _decide(pieces, psr=10.0, gain=8.0, cov=0.8):
    reasons, verified, supported, coverage = cr.assess_cut(pieces, psr, gain, cov)
    return cr.decide(verified, supported, coverage, cov), reasons, verified, supported, coverage


def test_coverage_is_the_verified_share_of_the_samples():
    pieces = [_pq(0, 600, first_block=0), _pq(600, 700, psr=4.0, first_block=6), _pq(700, 1000, first_block=7)]
    d, reasons, verified, supported, coverage = _decide(pieces)
    assert verified == [True, False, True]
    assert coverage == 900 / 1000
    assert supported == [False, False]  # both breaks touch the unverified piece
    assert d == "cut"  # no break between two consecutive verified pieces: nothing to support
    assert reasons == ["piece 1: psr 4.0 < 10.0"]
    d, reasons, *_ = _decide(pieces, cov=0.95)
    assert d == "untrusted" and reasons[-1] == "coverage 0.900 < 0.950"


def test_breaks_between_verified_pieces_need_both_gains():
    a, b = _pq(0, 500, gain_next=9.0), _pq(500, 1000, gain_prev=7.9, first_block=5)
    d, reasons, verified, supported, _ = _decide([a, b])
    assert verified == [True, True] and supported == [False] and d == "untrusted"
    assert reasons == ["break 0 (block 5): gain 9.0 / 7.9 < 8.0"]
    b.gain_prev = 8.0
    d, reasons, _, supported, _ = _decide([a, b])
    assert supported == [True] and d == "cut" and reasons == []


def test_single_piece_and_flat_pieces():
    assert _decide([_pq(0, 1000)])[0] == "single"
    assert _decide([_pq(0, 1000, psr=9.9)])[0] == "untrusted"
    d, reasons, verified, _, coverage = _decide([_pq(0, 1000, flat=True)])
    assert d == "untrusted" and verified == [False] and coverage == 0.0
    assert reasons[0] == "piece 0: flat correlation (std 0)"
    d, _, verified, _, _ = _decide([_pq(0, 400, flat=True), _pq(400, 1000, first_block=4)], cov=0.5)
    assert verified == [False, True] and d == "cut"
    assert _decide([])[0] == "untrusted"
    # nothing verified is never a cut, even with no coverage bar
    assert _decide([_pq(0, 500, psr=3.0), _pq(500, 1000, psr=2.0, first_block=5)], cov=0.0)[0] == "untrusted"


def test_numpy_thresholds_are_accepted():
    d = cr.assess_cut([_pq(0, 1000)], np.float32(8.0), np.int64(6), np.float32(0.5))
    assert d[1] == [True]


@pytest.mark.parametrize("bad", [dict(min_piece_psr=math.nan), dict(min_gain="8"), dict(min_coverage=1.5),
                                 dict(min_coverage=-0.1), dict(min_coverage=math.nan), dict(min_piece_psr=True),
                                 dict(min_gain=np.float32("nan")), dict(min_coverage=np.bool_(True))])
def test_bad_thresholds_raise(bad):
    args = dict(min_piece_psr=8.0, min_gain=8.0, min_coverage=0.5)
    args.update(bad)
    with pytest.raises(ValueError):
        cr.assess_cut([_pq(0, 10)], **args)


@pytest.mark.parametrize("bad", [dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0), dict(block_samples=300),
                                 dict(split_penalty=-1.0), dict(lag_range=(5, 4)), dict(min_coverage=1.5),
                                 dict(min_gain=math.nan)])
def test_bad_arguments_raise_before_any_native_call(bad, monkeypatch):
    def no_native(*a, **k):
        raise AssertionError("native call")

    monkeypatch.setattr(_native, "require_gpu", no_native)
    monkeypatch.setattr(_native, "load", no_native)
    args = dict(top_k=3, exclusion_samples=300, block_samples=1024, split_penalty=8192.0)
    args.update(bad)
    with pytest.raises(ValueError):
        cr.checked_cut_sync([(np.zeros(10), (np.array([0]), np.array([10 ** 6]), np.zeros(1, np.uint8)))], **args)
    if set(bad) <= {"top_k", "exclusion_samples", "block_samples", "split_penalty"}:
        with pytest.raises(ValueError):
            cr.split_range_report_batch(None, None, args["block_samples"], args["split_penalty"], args["top_k"],
                                        args["exclusion_samples"])
