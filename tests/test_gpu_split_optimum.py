"""The split aligners on the device against the independent piece-structure reference (tests/piecewise_reference.py),
not against their step-for-step models: ffs_align_split_batch and ffs_align_split_range_batch reach best[B], every piece
sits at the maximum of its own slice, the records hold together, and the documented edges hold -- one piece at the
largest maximising lag for P = inf and DBL_MAX, -0.0 as 0, the exact tie penalty.  The shapes are the ones no other
device test reaches: K that are not powers of two and K = 32 768, tail blocks of 1 to 33 samples, W = 1 and
2W = 262 144, one-lag ranges, ranges without overlap and a range of more than 262 144 lags; U1 and U8 inputs.  The
per-piece report is held to the same reference, and break refinement to its model at the new K."""
import math
import sys

import numpy as np
import pytest

import piecewise_reference as pw
import split_refine_model as rm

pytestmark = pytest.mark.gpu

DBL_MAX = sys.float_info.max
I0, I1 = (0.0, 1.0), (-1.0, 2.5)  # integer mapped levels: (-1, 1), (-3, 4)
F = (0.0, 24.0 / 25.0)  # the tolerance path
PENALTIES = [0.0, -0.0, 0.5, 3.0, 60.0, 8192.0, DBL_MAX, math.inf]

# window aligner: (K, W, pairs_in_flight, [(R, S, reference levels, subtitle levels)]) -- one call per group and penalty
WINDOW_GROUPS = [
    (256, 1, 2, [(900, 100, I0, I0), (2000, 768, I1, I0), (300, 1025, I0, I1), (5000, 1200, I1, F)]),
    (288, 2, None, [(3000, 288 * 5 + 31, I0, I0), (200, 900, I1, I1)]),
    (288, 31, 2, [(4000, 288 * 3 + 33, I0, I1), (1000, 288 * 2, I1, I0), (600, 2000, I0, F)]),
    (800, 32, None, [(9000, 800 * 4 + 1, I1, I1), (700, 3000, I0, I0)]),
    (800, 33, None, [(5000, 400, I0, I1), (20000, 800 * 6 + 31, I1, I0)]),
    (1024, 1000, 3, [(20000, 1024 * 8, I0, I0), (6000, 1024 * 7 + 33, I1, I0), (500, 3000, I0, I1),
                     (80000, 5000, I1, I1), (9000, 6000, I0, F)]),
    (2080, 131072, None, [(300000, 2080 * 4 + 33, I0, I0), (5000, 2080 * 3 + 1, I1, I0)]),
    (32768, 1000, None, [(120000, 32768 * 2 + 31, I0, I1), (70000, 32768 + 1, I1, F)]),
    (32768, 131072, None, [(200000, 32768 * 2 + 1, I0, I0)]),
]

FULL = "full"
# range aligner: (K, pairs_in_flight, [(R, S, reference levels, subtitle levels, (lag_lo, lag_hi) or FULL)])
RANGE_GROUPS = [
    (256, 2, [(2000, 700, I0, I0, (37, 37)), (3000, 1025, I1, I0, (100, 2100)), (1500, 800, I0, I1, (-3000, -5)),
              (900, 600, I1, I1, (910, 1400)), (1200, 1000, I0, F, FULL), (2500, 1300, I1, I1, (-40, -40))]),
    (288, None, [(4000, 288 * 3 + 31, I1, I1, (-500, 3000)), (250, 288 * 2 + 33, I0, I0, FULL)]),
    (800, None, [(280000, 3000, I0, I0, FULL)]),  # 282 999 lags: one row over 139 workgroups
    (1024, 3, [(20000, 1024 * 5 + 1, I0, I1, (-2000, 6000)), (7000, 4000, I1, I0, FULL), (500, 2500, I0, I0, FULL),
               (10000, 3000, I1, I1, (1, 1)), (3000, 1024 * 2, I0, I1, (-9000, -6000))]),
    (2080, None, [(50000, 2080 * 3 + 33, I0, I0, (-4000, 40000))]),
    (32768, None, [(100000, 32768 * 2 + 31, I0, I1, (-1000, 40000))]),
]


def _make_pair(seed, R, S, r_lv, s_lv, lo, hi):
    rng = np.random.RandomState(seed)
    d0 = int(rng.randint(lo, hi + 1))
    d1 = int(np.clip(d0 + rng.randint(-300, 301), lo, hi))
    rb, sb = pw.two_offset_bits(rng, R, S, (d0, d1), flip=0.04)
    return dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, ref=np.where(rb, r_lv[1], r_lv[0]),
                sub=np.where(sb, s_lv[1], s_lv[0]), lo=lo, hi=hi)


def _window_pairs(gi):
    k, w, _, specs = WINDOW_GROUPS[gi]
    return [_make_pair(8000 + 100 * gi + i, R, S, r_lv, s_lv, -w + 1, w) for i, (R, S, r_lv, s_lv) in enumerate(specs)]


def _range_pairs(gi):
    k, _, specs = RANGE_GROUPS[gi]
    out = []
    for i, (R, S, r_lv, s_lv, rng_) in enumerate(specs):
        lo, hi = (-(S - 1), R - 1) if rng_ == FULL else rng_
        out.append(_make_pair(9000 + 100 * gi + i, R, S, r_lv, s_lv, lo, hi))
    return out


def _device_pairs(pairs, packed=True):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    return batch.pack_pairs([(DeviceRaster.from_host(p["ref"], lists=False),
                              [DeviceRaster.from_host(p["sub"], lists=False)]) for p in pairs], packed=packed)


def _reference(pr, k):
    return pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])


def _record_bytes(res):
    return (res.block_offsets.tobytes(), res.block_scores.tobytes(), np.float64(res.total).tobytes())


def _check_group(name, refs, results_by_p, ties):
    """Checks 1-7 of one group: ``results_by_p`` maps each of PENALTIES (by index) to the call's SplitResults, ``ties``
    the per-pair (tie penalty, SplitResult) of a call at that penalty, or None."""
    bad = []
    for pi, p in enumerate(PENALTIES):
        for i, (ref, res) in enumerate(zip(refs, results_by_p[pi])):
            probs = pw.check_solution(ref, p, res.block_offsets, res.total, res.block_scores,
                                      [(q.first_block, q.end_block, q.offset, q.score) for q in res.pieces])
            if probs:
                bad.append((name, i, p, probs[:3]))
    inf_i, max_i, zero_i, nzero_i = len(PENALTIES) - 1, len(PENALTIES) - 2, 0, 1
    assert PENALTIES[inf_i] == math.inf and PENALTIES[max_i] == DBL_MAX and math.copysign(1, PENALTIES[nzero_i]) < 0
    for i, ref in enumerate(refs):
        res = results_by_p[inf_i][i]
        whole = ref.interval(0, ref.B)
        top = float(whole.max())
        tol = ref.tolerance(math.inf)
        want = ref.lo + int(np.flatnonzero(whole >= top - tol)[-1]) if not ref.exact else \
            ref.lo + int(np.flatnonzero(whole == top)[-1])
        if len(res.pieces) != 1 or (ref.exact and res.pieces[0].offset != want) or \
                not abs(ref.at(0, ref.B, res.pieces[0].offset) - top) <= tol:
            bad.append((name, i, "P = inf", [(q.offset, q.score) for q in res.pieces], want, top))
        if _record_bytes(results_by_p[max_i][i]) != _record_bytes(res):
            bad.append((name, i, "P = DBL_MAX differs from P = inf"))
        if _record_bytes(results_by_p[nzero_i][i]) != _record_bytes(results_by_p[zero_i][i]):
            bad.append((name, i, "P = -0.0 differs from P = 0"))
    for i, tie in enumerate(ties):
        if tie is None:
            continue
        p, res = tie
        probs = pw.check_solution(refs[i], p, res.block_offsets, res.total, res.block_scores)
        if probs:
            bad.append((name, i, "tie P = %r" % p, probs[:3]))
    return bad


def test_window_aligner_reaches_the_optimum():
    from ffsubsync_amd import split_align as sa

    bad, n_multi, n_ties, n_checked = [], 0, 0, 0
    for gi, (k, w, pif, _) in enumerate(WINDOW_GROUPS):
        pairs = _window_pairs(gi)
        refs = [_reference(pr, k) for pr in pairs]
        db = _device_pairs(pairs)
        by_p = [sa.split_align_batch(db, w, k, p, pairs_in_flight=pif) for p in PENALTIES]
        u8 = sa.split_align_batch(_device_pairs(pairs, packed=False), w, k, 60.0, pairs_in_flight=pif)
        for i, (a, b) in enumerate(zip(u8, by_p[PENALTIES.index(60.0)])):
            if _record_bytes(a) != _record_bytes(b):
                bad.append((k, w, i, "U8 records differ from U1"))
        ties = []
        for i, (pr, ref) in enumerate(zip(pairs, refs)):
            p = pw.tie_penalty(ref) if ref.exact else None
            ties.append(None if p is None else (p, sa.split_align_batch(_device_pairs([pr]), w, k, p)[0]))
        bad += _check_group("window K=%d W=%d" % (k, w), refs, by_p, ties)
        n_multi += sum(len(r.pieces) > 1 for res in by_p for r in res)
        n_ties += sum(t is not None for t in ties)
        n_checked += len(pairs) * len(PENALTIES)
    assert not bad, bad[:5]
    assert n_multi >= 40 and n_ties >= 5, (n_multi, n_ties, n_checked)


def test_range_aligner_reaches_the_optimum():
    from ffsubsync_amd import cut_align as ca

    bad, n_multi, n_ties = [], 0, 0
    assert any(pr["hi"] - pr["lo"] + 1 > 262144 for gi in range(len(RANGE_GROUPS)) for pr in _range_pairs(gi))
    for gi, (k, pif, _) in enumerate(RANGE_GROUPS):
        pairs = _range_pairs(gi)
        ranges = [(pr["lo"], pr["hi"]) for pr in pairs]
        refs = [_reference(pr, k) for pr in pairs]
        db = _device_pairs(pairs)
        by_p = [ca.split_align_range_batch(db, ranges, k, p, pairs_in_flight=pif) for p in PENALTIES]
        u8 = ca.split_align_range_batch(_device_pairs(pairs, packed=False), ranges, k, 60.0, pairs_in_flight=pif)
        for i, (a, b) in enumerate(zip(u8, by_p[PENALTIES.index(60.0)])):
            if _record_bytes(a) != _record_bytes(b):
                bad.append((k, i, "U8 records differ from U1"))
        ties = []
        for i, (pr, ref) in enumerate(zip(pairs, refs)):
            p = pw.tie_penalty(ref) if ref.exact else None
            one = None if p is None else ca.split_align_range_batch(_device_pairs([pr]), [ranges[i]], k, p)[0]
            ties.append(None if p is None else (p, one))
        bad += _check_group("range K=%d" % k, refs, by_p, ties)
        n_multi += sum(len(r.pieces) > 1 for res in by_p for r in res)
        n_ties += sum(t is not None for t in ties)
    ca.clear_plan_cache()
    assert not bad, bad[:5]
    assert n_multi >= 30 and n_ties >= 4, (n_multi, n_ties)


def _moments(curve):
    n = curve.size
    mean = math.fsum(curve) / n
    return mean, math.sqrt(math.fsum((curve - mean) ** 2) / n)


def test_piece_report_against_the_reference():
    """Integer-level window pairs at P = 3 and 60: per piece own_score == peaks[0] == M(a, c), prev / next scores ==
    I(a, c) at the neighbours' offsets, n_lags == 2W, mean and std within 1e-12 of the curve's population moments."""
    from ffsubsync_amd import split_report as sr

    bad, n_pieces, n_neigh = [], 0, 0
    for gi, (k, w, pif, _) in enumerate(WINDOW_GROUPS):
        pairs = [pr for pr in _window_pairs(gi) if pw.integer_levels(pr["r_lv"], pr["s_lv"])]
        if not pairs:
            continue
        refs = [_reference(pr, k) for pr in pairs]
        db = _device_pairs(pairs)
        for p in (3.0, 60.0):
            res, recs, counts = sr.split_report_batch(db, w, k, p, 4, 50, pairs_in_flight=pif, raw=True)
            for i, ref in enumerate(refs):
                pieces = pw.pieces_of(res[i].block_offsets)
                got = recs[i, :int(counts[i])]
                if len(got) != len(pieces):
                    bad.append((k, w, p, i, "piece count", len(got), len(pieces)))
                    continue
                for j, ((a, c, o), rec) in enumerate(zip(pieces, got)):
                    curve = ref.interval(a, c)
                    m = float(ref.M[a, c])
                    mean, std = _moments(curve)
                    want_prev = ref.at(a, c, pieces[j - 1][2]) if j > 0 else math.nan
                    want_next = ref.at(a, c, pieces[j + 1][2]) if j + 1 < len(pieces) else math.nan
                    scale = max(abs(mean), std)
                    ok = (int(rec["offset"]) == o and float(rec["own_score"]) == m == float(rec["peak_score"][0])
                          and np.array_equal(np.float64(rec["prev_score"]), np.float64(want_prev), equal_nan=True)
                          and np.array_equal(np.float64(rec["next_score"]), np.float64(want_next), equal_nan=True)
                          and int(rec["n_lags"]) == 2 * w
                          and abs(float(rec["mean"]) - mean) <= 1e-12 * scale
                          and abs(float(rec["std"]) - std) <= 1e-12 * scale)
                    n_pieces += 1
                    n_neigh += j > 0
                    if not ok:
                        bad.append((k, w, p, i, j, (a, c, o), float(rec["own_score"]), m, float(rec["peak_score"][0]),
                                    float(rec["mean"]), mean, float(rec["std"]), std))
    assert not bad, bad[:5]
    assert n_pieces >= 40 and n_neigh >= 15, (n_pieces, n_neigh)


@pytest.mark.parametrize("k", [288, 800, 2080, 32768])
def test_refine_at_new_block_lengths_equals_the_model(k):
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_refine as sr

    pairs = []
    for i, (nb, tail) in enumerate([(6, 0), (5, 1), (4, 31), (3, 33)]):
        rng = np.random.RandomState(9500 + 10 * k + i)
        S = nb * k + tail
        d0 = int(rng.randint(-1500, 1500))
        d1 = d0 + int(rng.choice([-1, 1])) * int(rng.randint(200, 900))
        rb, sb = pw.two_offset_bits(rng, S + 6000, S, (d0, d1), flip=0.03, cut=int(rng.randint(k, S - k // 2)))
        lv = [(I0, I0), (I1, I0), (I0, F), (I1, I1)][i]
        pairs.append(dict(rb=rb, sb=sb, r_lv=lv[0], s_lv=lv[1], ref=np.where(rb, lv[0][1], lv[0][0]),
                          sub=np.where(sb, lv[1][1], lv[1][0])))
    db = _device_pairs(pairs)
    res = sa.split_align_batch(db, 2000, k, 60.0, pairs_in_flight=2)
    recs, counts = sr.refine_breaks_batch(db, res, k, sr.DEFAULT_RADIUS_SAMPLES, sr.DEFAULT_UNMATCHED_MARGIN, raw=True)
    n_breaks = 0
    for i, pr in enumerate(pairs):
        want = rm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], res[i].block_offsets, k, sr.DEFAULT_RADIUS_SAMPLES,
                         sr.DEFAULT_UNMATCHED_MARGIN)
        got = recs[i, :int(counts[i])]
        n_breaks += len(want)
        assert got.shape == want.shape and all(got[f].tobytes() == want[f].tobytes() for f in want.dtype.names), \
            (k, i, got, want)
        assert not recs[i, int(counts[i]):].tobytes().strip(b"\0")
    assert n_breaks >= 2, n_breaks
