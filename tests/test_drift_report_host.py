"""The drift solve's per-segment path report without a GPU: the numpy model tests/drift_report_model.py against a
brute-force count, against split_report_model at max_step = 0 and on segments without steps; the host derivations
(drift_report.from_record, jump_support, assess_drift) on hand-made records; argument validation; the record layout."""
import math
import os
import re

import numpy as np
import pytest

import drift_report_model as drm
import split_model as sm
import split_report_model as srm
from ffsubsync_amd import _native
from ffsubsync_amd import drift_report as dr


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _small_problems(n=48):
    """Seeded small problems for the brute-force comparison: K in {32, 64}, W from 6 to 40, R != S, a short last block,
    a subtitle that drifts against the reference (so the DP steps), a break in every third (so it jumps too) and a true
    shift next to the window edge in every fourth (so the path touches the edge and the shift set is narrow)."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(9100 + seed)
        k = [32, 64][seed % 2]
        w = int([6, 9, 16, 25, 40][seed % 5])
        S = int(rng.randint(4 * k, 9 * k)) | 1
        R = S + int(rng.randint(-2 * k, 2 * k)) | 1
        if R == S:
            R += 2
        seg = np.maximum(1, rng.geometric(1.0 / 6.0, size=R + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        shift = (w - 2) * (1 if seed % 8 < 4 else -1) if seed % 4 == 3 else int(rng.randint(-w // 2, w // 2 + 1))
        drift = rng.uniform(-1.0, 1.0) * 3.0 / S * (4 if seed % 2 else 1)
        idx = np.arange(S) + shift + np.rint(drift * np.arange(S)).astype(np.int64)
        if seed % 3 == 1:
            idx[S // 2:] += int(rng.randint(3, max(4, w // 2)))
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.04
        r_lv = [(0.0, 1.0), (-1.0, 2.5)][seed % 7 == 0]
        s_lv = (0.0, [1.0, 0.959, 0.8][seed % 3])
        out.append(dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, k=k, w=w, p=[0.0, 6.0, 40.0, np.inf][(seed // 3) % 4],
                        s=[1, 2, 7, 0][(seed // 2) % 4], q=[0.0, 0.5, 2.0][(seed // 5) % 3]))
    return out


def _report(pr, **kw):
    return drm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], 3,
                      kw.get("excl", 5))


def test_path_curve_equals_brute_force_count():
    """I3: every block's slice compared with the reference at lag o_b + delta, no block counts, no prefix sums."""
    stepped = jumped = both = narrow = short_last = 0
    for pr in _small_problems():
        (offs, _, jump, _), recs, curves = _report(pr)
        S, k, w = pr["sb"].size, pr["k"], pr["w"]
        short_last += S % k != 0
        took = False
        for rec, c in zip(recs, curves):
            f, e = int(rec["first_block"]), int(rec["end_block"])
            want = drm.brute_path_curve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, w, f, e, offs)
            assert c.size == want.size == int(rec["n_lags"]) == 2 * w - int(rec["max_offset"] - rec["min_offset"])
            assert np.array_equal(_bits(c), _bits(want))
            assert int(rec["min_offset"]) == offs[f:e].min() and int(rec["max_offset"]) == offs[f:e].max()
            assert -w + 1 <= int(rec["min_offset"]) and int(rec["max_offset"]) <= w
            took |= bool(rec["min_offset"] != rec["max_offset"])
            narrow += c.size < 2 * w and (int(rec["min_offset"]) == -w + 1 or int(rec["max_offset"]) == w)
        stepped += took
        jumped += bool(jump.sum())
        both += took and bool(jump.sum())
    assert stepped >= 8 and jumped >= 8 and both >= 3 and narrow >= 2 and short_last >= 8, (stepped, jumped, both, narrow)


def test_own_score_is_the_block_score_sum_only_with_integer_terms():
    for pr in _small_problems(24):
        (offs, scores, _, _), recs, _ = _report(pr)
        if pr["r_lv"] == (0.0, 1.0) and pr["s_lv"] == (0.0, 1.0):
            for rec in recs:
                assert float(rec["own_score"]) == float(np.sum(scores[int(rec["first_block"]):int(rec["end_block"])]))


def test_max_step_zero_segments_are_split_report_pieces():
    """I1 at model level: every shared field bit for bit, peak_shift + offset = peak_offset, flat = own."""
    n_pieces = 0
    for pr in _small_problems():
        pr = dict(pr, s=0)
        _, recs, curves = _report(pr)
        _, want, wcurves = srm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"], 3, 5)
        assert len(recs) == len(want)
        n_pieces += len(want)
        for a, b, ca, cb in zip(recs, want, curves, wcurves):
            assert np.array_equal(_bits(ca), _bits(cb))
            for name in ("first_block", "end_block", "start_sample", "end_sample", "n_lags", "n_peaks", "flags"):
                assert a[name] == b[name], name
            for name in ("own_score", "prev_score", "next_score", "mean", "std"):
                assert _bits([a[name]])[0] == _bits([b[name]])[0], name
            assert np.array_equal(_bits(a["peak_score"]), _bits(b["peak_score"]))
            n = int(a["n_peaks"])
            assert np.array_equal(a["peak_shift"][:n] + b["offset"], b["peak_offset"][:n])
            assert a["first_offset"] == a["last_offset"] == a["min_offset"] == a["max_offset"] == b["offset"]
            assert _bits([a["flat_score"]])[0] == _bits([a["own_score"]])[0] and a["flat_offset"] == b["offset"]
    assert n_pieces > 60


def test_segment_without_steps_equals_the_piece_curve_of_its_samples():
    seen = 0
    for pr in _small_problems():
        (offs, _, _, _), recs, curves = _report(pr)
        n11 = sm.block_counts(pr["rb"], pr["sb"], pr["k"], pr["w"])
        for rec, c in zip(recs, curves):
            if rec["min_offset"] != rec["max_offset"]:
                continue
            f, e = int(rec["first_block"]), int(rec["end_block"])
            want = srm.piece_curve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], int(rec["start_sample"]),
                                   int(rec["end_sample"]), n11[f:e].sum(axis=0))
            assert np.array_equal(_bits(c), _bits(want))
            seen += 1
    assert seen > 30


def _edge_problem(seed, k, w, blocks=10):
    """A first half next to the window's lower edge, then a jump to a stretch that drifts down fast: the shift that would
    continue the first half lies outside the second segment's shift set."""
    rng = np.random.RandomState(seed)
    S = blocks * k - 7
    R = S + 3 * k + 1
    seg = np.maximum(1, rng.geometric(1.0 / 8.0, size=R + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    i = np.arange(S)
    half = S // 2
    idx = np.where(i < half, i - (w - 2), i + w // 3 - np.rint((i - half) * (0.6 * w) / (S - half)).astype(np.int64))
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    return dict(rb=rb, sb=sb, r_lv=(0.0, 1.0), s_lv=(0.0, 1.0), k=k, w=w, p=3.0 * k / 8, s=2, q=0.0)


def test_neighbour_scores_are_the_curve_at_the_continuing_shift_or_nan():
    nan_seen = real_seen = 0
    for pr in _small_problems() + [_edge_problem(1, 32, 16), _edge_problem(3, 256, 40)]:
        (offs, _, _, _), recs, curves = _report(pr)
        for i, (rec, c) in enumerate(zip(recs, curves)):
            lo = -pr["w"] + 1 - int(rec["min_offset"])
            assert _bits([rec["own_score"]])[0] == _bits([c[-lo]])[0]
            if i == 0:
                assert math.isnan(rec["prev_score"])
                continue
            q = int(recs[i - 1]["last_offset"] - rec["first_offset"]) - lo
            if 0 <= q < c.size:
                assert _bits([rec["prev_score"]])[0] == _bits([c[q]])[0]
                real_seen += 1
            else:
                assert math.isnan(rec["prev_score"])
                nan_seen += 1
    assert nan_seen >= 1 and real_seen >= 10, (nan_seen, real_seen)


def _record(**kw):
    rec = np.zeros(1, dtype=_native.SEGMENT_REPORT_DTYPE)[0]
    base = dict(first_block=0, end_block=10, start_sample=0, end_sample=10240, first_offset=5, last_offset=5, min_offset=5,
                max_offset=5, own_score=900.0, prev_score=math.nan, next_score=math.nan, flat_score=900.0, flat_offset=5,
                mean=100.0, std=100.0, n_lags=2000, n_peaks=2, flags=0)
    base.update(kw)
    peaks = base.pop("peaks", [(900.0, 0), (300.0, 700)])
    for name, v in base.items():
        rec[name] = v
    for i, (s, sh) in enumerate(peaks):
        rec["peak_score"][i], rec["peak_shift"][i] = s, sh
    rec["n_peaks"] = len(peaks)
    return rec


def test_from_record_derivations():
    q = dr.from_record(_record(first_offset=3, last_offset=9, min_offset=3, max_offset=9, flat_score=650.0, flat_offset=6,
                               prev_score=400.0, next_score=math.nan))
    assert (q.psr, q.margin, q.gain_prev, q.drift_gain) == (8.0, 6.0, 5.0, 2.5) and math.isnan(q.gain_next)
    assert q.stepped and q.own_is_peak and not q.flat and q.peaks == [(900.0, 0), (300.0, 700)]
    assert (q.first_offset, q.last_offset, q.min_offset, q.max_offset, q.flat_offset, q.n_lags) == (3, 9, 3, 9, 6, 2000)
    one = dr.from_record(_record(peaks=[(900.0, 0)]))
    assert one.margin == math.inf and one.drift_gain == 0.0 and not one.stepped
    flat = dr.from_record(_record(std=0.0, mean=900.0, prev_score=900.0, flags=_native.QUALITY_FLAT))
    assert (flat.psr, flat.margin, flat.gain_prev, flat.drift_gain) == (0.0, 0.0, 0.0, 0.0) and math.isnan(flat.gain_next)
    assert flat.flat
    off = dr.from_record(_record(flags=_native.SEGMENT_OWN_NOT_PEAK, peaks=[(950.0, 12), (300.0, 700)]))
    assert not off.own_is_peak and off.psr == 8.5


def test_jump_support_and_assess_drift():
    a = dr.from_record(_record(next_score=100.0))  # gain_next 8
    b = dr.from_record(_record(first_block=10, end_block=20, prev_score=300.0, next_score=math.nan))  # gain_prev 6
    assert dr.jump_support([a, b], 6.0) == [True] and dr.jump_support([a, b], 6.5) == [False]
    assert dr.assess_drift([a, b], 7.0, 6.0, 1.0) == []
    assert dr.assess_drift([a, b], 8.5, 6.0, 1.0) == ["segment 0: psr 8.0 < 8.5", "segment 1: psr 8.0 < 8.5"]
    assert dr.assess_drift([a, b], 7.0, 7.0, 1.0) == ["jump 0 (block 10): gain 8.0 / 6.0 < 7.0"]
    # a NaN neighbour score (the continuing shift lies outside the shift set) compares false: unsupported
    c = dr.from_record(_record(first_block=10, end_block=20, prev_score=math.nan))
    assert dr.jump_support([a, c], 0.0) == [False]
    assert dr.assess_drift([a, c], 7.0, 0.0, 1.0) == ["jump 0 (block 10): gain 8.0 / nan < 0.0"]
    # drift claimed without evidence: a segment that took a step, drift_gain below the floor
    s = dr.from_record(_record(min_offset=5, max_offset=7, last_offset=7, flat_score=850.0))  # drift_gain 0.5
    assert dr.assess_drift([s], 7.0, 6.0, 1.0) == ["segment 0: drift gain 0.5 < 1.0"]
    assert dr.assess_drift([s], 7.0, 6.0, 0.5) == []
    # the same gain without a step is no claim
    assert dr.assess_drift([dr.from_record(_record(flat_score=850.0))], 7.0, 6.0, 1.0) == []
    flat = dr.from_record(_record(std=0.0, flags=_native.QUALITY_FLAT))
    assert dr.assess_drift([flat], 7.0, 6.0, 1.0) == ["segment 0: flat correlation (std 0)"]


def test_argument_validation_raises_before_any_native_call():
    ok = dict(block_samples=1024, max_offset_samples=6000, split_penalty=8192.0, max_step=2, step_cost=128.0, top_k=3,
              exclusion_samples=300)
    dr.validate_args(**ok)
    for bad in (dict(block_samples=1000), dict(max_offset_samples=0), dict(split_penalty=-1.0), dict(max_step=8),
                dict(max_step=1.5), dict(step_cost=-1.0), dict(step_cost=float("nan")), dict(top_k=0), dict(top_k=9),
                dict(exclusion_samples=0)):
        with pytest.raises(ValueError):
            dr.validate_args(**dict(ok, **bad))
    with pytest.raises(ValueError):
        dr.drift_report_batch(None, 6000, top_k=9)
    with pytest.raises(ValueError):
        dr.checked_drift_sync([], max_step=9)


def test_record_layout_matches_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ffsubsync_amd.h")).read()
    body = re.search(r"typedef struct ffs_segment_report \{(.*?)\} ffs_segment_report;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x).strip() for x in decl.split(None, 1)[1].split(",")]
    assert names == list(_native.SEGMENT_REPORT_DTYPE.names)
    assert "sizeof(ffs_segment_report) == %d" % _native.SEGMENT_REPORT_BYTES in text
    assert "#define FFS_SEGMENT_OWN_NOT_PEAK %d" % _native.SEGMENT_OWN_NOT_PEAK in text
    assert "ffs_align_drift_report_batch" in _native.EXPORTED_SYMBOLS and "ffs_align_drift_report_batch(" in text
