"""The drift solve's per-segment path report on the device (csrc/ffs_drift_report.h via ffsubsync_amd.drift_report): bit
for bit against the numpy model tests/drift_report_model.py; max_step = 0 against split_report_batch; the drift outputs
against drift_align_batch; long pairs, batching, the workspace, the C entry point's error returns, and
checked_drift_sync's decisions at the calibrated defaults."""
import ctypes
import math

import numpy as np
import pytest

import drift_report_model as drm
from test_gpu_drift import _bits, _device_pairs, _fuzz_problems as _drift_fuzz_problems, _same

pytestmark = pytest.mark.gpu

FP_FIELDS = ("own_score", "prev_score", "next_score", "flat_score", "mean", "std", "peak_score")
INT_FIELDS = ("first_block", "end_block", "start_sample", "end_sample", "first_offset", "last_offset", "min_offset",
              "max_offset", "flat_offset", "n_lags", "peak_shift", "n_peaks", "flags")

# checked_drift_sync at the defaults, two-hour problems of workloads/drift.py, +-60 s (a window the calibration covers:
# profiles/drift_report_calibration.json).  The device equals the model bit for bit, so the decision of
# every seed is known from the CPU model: drifting seeds 0..7 one segment each, psr 7.96 .. 8.33, drift gain
# 2.54 .. 5.30 -> "drift"; clean seeds 0..7 one segment, no step, psr 8.10 .. 8.42 -> "drift"; wrong pairs 0..7 (subtitle
# of seed i, reference of seed i+1) segment psr <= 4.09 < 6 and whole-file psr 2.45 .. 3.10 < 5 -> "untrusted".  No seed
# is left out of any class.
VERDICT_SEEDS = tuple(range(8))
DRIFTING_DECISION = {s: "drift" for s in VERDICT_SEEDS}
CLEAN_DECISION = {s: "drift" for s in VERDICT_SEEDS}
WRONG_DECISION = {s: "untrusted" for s in VERDICT_SEEDS}


def _edge_problem(seed, k, w, blocks=10):
    """A first half next to the window's lower edge, then a jump to a stretch that drifts down fast: the shift that would
    continue the first half lies outside the second segment's shift set (NaN neighbour scores)."""
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
    return dict(ref=rb.astype(float), sub=sb.astype(float), rb=rb, sb=sb, r_lv=(0.0, 1.0), s_lv=(0.0, 1.0), k=k, w=w,
                p=3.0 * k / 8, s=2, q=0.0)


def _fuzz_problems(n=96):
    """test_gpu_drift's fuzz set (K in {256, 1024, 4096}, W from 40 to 6000, P in {0, 100, 8192, inf}, max_step in
    {0, 1, 2, 7}, step_cost in {0, 0.5, 64, 1e6}, non-default levels) plus three problems whose path touches the window
    edge; top_k and the exclusion distance vary with the problem."""
    out = _drift_fuzz_problems(n) + [_edge_problem(3, 256, 40), _edge_problem(5, 1024, 63), _edge_problem(4, 256, 200)]
    for i, pr in enumerate(out):
        pr["top_k"] = 1 + i % 8
        pr["excl"] = [1, 5, 300, 50, 2000][i % 5]
    return out


def _model(pr):
    return drm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], pr["top_k"],
                      pr["excl"])


def _diff(got, want):
    """Names of the fields in which two SEGMENT_REPORT_DTYPE arrays differ, fp64 fields compared as int64 bits."""
    bad = [f for f in FP_FIELDS if not np.array_equal(_bits(got[f]), _bits(want[f]))]
    return bad + [f for f in INT_FIELDS if not np.array_equal(got[f], want[f])]


def test_device_records_equal_the_model_bit_for_bit():
    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_report as dr

    assert set(FP_FIELDS) | set(INT_FIELDS) == set(_native.SEGMENT_REPORT_DTYPE.names)
    bad = []
    stepping = many = nan_inside = own_not_peak = narrow = 0
    for i, pr in enumerate(_fuzz_problems()):
        res, recs, counts = dr.drift_report_batch(_device_pairs([(pr["ref"], pr["sub"])]), pr["w"], pr["k"], pr["p"],
                                                  pr["s"], pr["q"], pr["top_k"], pr["excl"], raw=True)
        want_solve, want, _ = _model(pr)
        n = len(want)
        stepping += int((want["min_offset"] != want["max_offset"]).sum())
        many += n > 8
        nan_inside += int(np.isnan(want["prev_score"][1:]).sum() + np.isnan(want["next_score"][:-1]).sum())
        own_not_peak += int(((want["flags"] & _native.SEGMENT_OWN_NOT_PEAK) != 0).sum())
        narrow += int((want["n_lags"] < 2 * pr["w"]).sum())
        if not _same(res[0], want_solve) or int(counts[0]) != n:
            bad.append((i, "solve", int(counts[0]), n))
            continue
        d = _diff(recs[0, :n], want)
        if d or recs[0, n:].tobytes().strip(b"\0"):
            bad.append((i, pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], n, d))
    assert not bad, bad[:5]
    # the set holds what the report has to get right
    assert stepping >= 20 and many >= 3 and nan_inside >= 1 and own_not_peak >= 1 and narrow >= 20, \
        (stepping, many, nan_inside, own_not_peak, narrow)


def test_max_step_zero_equals_split_report_and_outputs_equal_drift_align():
    """I1 and I2 on the same batches, one of them with more pairs than pairs_in_flight and mixed lengths."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_report as dr
    from ffsubsync_amd import split_report as sr

    base = [pr for pr in _drift_fuzz_problems(60) if pr["k"] == 256][:20]
    probs = []
    for i in range(50):
        pr = base[i % len(base)]
        probs.append(dict(pr, sub=pr["sub"][: pr["sub"].size - 37 * (i // len(base))], ref=np.roll(pr["ref"], 11 * i)))
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    assert len(set(int(x) for x in db.lens[:, 1])) > 10
    for w, p, s, q, pif in ((1000, 100.0, 0, 3.0, 16), (1000, 100.0, 2, 0.5, 16), (511, 0.0, 0, 0.0, None),
                            (200, np.inf, 7, 0.0, 7)):
        dr.clear_plan_cache()
        drift = da.drift_align_batch(db, w, 256, p, s, q)
        reps = dr.drift_report_batch(db, w, 256, p, s, q, 4, 50, pairs_in_flight=pif)
        for a, rep in zip(drift, reps):  # I2
            b = rep.drift
            assert np.array_equal(a.block_offsets, b.block_offsets) and np.array_equal(a.block_jump, b.block_jump)
            assert np.array_equal(_bits(a.block_scores), _bits(b.block_scores)) and _bits([a.total])[0] == _bits([b.total])[0]
            assert len(rep.segments) == len(b.segments)
            for x, y in zip(rep.segments, b.segments):
                assert (x.first_block, x.end_block, x.start_sample, x.end_sample, x.first_offset, x.last_offset) == \
                    (y.first_block, y.end_block, y.start_sample, y.end_sample, y.first_offset, y.last_offset)
        if s:
            continue
        _, want, wn = sr.split_report_batch(db, w, 256, p, 4, 50, raw=True)
        _, got, gn = dr.drift_report_batch(db, w, 256, p, 0, q, 4, 50, pairs_in_flight=pif, raw=True)
        assert np.array_equal(wn, gn)
        for pi in range(len(probs)):  # I1
            a, b = got[pi, :gn[pi]], want[pi, :wn[pi]]
            for name in ("first_block", "end_block", "start_sample", "end_sample", "n_lags", "n_peaks", "flags"):
                assert np.array_equal(a[name], b[name]), (pi, name)
            for name in ("own_score", "prev_score", "next_score", "mean", "std", "peak_score"):
                assert np.array_equal(_bits(a[name]), _bits(b[name])), (pi, name)
            live = np.arange(8)[None, :] < a["n_peaks"][:, None]
            assert np.array_equal((a["peak_shift"] + b["offset"][:, None])[live], b["peak_offset"][live]), pi
            for name in ("first_offset", "last_offset", "min_offset", "max_offset", "flat_offset"):
                assert np.array_equal(a[name], b["offset"]), (pi, name)
            assert np.array_equal(_bits(a["flat_score"]), _bits(a["own_score"])), pi
    dr.clear_plan_cache()


def test_two_hour_pairs_equal_the_model():
    """Two-hour problems of workloads/drift.py at the defaults: two at +-60 s, one at +-5 min with an inserted break (two
    segments, one supported jump), one at +-10 min."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_report as dr
    from workloads import drift

    cases = [(drift.make_problem(3), 6000), (drift.make_problem(4), 6000),
             (drift.make_problem(5, insert_break=True), 30000), (drift.make_problem(6), 60000)]
    for pr, w in cases:
        db = _device_pairs([(pr.ref.astype(float), pr.sub.astype(float) * pr.sub_hi)])
        res, recs, counts = dr.drift_report_batch(db, w, raw=True)
        want_solve, want, _ = drm.report(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), 1024, w, da.DEFAULT_SPLIT_PENALTY,
                                         da.DEFAULT_MAX_STEP, da.DEFAULT_STEP_COST, dr.DEFAULT_TOP_K,
                                         dr.DEFAULT_EXCLUSION_SAMPLES)
        assert _same(res[0], want_solve), (pr.seed, w)
        assert int(counts[0]) == len(want) and not _diff(recs[0, :len(want)], want), (pr.seed, w, _diff(recs[0, :len(want)], want))
        q = [dr.from_record(r) for r in recs[0, :len(want)]]
        assert all(s.stepped and s.own_is_peak for s in q)
        if pr.break_ref_s is not None:
            assert len(q) == 2 and dr.jump_support(q) == [True] and dr.assess_drift(q) == []
        dr.clear_plan_cache()


def test_report_workspace_is_added_by_the_first_report_call_only():
    import torch

    from ffsubsync_amd import _native

    pr = _drift_fuzz_problems(8)[4]
    db = _device_pairs([(pr["ref"], pr["sub"])] * 3)
    k, w = pr["k"], pr["w"]
    max_b = int((db.lens[:, 1].max() + k - 1) // k)
    plan = _native.DriftPlan(2, max_b, 2 * w, int(db.lens[:, 1].max()))
    n = db.n_pairs

    def outputs():
        return (torch.zeros(n * max_b, dtype=torch.int32, device="cuda"), torch.zeros(n * max_b, dtype=torch.float64, device="cuda"),
                torch.zeros(n * max_b, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"))

    def plain():
        o = outputs()
        plan.align(*db.pair_arrays(), k, w, 100.0, 2, 0.5, *o)
        return [x.cpu().numpy().tobytes() for x in o]

    size = plan.workspace_bytes
    before = plain()
    assert plan.workspace_bytes == size
    o = outputs()
    rep = torch.zeros(n * max_b * _native.SEGMENT_REPORT_BYTES // 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.report(*db.pair_arrays(), k, w, 100.0, 2, 0.5, 3, 50, *o, rep, cnt)
    lpad = (2 * w + 63) // 64 * 64
    assert plan.workspace_bytes == size + 2 * 8 * lpad * 8  # pairs in flight * 8 fp64 rows of the padded lag count
    assert [x.cpu().numpy().tobytes() for x in o] == before
    assert plain() == before and plan.workspace_bytes == size + 2 * 8 * lpad * 8
    recs = rep.cpu().numpy().view(_native.SEGMENT_REPORT_DTYPE).reshape(n, max_b)
    assert (cnt.cpu().numpy() >= 1).all() and recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes()
    plan.close()


def test_error_returns_through_ctypes_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    lib = _native.load()
    plan = _native.DriftPlan(2, 8, 2000, 4096)
    words = torch.zeros(256, dtype=torch.int32, device="cuda")
    ptr = np.array([words.data_ptr()], dtype=np.uint64)
    n_r, n_s = np.array([4000], np.int64), np.array([3000], np.int64)
    lo, hi = np.array([0.0]), np.array([1.0])
    offs = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    scores = torch.full((8,), 7.5, dtype=torch.float64, device="cuda")
    jumps = torch.full((8,), 9, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), 7.5, dtype=torch.float64, device="cuda")
    rep = torch.full((8 * _native.SEGMENT_REPORT_BYTES // 8 + 1,), 123, dtype=torch.int64, device="cuda")
    cnt = torch.full((2,), 55, dtype=torch.int32, device="cuda")
    outs = (offs, scores, jumps, total, rep, cnt)
    before = [x.cpu().numpy().tobytes() for x in outs]

    def call(handle=plan.handle, n=1, n_s=n_s, hi=hi, k=512, w=1000, p=8192.0, s=2, q=64.0, top_k=3, excl=300,
             rep_ptr=None, cnt_ptr=None):
        return lib.ffs_align_drift_report_batch(
            handle, n, ptr.ctypes.data, n_r.ctypes.data, lo.ctypes.data, hi.ctypes.data, ptr.ctypes.data, n_s.ctypes.data,
            lo.ctypes.data, hi.ctypes.data, k, w, p, s, q, top_k, excl, offs.data_ptr(), scores.data_ptr(),
            jumps.data_ptr(), total.data_ptr(), rep.data_ptr() if rep_ptr is None else rep_ptr,
            cnt.data_ptr() if cnt_ptr is None else cnt_ptr, None)

    inv, empty = -1, -5  # FFS_E_INVALID, FFS_E_EMPTY
    assert call(n=0) == 0
    assert call(handle=None) == inv and call(n=-1) == inv
    assert call(top_k=0) == inv and b"top_k" in lib.ffs_last_error()
    assert call(top_k=9) == inv
    assert call(excl=0) == inv and b"exclusion_samples" in lib.ffs_last_error()
    assert call(rep_ptr=ctypes.c_void_p(0)) == inv and call(cnt_ptr=ctypes.c_void_p(0)) == inv
    assert call(rep_ptr=ctypes.c_void_p(rep.data_ptr() + 4)) == inv and b"misaligned" in lib.ffs_last_error()
    assert call(cnt_ptr=ctypes.c_void_p(cnt.data_ptr() + 2)) == inv
    assert call(s=-1) == inv and call(s=8) == inv
    for q in (-1.0, float("nan"), float("inf")):
        assert call(q=q) == inv and b"step_cost" in lib.ffs_last_error()
    assert call(p=-1.0) == inv and call(p=float("nan")) == inv
    assert call(k=500) == inv and call(k=128) == inv
    assert call(w=0) == inv and call(w=1001) == inv  # 2W beyond the plan's max_lags
    assert call(n_s=np.array([0], np.int64)) == empty
    assert call(n_s=np.array([4097], np.int64)) == inv  # beyond max_samples
    assert call(n_s=np.array([4096], np.int64), k=256) == inv  # 16 blocks beyond max_blocks
    assert call(hi=np.array([np.inf])) == inv
    torch.cuda.synchronize()
    assert [x.cpu().numpy().tobytes() for x in outs] == before  # every refusal came before any launch
    assert call() == 0 and call(top_k=8, excl=1, s=7, q=0.0, p=float("inf")) == 0
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) >= 1 and int(cnt.cpu()[1]) == 55
    plan.close()
    with pytest.raises(ValueError):
        from ffsubsync_amd import drift_report as dr

        dr.drift_report_batch(None, 100, exclusion_samples=0)


def _errors(results, probs):
    return [float(np.mean(np.abs(r.cue_start_us - p.true_start_us))) / 1e4 for r, p in zip(results, probs)]


def test_checked_drift_sync_applies_real_drift():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_report as dr
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    assert len(VERDICT_SEEDS) >= 8 and VERDICT_SEEDS == tuple(range(len(VERDICT_SEEDS)))
    probs = [drift.make_problem(seed) for seed in VERDICT_SEEDS]
    items = [(p.ref.astype(float), p.track) for p in probs]
    got = dr.checked_drift_sync(items, max_offset_seconds=60)
    plain = da.drift_sync(items, max_offset_seconds=60)
    split = sa.split_sync(items, max_offset_seconds=60)
    rows = [(p.seed, g.decision, [round(q.psr, 2) for q in g.segment_quality], [round(q.drift_gain, 2) for q in g.segment_quality],
             round(es, 2), round(eg, 2)) for p, g, es, eg in zip(probs, got, _errors(split, probs), _errors(got, probs))]
    print("seed, decision, segment psr, drift gain, split error, checked error (samples):", rows)
    for p, g, d in zip(probs, got, plain):
        assert g.decision == DRIFTING_DECISION[p.seed] and g.reasons == [], (p.seed, g.decision, g.reasons)
        assert np.array_equal(g.cue_start_us, d.cue_start_us) and np.array_equal(g.cue_end_us, d.cue_end_us)
        assert np.array_equal(g.cue_segment, d.cue_segment) and g.fallback is None
        assert len(g.segment_quality) == len(g.segments) == len(d.segments) and len(g.supported) == len(g.segments) - 1
        assert any(q.stepped for q in g.segment_quality)
    assert all(r[5] <= 0.5 * r[4] for r in rows), rows


def test_checked_drift_sync_on_clean_problems_gives_split_sync_times():
    from ffsubsync_amd import drift_report as dr
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    probs = [drift.make_problem(seed, clean=True) for seed in VERDICT_SEEDS]
    items = [(p.ref.astype(float), p.track) for p in probs]
    got = dr.checked_drift_sync(items, max_offset_seconds=60)
    for p, g, a in zip(probs, got, sa.split_sync(items, max_offset_seconds=60)):
        assert g.decision == CLEAN_DECISION[p.seed], (p.seed, g.decision, g.reasons)
        assert not any(q.stepped for q in g.segment_quality)
        assert np.array_equal(g.cue_start_us, a.cue_start_us) and np.array_equal(g.cue_end_us, a.cue_end_us)
        assert (g.ratio, g.global_offset) == (a.ratio, a.global_offset)


def test_checked_drift_sync_leaves_wrong_pairs_alone():
    from ffsubsync_amd import drift_report as dr
    from workloads import drift

    probs = [drift.make_problem(seed) for seed in range(len(VERDICT_SEEDS) + 1)]
    items = [(probs[i + 1].ref.astype(float), probs[i].track) for i in VERDICT_SEEDS]
    got = dr.checked_drift_sync(items, max_offset_seconds=60)
    print("seed, decision, max segment psr:", [(i, g.decision, round(max(q.psr for q in g.segment_quality), 2))
                                               for i, g in zip(VERDICT_SEEDS, got)])
    for i, g in zip(VERDICT_SEEDS, got):
        assert g.decision == WRONG_DECISION[i], (i, g.decision, g.reasons)
        assert np.array_equal(g.cue_start_us, probs[i].start_us) and np.array_equal(g.cue_end_us, probs[i].end_us)
        assert g.reasons and g.fallback is not None and (g.cue_segment == -1).all()
        assert any(r.startswith("segment") for r in g.reasons)
    assert math.isfinite(sum(q.psr for g in got for q in g.segment_quality))
