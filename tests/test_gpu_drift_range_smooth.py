"""The smooth drift fit over a lag range on the device (csrc/ffs_drift_range_smooth.h via
ffsubsync_amd.drift_range_smooth): bit for bit against the numpy model tests/drift_range_smooth_model.py on every
output, alone and batched; against smooth_align_batch at [-W+1, W]; the drift outputs against drift_align_range_batch;
the workspace the first smooth call adds; the C entry point's refusals; and smooth_cut_sync's three steps on subtitles
for another cut that also drift.  Every comparison is exact."""
import ctypes
import json
import os

import numpy as np
import pytest

import drift_range_smooth_model as drsm
from drift_range_smooth_cases import SMALL, coverage, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_FIELDS = ("fit_total", "line_score", "bend_total")
INT_FIELDS = ("n_knots", "reserved")
BATCH_SETTING = (60.0, 2, 1.0, 3, 5, 1.0)  # split_penalty, max_step, step_cost, knot_blocks, radius, bend_cost


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_pairs(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _same_drift(res, want):
    offs, scores, jump, total = want
    return (np.array_equal(res.block_offsets, offs) and np.array_equal(_bits(res.block_scores), _bits(scores))
            and np.array_equal(res.block_jump, jump) and _bits([res.total])[0] == _bits([total])[0])


def _diff(raw, p, want):
    """Names of the outputs of pair ``p`` of a raw result that differ from the model's ``want``."""
    res, smooth, knot, recs, counts = raw
    want_solve, want_smooth, want_knot, want_recs = want
    n, nb = len(want_recs), want_smooth.size
    d = [] if _same_drift(res[p], want_solve) else ["drift"]
    if int(counts[p]) != n:
        return d + ["n_segments"]
    d += [f for f in FP_FIELDS if not np.array_equal(_bits(recs[p, :n][f]), _bits(want_recs[f]))]
    d += [f for f in INT_FIELDS if not np.array_equal(recs[p, :n][f], want_recs[f])]
    if not np.array_equal(smooth[p, :nb], want_smooth) or smooth[p, nb:].any():
        d.append("smooth_offset")
    if not np.array_equal(knot[p, :nb], want_knot) or knot[p, nb:].any():
        d.append("knot")
    if recs[p, n:].tobytes().strip(b"\0"):
        d.append("records past the count")
    return d


def test_device_equals_the_model_bit_for_bit():
    """Every problem in a call of its own at its own parameters, then all of them per K in one batch of several
    sub-batches (pairs_in_flight 3, so slot != output row) at one setting."""
    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_range_smooth as drs

    assert set(FP_FIELDS) | set(INT_FIELDS) == set(_native.SMOOTH_SEGMENT_DTYPE.names)
    c = coverage()
    assert c["one_block"] >= 1 and c["two_block"] >= 1 and c["last_shorter"] >= 1 and c["last_longer"] >= 1, c
    assert c["most_intervals"] > 64 and c["most_segments"] > 4 and c["widest_step"] >= 1 and c["knot_outside"] >= 1, c
    assert c["moved"] >= 20, c
    assert {1, 5, 63, 65, 2049} <= {pr["hi"] - pr["lo"] + 1 for pr in SMALL}
    bad = []
    for i, pr in enumerate(SMALL):
        raw = drs.smooth_align_range_batch(_device_pairs([(pr["ref"], pr["sub"])]), (pr["lo"], pr["hi"]), pr["k"], pr["p"],
                                           pr["s"], pr["q"], pr["m"], pr["r"], pr["lam"], raw=True)
        d = _diff(raw, 0, model(i))
        if d:
            bad.append((i, pr["k"], pr["lo"], pr["hi"], pr["s"], pr["m"], pr["r"], pr["lam"], d))
    assert not bad, bad[:5]
    p, s, q, m, r, lam = BATCH_SETTING
    for k in (256, 512, 1024):
        idx = [i for i, pr in enumerate(SMALL) if pr["k"] == k]
        db = _device_pairs([(SMALL[i]["ref"], SMALL[i]["sub"]) for i in idx])
        drs.clear_plan_cache()
        raw = drs.smooth_align_range_batch(db, [(SMALL[i]["lo"], SMALL[i]["hi"]) for i in idx], k, p, s, q, m, r, lam,
                                           pairs_in_flight=3, raw=True)
        for at, i in enumerate(idx):
            pr = SMALL[i]
            want = drsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], p, s, q, m, r, lam)
            assert not _diff(raw, at, want), (k, i, _diff(raw, at, want))
    drs.clear_plan_cache()


def _same_raw(a, b, n):
    for p in range(n):
        x, y = a[0][p], b[0][p]
        if not (np.array_equal(x.block_offsets, y.block_offsets) and np.array_equal(x.block_jump, y.block_jump)
                and np.array_equal(_bits(x.block_scores), _bits(y.block_scores)) and _bits([x.total])[0] == _bits([y.total])[0]):
            return False
    return all(a[j].tobytes() == b[j].tobytes() for j in (1, 2, 3, 4))


def test_symmetric_range_equals_smooth_align_batch():
    """All eight outputs byte for byte at [-W+1, W]: the small problems per K at several settings, and one two-hour pair
    of workloads/drift.py at W = 6000 and drift_smooth's defaults."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_range_smooth as drs
    from ffsubsync_amd import drift_smooth as ds
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    settings = ((40, 60.0, 2, 1.0, 3, 5, 1.0), (700, 0.0, 7, 0.0, 1, 16, 0.0), (3000, np.inf, 1, 16.0, 256, 1, 64.0),
                (333, 60.0, 3, 1.0, 8, 16, 1e6))
    moved = 0
    for k in (256, 512, 1024):
        idx = [i for i, pr in enumerate(SMALL) if pr["k"] == k]
        db = _device_pairs([(SMALL[i]["ref"], SMALL[i]["sub"]) for i in idx])
        for w, p, s, q, m, r, lam in settings:
            want = ds.smooth_align_batch(db, w, k, p, s, q, m, r, lam, raw=True)
            got = drs.smooth_align_range_batch(db, (-w + 1, w), k, p, s, q, m, r, lam, raw=True)
            assert _same_raw(got, want, len(idx)), (k, w, m, r)
            moved += int(sum((want[1][at, :res.block_offsets.size] != res.block_offsets).sum()
                             for at, res in enumerate(want[0])))
    assert moved >= 50
    pr = drift.make_problem(3)
    db = _device_pairs([(pr.ref.astype(float), pr.sub.astype(float) * pr.sub_hi)])
    w = 6000
    want = ds.smooth_align_batch(db, w, raw=True)
    got = drs.smooth_align_range_batch(db, (-w + 1, w), split_penalty=sa.DEFAULT_SPLIT_PENALTY, max_step=da.DEFAULT_MAX_STEP,
                                       step_cost=da.DEFAULT_STEP_COST, knot_blocks=ds.DEFAULT_KNOT_BLOCKS,
                                       radius=ds.DEFAULT_RADIUS, bend_cost=ds.DEFAULT_BEND_COST, raw=True)
    assert _same_raw(got, want, 1)
    assert np.count_nonzero(want[1][0] != want[0][0].block_offsets) > 100  # the fit moved the path
    ds.clear_plan_cache()
    drs.clear_plan_cache()


def test_drift_outputs_equal_drift_align_range_batch():
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs

    for k in (256, 512, 1024):
        idx = [i for i, pr in enumerate(SMALL) if pr["k"] == k]
        db = _device_pairs([(SMALL[i]["ref"], SMALL[i]["sub"]) for i in idx])
        ranges = [(SMALL[i]["lo"], SMALL[i]["hi"]) for i in idx]
        for p, s, q, m, r, lam in ((60.0, 2, 1.0, 3, 5, 1.0), (0.0, 7, 0.0, 256, 16, 0.0), (np.inf, 0, 128.0, 1, 0, 64.0)):
            want = dr.drift_align_range_batch(db, ranges, k, p, s, q)
            got = drs.smooth_align_range_batch(db, ranges, k, p, s, q, m, r, lam, pairs_in_flight=4)
            for i, x, y in zip(idx, want, got):
                assert _same_drift(y.drift, (x.block_offsets, x.block_scores, x.block_jump, x.total)), (k, i, s)
                assert [(g.first_block, g.end_block) for g in y.segments] == [(g.first_block, g.end_block) for g in x.segments]
    dr.clear_plan_cache()
    drs.clear_plan_cache()


def _outputs(torch, n, max_b, fill=0):
    from ffsubsync_amd import _native

    return (torch.full((n * max_b,), fill, dtype=torch.int32, device="cuda"),
            torch.full((n * max_b,), float(fill), dtype=torch.float64, device="cuda"),
            torch.full((n * max_b,), fill, dtype=torch.uint8, device="cuda"),
            torch.full((n,), float(fill), dtype=torch.float64, device="cuda"),
            torch.full((n * max_b,), fill, dtype=torch.int32, device="cuda"),
            torch.full((n * max_b,), fill, dtype=torch.uint8, device="cuda"),
            torch.full((n * max_b * _native.SMOOTH_SEGMENT_BYTES // 8,), fill, dtype=torch.int64, device="cuda"),
            torch.full((n,), fill, dtype=torch.int32, device="cuda"))


def test_smooth_workspace_is_added_by_the_first_smooth_call_only():
    import torch

    from ffsubsync_amd import _native

    pr = SMALL[0]
    db = _device_pairs([(pr["ref"], pr["sub"])] * 3)
    k = pr["k"]
    max_b = int((db.lens[:, 1].max() + k - 1) // k)
    n = db.n_pairs
    lo, hi = np.full(n, pr["lo"], np.int64), np.full(n, pr["hi"], np.int64)
    cap = 7
    plan = _native.DriftRangePlan(2, max_b, pr["hi"] - pr["lo"] + 1, int(db.lens.max()), cap)
    other = _native.DriftRangePlan(2, max_b, pr["hi"] - pr["lo"] + 1, int(db.lens.max()), cap)

    def plain(pl):
        o = _outputs(torch, n, max_b)[:4]
        pl.align(*db.pair_arrays(), k, lo, hi, 60.0, 2, 1.0, *o)
        return [x.cpu().numpy().tobytes() for x in o]

    size = plan.workspace_bytes
    before = plain(plan)
    assert plan.workspace_bytes == size == other.workspace_bytes and plain(other) == before
    o = _outputs(torch, n, max_b)
    plan.smooth(*db.pair_arrays(), k, lo, hi, 60.0, 2, 1.0, 2, 1, 4.0, *o)
    grown = plan.workspace_bytes
    mb = (max_b + 15) // 16 * 16
    assert grown - size == plan.smooth_bytes()  # the documented amount, to the byte
    assert 2 * mb * (9837 + 2 * (cap * 384 + 33)) <= grown - size <= 2 * mb * (9837 + 2 * (cap * 384 + 33)) + 128
    assert [x.cpu().numpy().tobytes() for x in o[:4]] == before  # the smooth call's drift outputs
    first = [x.cpu().numpy().tobytes() for x in o]
    assert plain(plan) == before and plan.workspace_bytes == grown  # the drift call after the workspace has grown
    plan.smooth(*db.pair_arrays(), k, lo, hi, 60.0, 7, 0.0, 256, 16, 0.0, *o)  # larger M, R and max_step, within the caps
    assert plan.workspace_bytes == grown
    plan.smooth(*db.pair_arrays(), k, lo, hi, 60.0, 2, 1.0, 2, 1, 4.0, *o)
    assert [x.cpu().numpy().tobytes() for x in o] == first and plan.workspace_bytes == grown
    assert other.workspace_bytes == size and plain(other) == before  # a plan that never calls it keeps its size
    recs = o[6].cpu().numpy().view(_native.SMOOTH_SEGMENT_DTYPE).reshape(n, max_b)
    assert (o[7].cpu().numpy() >= 1).all() and recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes()
    plan.close()
    other.close()


def test_refused_calls_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    lib = _native.load()
    plan = _native.DriftRangePlan(2, 8, 5000, 4096, 2)
    words = torch.zeros(256, dtype=torch.int32, device="cuda")
    ptr = np.array([words.data_ptr()], dtype=np.uint64)
    n_r, n_s = np.array([4000], np.int64), np.array([3000], np.int64)
    lo, hi = np.array([0.0]), np.array([1.0])
    offs = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    scores = torch.full((8,), 77.25, dtype=torch.float64, device="cuda")
    jumps = torch.full((8,), 0x5A, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), 77.25, dtype=torch.float64, device="cuda")
    smooth = torch.full((9,), 66, dtype=torch.int32, device="cuda")
    knot = torch.full((8,), 5, dtype=torch.uint8, device="cuda")
    rec = torch.full((8 * _native.SMOOTH_SEGMENT_BYTES // 8 + 1,), 123, dtype=torch.int64, device="cuda")
    cnt = torch.full((2,), 55, dtype=torch.int32, device="cuda")
    outs = (offs, scores, jumps, total, smooth, knot, rec, cnt)
    before = [x.cpu().numpy().tobytes() for x in outs]
    size = plan.workspace_bytes

    def call(handle=plan.handle, n=1, n_s=n_s, hi=hi, k=512, rng=(-1000, 2000), p=8192.0, s=2, q=64.0, m=2, r=3, lam=8.0,
             offs_ptr=None, jumps_ptr=None, smooth_ptr=None, knot_ptr=None, rec_ptr=None, cnt_ptr=None):
        l0, l1 = np.array([rng[0]], np.int64), np.array([rng[1]], np.int64)
        pick = lambda given, t: t.data_ptr() if given is None else given
        return lib.ffs_align_drift_range_smooth_batch(
            handle, n, ptr.ctypes.data, n_r.ctypes.data, lo.ctypes.data, hi.ctypes.data, ptr.ctypes.data, n_s.ctypes.data,
            lo.ctypes.data, hi.ctypes.data, k, l0.ctypes.data, l1.ctypes.data, p, s, q, m, r, lam, pick(offs_ptr, offs),
            scores.data_ptr(), pick(jumps_ptr, jumps), total.data_ptr(), pick(smooth_ptr, smooth), pick(knot_ptr, knot),
            pick(rec_ptr, rec), pick(cnt_ptr, cnt), None)

    inv, empty = -1, -5  # FFS_E_INVALID, FFS_E_EMPTY
    assert call(n=0) == 0
    # what the range drift call refuses
    assert call(rng=(5, 4)) == inv and b"lag range" in lib.ffs_last_error()
    assert call(rng=(-2 ** 31, 0)) == inv
    assert call(rng=(0, 5000)) == inv and b"max_lags" in lib.ffs_last_error()
    assert call(s=3) == inv and b"max_step" in lib.ffs_last_error()  # above the plan's cap
    assert call(s=-1) == inv
    for q in (-1.0, float("nan"), float("inf")):
        assert call(q=q) == inv and b"step_cost" in lib.ffs_last_error()
    assert call(p=-1.0) == inv and call(p=float("nan")) == inv
    assert call(k=500) == inv and call(k=128) == inv
    assert call(handle=None) == inv and call(n=-1) == inv
    assert call(n_s=np.array([0], np.int64)) == empty
    assert call(n_s=np.array([4097], np.int64)) == inv  # beyond max_samples
    assert call(n_s=np.array([4096], np.int64), k=256) == inv  # 16 blocks beyond max_blocks
    assert call(hi=np.array([np.inf])) == inv
    null = ctypes.c_void_p(0)
    assert call(jumps_ptr=null) == inv
    assert call(offs_ptr=ctypes.c_void_p(offs.data_ptr() + 2)) == inv and b"misaligned" in lib.ffs_last_error()
    # the fit's parameter and alignment checks
    assert call(m=0) == inv and b"knot_blocks" in lib.ffs_last_error()
    assert call(m=257) == inv and call(m=-3) == inv
    assert call(r=-1) == inv and b"radius" in lib.ffs_last_error()
    assert call(r=17) == inv
    for lam in (-1.0, float("nan"), float("inf")):
        assert call(lam=lam) == inv and b"bend_cost" in lib.ffs_last_error()
    assert call(smooth_ptr=null) == inv and call(knot_ptr=null) == inv and call(rec_ptr=null) == inv and call(cnt_ptr=null) == inv
    assert call(smooth_ptr=ctypes.c_void_p(smooth.data_ptr() + 2)) == inv and b"misaligned" in lib.ffs_last_error()
    assert call(rec_ptr=ctypes.c_void_p(rec.data_ptr() + 4)) == inv
    assert call(cnt_ptr=ctypes.c_void_p(cnt.data_ptr() + 2)) == inv
    torch.cuda.synchronize()
    assert [x.cpu().numpy().tobytes() for x in outs] == before  # every refusal came before any launch
    assert plan.workspace_bytes == size  # ... and before the workspace grew
    # and the accepted calls write them
    assert call() == 0 and call(m=256, r=16, lam=0.0, s=2, q=0.0, p=float("inf")) == 0 and call(m=1, r=0, s=0) == 0
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) >= 1 and int(cnt.cpu()[1]) == 55 and int(smooth.cpu()[8]) == 66
    assert int(rec.cpu()[-1]) == 123 and float(total[0]) != 77.25
    assert plan.workspace_bytes == size + plan.smooth_bytes()
    plan.close()
    with pytest.raises(ValueError):
        from ffsubsync_amd import drift_range_smooth as drs

        drs.smooth_align_range_batch(None, None, radius=17)


def test_smooth_cut_sync_chains_the_ratio_solve_the_range_fit_and_the_polyline_cue_map():
    """Two ten-minute steep problems of workloads/cut_drift.py (eps = +-6e-4, 22.5-30 min of inserts, so the range
    reaches beyond +-131 072) in one batch over one lag range: the drift part is cut_drift_sync's, the fit is
    smooth_align_range_batch's on the chosen candidates, the cue times are map_cues_smooth's.  (The accuracy test against
    profiles/drift_range_smooth_calibration.json is not here: that calibration chose nothing)"""
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs
    from ffsubsync_amd import drift_smooth as ds
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import cut_drift

    with open(os.path.join(ROOT, "profiles", "drift_range_smooth_calibration.json")) as f:
        doc = json.load(f)
    assert doc["chosen"] is None  # uncalibrated: the defaults are drift_smooth's
    assert (drs.DEFAULT_RANGE_KNOT_BLOCKS, drs.DEFAULT_RANGE_RADIUS, drs.DEFAULT_RANGE_BEND_COST) == \
        (ds.DEFAULT_KNOT_BLOCKS, ds.DEFAULT_RADIUS, ds.DEFAULT_BEND_COST) == \
        tuple(doc["shipped_uncalibrated"][x] for x in ("knot_blocks", "radius", "bend_cost"))
    k = drs.DEFAULT_BLOCK_SAMPLES
    probs = [cut_drift.make_problem(seed, duration_s=600.0, fixed=True) for seed in (0, 1)]
    truth = np.concatenate([cut_drift.block_truth(p, (p.sub.size + k - 1) // k, k) for p in probs])
    lo = int(np.floor((truth.min() - 4096) / 2048)) * 2048
    hi = int(np.ceil((truth.max() + 4096) / 2048)) * 2048
    assert hi > 131072
    items = [(p.ref.astype(float), p.track) for p in probs]
    got = drs.smooth_cut_sync(items, (lo, hi))
    plain = dr.cut_drift_sync(items, (lo, hi))
    db, best, _ = ca.solve_ratios_windowless(items, list(candidate_ratios()))
    fits = drs.smooth_align_range_batch(db.select_candidates(best), (lo, hi))
    moved = 0
    for p, g, x, f in zip(probs, got, plain, fits):
        assert (g.ratio, g.ratio_index, g.global_offset, g.lag_range) == (x.ratio, x.ratio_index, x.global_offset, (lo, hi))
        assert np.array_equal(g.block_offsets, x.block_offsets) and np.array_equal(g.block_jump, x.block_jump)
        assert _bits([g.total])[0] == _bits([x.total])[0] and np.array_equal(g.cue_segment, x.cue_segment)
        assert np.array_equal(g.smooth_offsets, f.smooth_offsets) and g.smooth_offsets.dtype == np.int32
        assert [s.knots for s in g.smooth_segments] == [s.knots for s in f.segments] and len(g.smooth_segments) == len(g.segments)
        cs, ce, which = ds.map_cues_smooth(p.pair.start_us, p.pair.end_us, g.ratio, f, k)
        assert np.array_equal(g.cue_start_us, cs) and np.array_equal(g.cue_end_us, ce)
        assert np.array_equal(g.cue_end_us - g.cue_start_us, x.cue_end_us - x.cue_start_us)
        assert g.smooth_offsets.min() >= lo and g.smooth_offsets.max() <= hi
        moved += int((g.smooth_offsets != g.block_offsets).sum())
    assert moved >= 10  # the fit did something
    ca.clear_plan_cache()
    dr.clear_plan_cache()
    drs.clear_plan_cache()
