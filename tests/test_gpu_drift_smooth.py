"""The smooth drift fit on the device (csrc/ffs_drift_smooth.h via ffsubsync_amd.drift_smooth): bit for bit against the
numpy model tests/drift_smooth_model.py on every output; the drift outputs against drift_align_batch before and after the
workspace has grown; the M = 1, R = 0 identity; long pairs, batching, the C entry point's error returns, and smooth_sync
end to end against drift_sync."""
import ctypes

import numpy as np
import pytest

import drift_smooth_model as dsm
from test_gpu_drift import SYNC_SEEDS, _bits, _device_pairs, _fuzz_problems as _drift_fuzz_problems, _same
from test_gpu_drift_report import _edge_problem

pytestmark = pytest.mark.gpu

FP_FIELDS = ("fit_total", "line_score", "bend_total")
INT_FIELDS = ("n_knots", "reserved")


def _fuzz_problems(n=96):
    """test_gpu_drift's fuzz set (K in {256, 1024, 4096}, W from 40 to 6000, P in {0, 100, 8192, inf} -- P = 0 gives a
    segment per block --, levels other than 0/1) plus three problems whose path touches the window's edge (candidates
    outside the window, blocks that overlap the reference only in part); knot_blocks, radius and bend_cost vary with the
    problem."""
    out = _drift_fuzz_problems(n) + [_edge_problem(3, 256, 40), _edge_problem(5, 1024, 63), _edge_problem(4, 256, 200)]
    for i, pr in enumerate(out):
        pr["m"] = [1, 2, 3, 4, 16, 256][i % 6]
        pr["r"] = [0, 1, 2, 5, 16][i % 5]
        pr["lam"] = [0.0, 0.5, 8.0, 64.0, 1e6][(i // 2) % 5]
    return out


def _model(pr):
    return dsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], pr["m"],
                     pr["r"], pr["lam"])


def _diff(got, want):
    bad = [f for f in FP_FIELDS if not np.array_equal(_bits(got[f]), _bits(want[f]))]
    return bad + [f for f in INT_FIELDS if not np.array_equal(got[f], want[f])]


def _run(pr, **kw):
    from ffsubsync_amd import drift_smooth as ds

    return ds.smooth_align_batch(_device_pairs([(pr["ref"], pr["sub"])]), pr["w"], pr["k"], pr["p"], pr["s"], pr["q"],
                                 pr["m"], pr["r"], pr["lam"], raw=True, **kw)


def test_device_equals_the_model_bit_for_bit():
    from ffsubsync_amd import _native

    assert set(FP_FIELDS) | set(INT_FIELDS) == set(_native.SMOOTH_SEGMENT_DTYPE.names)
    bad = []
    moved = one_block = many_knots = many_segments = clipped = 0
    for i, pr in enumerate(_fuzz_problems()):
        res, smooth, knot, recs, counts = _run(pr)
        want_solve, want_smooth, want_knot, want = _model(pr)
        n, nb = len(want), want_smooth.size
        moved += int((want_smooth != want_solve[0]).sum())
        one_block += int((want["n_knots"] == 1).sum())
        many_knots += int((want["n_knots"] >= 4).sum())
        many_segments += n > 8
        clipped += int(np.abs(want_solve[0]).max() + pr["r"] > pr["w"] - 1)
        if not _same(res[0], want_solve) or int(counts[0]) != n:
            bad.append((i, "solve", int(counts[0]), n))
            continue
        d = _diff(recs[0, :n], want)
        if not np.array_equal(smooth[0, :nb], want_smooth):
            d.append("smooth_offset")
        if not np.array_equal(knot[0, :nb], want_knot):
            d.append("knot")
        if d or recs[0, n:].tobytes().strip(b"\0") or smooth[0, nb:].any() or knot[0, nb:].any():
            bad.append((i, pr["k"], pr["w"], pr["p"], pr["m"], pr["r"], pr["lam"], n, d))
    assert not bad, bad[:5]
    # the set holds what the fit has to get right
    assert moved >= 50 and one_block >= 20 and many_knots >= 10 and many_segments >= 3 and clipped >= 3, \
        (moved, one_block, many_knots, many_segments, clipped)


def test_one_block_knots_without_radius_return_the_path_on_the_device():
    for pr in _fuzz_problems(24):
        pr = dict(pr, m=1, r=0, lam=64.0)
        res, smooth, knot, recs, counts = _run(pr)
        nb = res[0].block_offsets.size
        assert np.array_equal(smooth[0, :nb], res[0].block_offsets) and knot[0, :nb].all()
        assert [int(x) for x in recs[0, :counts[0]]["n_knots"]] == [s.end_block - s.first_block for s in res[0].segments]


def test_batches_larger_than_pairs_in_flight_and_drift_outputs_equal_drift_align():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds

    base = [pr for pr in _drift_fuzz_problems(60) if pr["k"] == 256][:20]
    probs = []
    for i in range(50):
        pr = base[i % len(base)]
        probs.append(dict(pr, sub=pr["sub"][: pr["sub"].size - 37 * (i // len(base))], ref=np.roll(pr["ref"], 11 * i)))
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    assert len(set(int(x) for x in db.lens[:, 1])) > 10
    for w, p, s, q, m, r, lam, pif in ((1000, 100.0, 2, 0.5, 2, 3, 4.0, 16), (200, np.inf, 7, 0.0, 3, 16, 0.0, 7),
                                       (511, 0.0, 1, 0.0, 1, 2, 1.0, None)):
        ds.clear_plan_cache()
        drift = da.drift_align_batch(db, w, 256, p, s, q)
        many = ds.smooth_align_batch(db, w, 256, p, s, q, m, r, lam, pairs_in_flight=pif)
        ds.clear_plan_cache()
        for i, (a, got) in enumerate(zip(drift, many)):
            b = got.drift
            assert np.array_equal(a.block_offsets, b.block_offsets) and np.array_equal(a.block_jump, b.block_jump), i
            assert np.array_equal(_bits(a.block_scores), _bits(b.block_scores)) and _bits([a.total])[0] == _bits([b.total])[0]
            assert [(x.first_block, x.end_block) for x in got.segments] == [(y.first_block, y.end_block) for y in b.segments]
            if i % 7 == 0:
                one = ds.smooth_align_batch(_device_pairs([(probs[i]["ref"], probs[i]["sub"])]), w, 256, p, s, q, m, r, lam)[0]
                assert np.array_equal(one.smooth_offsets, got.smooth_offsets) and np.array_equal(one.knot, got.knot), i
                assert [(x.knots, _bits([x.fit_total, x.line_score, x.bend_total]).tolist()) for x in one.segments] == \
                    [(x.knots, _bits([x.fit_total, x.line_score, x.bend_total]).tolist()) for x in got.segments], i
    ds.clear_plan_cache()


def test_two_hour_pairs_equal_the_model_at_the_defaults():
    """Two-hour problems of workloads/drift.py at the defaults: two at +-60 s, one at +-5 min with an inserted break (two
    segments), one at +-10 min."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    cases = [(drift.make_problem(3), 6000), (drift.make_problem(4), 6000),
             (drift.make_problem(5, insert_break=True), 30000), (drift.make_problem(6), 60000)]
    for pr, w in cases:
        db = _device_pairs([(pr.ref.astype(float), pr.sub.astype(float) * pr.sub_hi)])
        res, smooth, knot, recs, counts = ds.smooth_align_batch(db, w, raw=True)
        want_solve, want_smooth, want_knot, want = dsm.solve(
            pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), 1024, w, da.DEFAULT_SPLIT_PENALTY, da.DEFAULT_MAX_STEP,
            da.DEFAULT_STEP_COST, ds.DEFAULT_KNOT_BLOCKS, ds.DEFAULT_RADIUS, ds.DEFAULT_BEND_COST)
        nb = want_smooth.size
        assert _same(res[0], want_solve), (pr.seed, w)
        assert int(counts[0]) == len(want) and not _diff(recs[0, :len(want)], want), (pr.seed, w, _diff(recs[0, :len(want)], want))
        assert np.array_equal(smooth[0, :nb], want_smooth) and np.array_equal(knot[0, :nb], want_knot), (pr.seed, w)
        assert np.count_nonzero(want_smooth != want_solve[0]) > 100  # the fit moved the path
        path, fitted = drift.mean_block_error(pr, want_solve[0], 1024), drift.mean_block_error(pr, want_smooth, 1024)
        print("seed %d W %d: path %.2f, fitted %.2f samples" % (pr.seed, w, path, fitted))
        if pr.break_ref_s is not None:
            assert len(want) == 2
        ds.clear_plan_cache()


def test_smooth_workspace_is_added_by_the_first_smooth_call_only():
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
    smooth = torch.zeros(n * max_b, dtype=torch.int32, device="cuda")
    knot = torch.zeros(n * max_b, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(n * max_b * _native.SMOOTH_SEGMENT_BYTES // 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.smooth(*db.pair_arrays(), k, w, 100.0, 2, 0.5, 2, 16, 4.0, *o, smooth, knot, rec, cnt)
    grown = plan.workspace_bytes
    mb = (max_b + 15) // 16 * 16
    assert 2 * mb * 33 * 33 * 9 <= grown - size <= 2 * mb * (33 * 33 * 9 + 36) + 256
    assert [x.cpu().numpy().tobytes() for x in o] == before  # the smooth call's drift outputs
    assert plain() == before and plan.workspace_bytes == grown  # and the drift call after the workspace has grown
    plan.smooth(*db.pair_arrays(), k, w, 100.0, 2, 0.5, 1, 0, 0.0, *o, smooth, knot, rec, cnt)
    assert plan.workspace_bytes == grown and [x.cpu().numpy().tobytes() for x in o] == before
    recs = rec.cpu().numpy().view(_native.SMOOTH_SEGMENT_DTYPE).reshape(n, max_b)
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
    smooth = torch.full((9,), 66, dtype=torch.int32, device="cuda")
    knot = torch.full((8,), 5, dtype=torch.uint8, device="cuda")
    rec = torch.full((8 * _native.SMOOTH_SEGMENT_BYTES // 8 + 1,), 123, dtype=torch.int64, device="cuda")
    cnt = torch.full((2,), 55, dtype=torch.int32, device="cuda")
    outs = (offs, scores, jumps, total, smooth, knot, rec, cnt)
    before = [x.cpu().numpy().tobytes() for x in outs]
    size = plan.workspace_bytes

    def call(handle=plan.handle, n=1, n_s=n_s, hi=hi, k=512, w=1000, p=8192.0, s=2, q=64.0, m=2, r=3, lam=8.0,
             smooth_ptr=None, knot_ptr=None, rec_ptr=None, cnt_ptr=None):
        return lib.ffs_align_drift_smooth_batch(
            handle, n, ptr.ctypes.data, n_r.ctypes.data, lo.ctypes.data, hi.ctypes.data, ptr.ctypes.data, n_s.ctypes.data,
            lo.ctypes.data, hi.ctypes.data, k, w, p, s, q, m, r, lam, offs.data_ptr(), scores.data_ptr(), jumps.data_ptr(),
            total.data_ptr(), smooth.data_ptr() if smooth_ptr is None else smooth_ptr,
            knot.data_ptr() if knot_ptr is None else knot_ptr, rec.data_ptr() if rec_ptr is None else rec_ptr,
            cnt.data_ptr() if cnt_ptr is None else cnt_ptr, None)

    inv, empty = -1, -5  # FFS_E_INVALID, FFS_E_EMPTY
    assert call(n=0) == 0
    assert call(handle=None) == inv and call(n=-1) == inv
    assert call(m=0) == inv and b"knot_blocks" in lib.ffs_last_error()
    assert call(m=257) == inv and call(m=-3) == inv
    assert call(r=-1) == inv and b"radius" in lib.ffs_last_error()
    assert call(r=17) == inv
    for lam in (-1.0, float("nan"), float("inf")):
        assert call(lam=lam) == inv and b"bend_cost" in lib.ffs_last_error()
    null = ctypes.c_void_p(0)
    assert call(smooth_ptr=null) == inv and call(knot_ptr=null) == inv and call(rec_ptr=null) == inv and call(cnt_ptr=null) == inv
    assert call(smooth_ptr=ctypes.c_void_p(smooth.data_ptr() + 2)) == inv and b"misaligned" in lib.ffs_last_error()
    assert call(rec_ptr=ctypes.c_void_p(rec.data_ptr() + 4)) == inv
    assert call(cnt_ptr=ctypes.c_void_p(cnt.data_ptr() + 2)) == inv
    assert call(s=-1) == inv and call(s=8) == inv
    assert call(q=float("nan")) == inv and call(p=-1.0) == inv
    assert call(k=500) == inv and call(w=0) == inv and call(w=1001) == inv
    assert call(n_s=np.array([0], np.int64)) == empty
    assert call(n_s=np.array([4097], np.int64)) == inv
    assert call(hi=np.array([np.inf])) == inv
    torch.cuda.synchronize()
    assert [x.cpu().numpy().tobytes() for x in outs] == before  # every refusal came before any launch
    assert plan.workspace_bytes == size  # ... and before the workspace grew
    assert call() == 0 and call(m=256, r=16, lam=0.0, s=7, q=0.0, p=float("inf")) == 0 and call(m=1, r=0) == 0
    torch.cuda.synchronize()
    assert int(cnt.cpu()[0]) >= 1 and int(cnt.cpu()[1]) == 55 and int(smooth.cpu()[8]) == 66
    assert plan.workspace_bytes > size
    plan.close()
    with pytest.raises(ValueError):
        from ffsubsync_amd import drift_smooth as ds

        ds.smooth_align_batch(None, 100, radius=17)


def _errors(results, probs):
    return [float(np.mean(np.abs(r.cue_start_us - p.true_start_us))) / 1e4 for r, p in zip(results, probs)]


def test_smooth_sync_beats_drift_sync_on_every_drifting_problem():
    """The twelve drifting problems of tests/test_gpu_drift.py, none left out: the mean cue-start error of smooth_sync is
    strictly below drift_sync's on every one."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    assert SYNC_SEEDS == tuple(range(12))
    probs = [drift.make_problem(seed) for seed in SYNC_SEEDS]
    items = [(p.ref.astype(float), p.track) for p in probs]
    plain = da.drift_sync(items, max_offset_seconds=60)
    got = ds.smooth_sync(items, max_offset_seconds=60)
    rows = [(p.seed, round(a, 3), round(b, 3)) for p, a, b in zip(probs, _errors(plain, probs), _errors(got, probs))]
    print("seed, drift_sync error, smooth_sync error (samples):", rows)
    for p, a, b in zip(probs, plain, got):
        assert (b.ratio, b.ratio_index, b.global_offset, b.total) == (a.ratio, a.ratio_index, a.global_offset, a.total)
        assert [(s.first_block, s.end_block, s.first_offset, s.last_offset) for s in b.segments] == \
            [(s.first_block, s.end_block, s.first_offset, s.last_offset) for s in a.segments]
        assert len(b.smooth_segments) == len(b.segments) and np.array_equal(b.cue_segment, a.cue_segment)
        assert np.array_equal(b.cue_end_us - b.cue_start_us, a.cue_end_us - a.cue_start_us)
        assert all(len(s.ratios) == len(s.knots) - 1 for s in b.smooth_segments)
    assert all(r[2] < r[1] for r in rows), rows


def test_smooth_sync_on_clean_problems_gives_drift_sync_times_exactly():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    probs = [drift.make_problem(seed, clean=True) for seed in range(8)]
    items = [(p.ref.astype(float), p.track) for p in probs]
    for a, b in zip(da.drift_sync(items, max_offset_seconds=60), ds.smooth_sync(items, max_offset_seconds=60)):
        assert np.array_equal(a.cue_start_us, b.cue_start_us) and np.array_equal(a.cue_end_us, b.cue_end_us)
        assert (a.ratio, a.global_offset) == (b.ratio, b.global_offset)
        assert all(r == 1.0 for s in b.smooth_segments for r in s.ratios)
