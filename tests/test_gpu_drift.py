"""Drift-tolerant alignment on the device (csrc/ffs_drift.h via ffsubsync_amd.drift_align): bit for bit against the numpy
model tests/drift_model.py on block offsets, jump flags, block scores and totals; max_step = 0 against split_align_batch;
long pairs, batching, drift_sync end to end against split_sync, and the C entry point's error returns.  That the model's
path IS the maximum over all lag paths, and that the device reaches it at the shapes this module does not run (W = 1 and
2, 2W = 262 144, K off the powers of two, K = 32 768), is pinned in tests/test_gpu_drift_optimum.py against
tests/drift_path_reference.py, which shares nothing with the model."""
import ctypes

import numpy as np
import pytest

import drift_model as dm

pytestmark = pytest.mark.gpu

# drift_sync against split_sync: two-hour problems of workloads/drift.py (seeds as drawn), +-60 s.  The device equals
# the model bit for bit, so the first 12 seeds were run through the two models on the CPU (ratio by the windowed
# FFTAligner score over the seven candidates, then split_model / drift_model at the defaults, then map_cues); the seeds
# below are those on which the MODELS meet "at most half of split's error".  None was dropped for any other reason.
SYNC_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _device_pairs(problems):
    """DeviceBatch (one candidate per pair) from host (ref values, sub values) pairs of two-level float vectors."""
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _fuzz_problems(n=96):
    """Seeded small problems: K in {256, 1024, 4096}, W from 40 to 6000, R != S, lengths not multiples of 32 or K,
    sub_hi = min(1/ratio, 1) levels, P in {0, 100, 8192, inf}, max_step in {0, 1, 2, 7}, step_cost in {0, 0.5, 64, 1e6}.
    The default 0/1 levels give integer scores: with step_cost = 0 (and 0.5, 64) exact ties between STAY, the moves and
    JUMP are common, so these cases test the tie order on the device."""
    from ffsubsync_amd.constants import candidate_ratios

    ratios = list(candidate_ratios())
    out = []
    for seed in range(n):
        rng = np.random.RandomState(7000 + seed)
        k = [256, 1024, 4096][seed % 3]
        w = int([40, 63, 64, 65, 200, 511, 1000, 2500, 6000][seed % 9])
        p = [0.0, 100.0, 8192.0, np.inf][(seed // 3) % 4]
        s = [0, 1, 2, 7][(seed // 2) % 4]
        q = [0.0, 0.5, 64.0, 1e6][(seed // 5) % 4]
        R = int(rng.randint(3 * k, 14 * k)) | 1
        S = int(rng.randint(3 * k, 14 * k)) | 1
        if S % k == 0:
            S += 2
        if R == S:
            R += 2
        ratio = ratios[seed % len(ratios)]
        s_lv = (0.0, min(1.0 / ratio, 1.0))
        r_lv = [(0.0, 1.0), (0.0, 1.0), (-1.0, 2.5)][seed % 3 if seed % 7 == 0 else 0]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        # a subtitle vector that drifts against the reference: sample i meets reference sample i + shift + drift * i
        shift = int(rng.randint(-min(w, 3000) // 2, min(w, 3000) // 2 + 1))
        drift = rng.uniform(-2e-3, 2e-3)
        idx = np.arange(S) + shift + np.rint(drift * np.arange(S)).astype(np.int64)
        if seed % 4 == 1:  # and a break
            idx[S // 2:] += int(rng.randint(5, max(6, w // 3)))
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, k=k, w=w, p=p, s=s, q=q))
    return out


def _same(res, want):
    offs, scores, jump, total = want
    return (np.array_equal(res.block_offsets.astype(np.int64), offs) and np.array_equal(res.block_jump, jump)
            and np.array_equal(_bits(res.block_scores), _bits(scores)) and _bits([res.total])[0] == _bits([total])[0])


def test_device_equals_model_bit_for_bit():
    from ffsubsync_amd import drift_align as da

    bad, moved, jumped = [], 0, 0
    for i, pr in enumerate(_fuzz_problems()):
        res = da.drift_align_batch(_device_pairs([(pr["ref"], pr["sub"])]), pr["w"], pr["k"], pr["p"], pr["s"], pr["q"])[0]
        want = dm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"], pr["s"], pr["q"])
        step = np.diff(want[0]) != 0
        moved += int((step & (want[2][1:] == 0)).sum())
        jumped += int(want[2].sum())
        if not _same(res, want):
            bad.append((i, pr["k"], pr["w"], pr["p"], pr["s"], pr["q"], res.total, want[3],
                        int((res.block_offsets != want[0]).sum()), int((res.block_jump != want[2]).sum())))
        segs = da.segments_from_blocks(want[0], want[1], want[2], pr["k"], pr["sb"].size)
        assert [(s.first_block, s.end_block, s.first_offset, s.last_offset, s.score) for s in res.segments] == \
            [(s.first_block, s.end_block, s.first_offset, s.last_offset, s.score) for s in segs]
    assert not bad, bad[:5]
    assert moved > 50 and jumped > 50, (moved, jumped)  # the set exercises both kinds of move


def test_max_step_zero_equals_split_align_batch():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import split_align as sa

    probs = [pr for pr in _fuzz_problems(48) if pr["k"] == 1024]
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    for w, p in ((511, 0.0), (2500, 100.0), (6000, 8192.0), (200, np.inf)):
        split = sa.split_align_batch(db, w, 1024, p)
        drift = da.drift_align_batch(db, w, 1024, p, max_step=0, step_cost=3.0)
        for a, b in zip(split, drift):
            assert np.array_equal(a.block_offsets, b.block_offsets)
            assert np.array_equal(_bits(a.block_scores), _bits(b.block_scores))
            assert _bits([a.total])[0] == _bits([b.total])[0]
            assert np.array_equal(b.block_jump[1:], (np.diff(b.block_offsets) != 0).astype(np.uint8)) and b.block_jump[0] == 0
            assert [(s.first_block, s.end_block, s.first_offset, s.score, s.drift) for s in b.segments] == \
                [(q.first_block, q.end_block, q.offset, q.score, 0.0) for q in a.pieces]


def test_two_hour_pairs_equal_the_model():
    """Two-hour problems of workloads/drift.py at the defaults: two at +-60 s, one at +-5 min with an inserted
    break (a jump and drift in one problem), one at +-10 min."""
    from ffsubsync_amd import drift_align as da
    from workloads import drift

    cases = [(drift.make_problem(3), 6000), (drift.make_problem(4), 6000),
             (drift.make_problem(5, insert_break=True), 30000), (drift.make_problem(6), 60000)]
    for pr, w in cases:
        db = _device_pairs([(pr.ref.astype(float), pr.sub.astype(float) * pr.sub_hi)])
        res = da.drift_align_batch(db, w)[0]
        want = dm.solve(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), 1024, w, da.DEFAULT_SPLIT_PENALTY,
                        da.DEFAULT_MAX_STEP, da.DEFAULT_STEP_COST)
        assert _same(res, want), (pr.seed, w, res.total, want[3])
        if pr.break_ref_s is not None:
            assert int(res.block_jump.sum()) == 1 and len(res.segments) == 2
        assert np.count_nonzero(np.diff(res.block_offsets)) > 20  # it followed the drift


def test_batch_larger_than_pairs_in_flight_mixed_lengths_bytes_and_bits():
    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_align as da

    base = [pr for pr in _fuzz_problems(60) if pr["k"] == 256][:20]
    probs = []
    for i in range(50):
        pr = base[i % len(base)]
        cut = 37 * (i // len(base))
        probs.append(dict(pr, sub=pr["sub"][: pr["sub"].size - cut], ref=np.roll(pr["ref"], 11 * i)))
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    assert db.dtype == _native.FFS_DTYPE_U1 and len(set(int(x) for x in db.lens[:, 1])) > 10
    da.clear_plan_cache()
    many = da.drift_align_batch(db, 1000, 256, 100.0, 2, 0.5, pairs_in_flight=16)  # four sub-batches
    da.clear_plan_cache()
    for i, (pr, got) in enumerate(zip(probs, many)):
        one = da.drift_align_batch(_device_pairs([(pr["ref"], pr["sub"])]), 1000, 256, 100.0, 2, 0.5)[0]
        assert np.array_equal(got.block_offsets, one.block_offsets) and np.array_equal(got.block_jump, one.block_jump), i
        assert np.array_equal(_bits(got.block_scores), _bits(one.block_scores)) and got.total == one.total, i
    # 0/1 bytes go through to_bits(): the same records
    from workloads import synth

    specs = [synth.make_pair_spec(s, duration_s=600.0) for s in range(4)]
    idx = [sp.true_ratio_index for sp in specs]
    d_bits = synth.build_device_batch(specs, packed=True).select_candidates(idx)
    d_bytes = synth.build_device_batch(specs, packed=False).select_candidates(idx)
    assert d_bytes.dtype == _native.FFS_DTYPE_U8
    for a, b in zip(da.drift_align_batch(d_bits, 6000), da.drift_align_batch(d_bytes, 6000)):
        assert np.array_equal(a.block_offsets, b.block_offsets) and np.array_equal(a.block_jump, b.block_jump)
        assert np.array_equal(_bits(a.block_scores), _bits(b.block_scores)) and a.total == b.total


def test_drift_sync_halves_the_cue_error_of_split_sync():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    assert len(SYNC_SEEDS) >= 8 and max(SYNC_SEEDS) < 12
    probs = [drift.make_problem(seed) for seed in SYNC_SEEDS]
    items = [(p.ref.astype(float), p.track) for p in probs]
    split = sa.split_sync(items, max_offset_seconds=60)
    got = da.drift_sync(items, max_offset_seconds=60)
    rows = []
    for p, a, b in zip(probs, split, got):
        e_split = float(np.mean(np.abs(a.cue_start_us - p.true_start_us))) / 1e4  # samples of 10 ms
        e_drift = float(np.mean(np.abs(b.cue_start_us - p.true_start_us))) / 1e4
        rows.append((p.seed, a.ratio, b.ratio, round(e_split, 2), round(e_drift, 2)))
        assert b.ratio_index == a.ratio_index and b.global_offset == a.global_offset
        assert b.cue_segment.size == p.start_us.size and b.cue_segment.max() < len(b.segments)
    print("seed, ratio, ratio, split error, drift error (samples):", rows)
    assert all(r[4] <= 0.5 * r[3] for r in rows), rows


def test_drift_sync_on_clean_problems_equals_split_sync():
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    probs = [drift.make_problem(seed, clean=True) for seed in range(8)]
    items = [(p.ref.astype(float), p.track) for p in probs]
    for a, b in zip(sa.split_sync(items, max_offset_seconds=60), da.drift_sync(items, max_offset_seconds=60)):
        assert np.array_equal(a.cue_start_us, b.cue_start_us) and np.array_equal(a.cue_end_us, b.cue_end_us)
        assert (a.ratio, a.global_offset) == (b.ratio, b.global_offset)


def test_error_returns_through_ctypes():
    import torch

    from ffsubsync_amd import _native

    lib = _native.load()
    plan = _native.DriftPlan(2, 8, 2000, 4096)
    assert plan.workspace_bytes >= 2 * 8 * 2048 * 2.5
    words = torch.zeros(256, dtype=torch.int32, device="cuda")
    ptr = np.array([words.data_ptr()], dtype=np.uint64)
    n_r, n_s = np.array([4000], np.int64), np.array([3000], np.int64)
    lo, hi = np.array([0.0]), np.array([1.0])
    offs = torch.zeros(8, dtype=torch.int32, device="cuda")
    scores = torch.zeros(8, dtype=torch.float64, device="cuda")
    jumps = torch.zeros(8, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.float64, device="cuda")

    def call(handle=plan.handle, n=1, n_s=n_s, hi=hi, k=512, w=1000, p=8192.0, s=2, q=64.0, jumps_ptr=None):
        return lib.ffs_align_drift_batch(handle, n, ptr.ctypes.data, n_r.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                         ptr.ctypes.data, n_s.ctypes.data, lo.ctypes.data, hi.ctypes.data, k, w, p, s, q,
                                         offs.data_ptr(), scores.data_ptr(),
                                         jumps.data_ptr() if jumps_ptr is None else jumps_ptr, total.data_ptr(), None)

    inv, empty = -1, -5  # FFS_E_INVALID, FFS_E_EMPTY
    assert call() == 0
    assert call(n=0) == 0
    assert call(handle=None) == inv
    assert call(n=-1) == inv
    assert call(s=-1) == inv and b"max_step" in lib.ffs_last_error()
    assert call(s=8) == inv
    assert call(s=7) == 0
    for q in (-1.0, float("nan"), float("inf")):
        assert call(q=q) == inv and b"step_cost" in lib.ffs_last_error()
    assert call(q=0.0) == 0
    assert call(p=-1.0) == inv and call(p=float("nan")) == inv
    assert call(p=float("inf")) == 0
    assert call(k=500) == inv and call(k=128) == inv
    assert call(w=0) == inv and call(w=1001) == inv  # 2W beyond the plan's max_lags
    assert call(n_s=np.array([0], np.int64)) == empty
    assert call(n_s=np.array([4097], np.int64)) == inv  # beyond max_samples
    assert call(n_s=np.array([4096], np.int64), k=256) == inv  # 16 blocks beyond max_blocks
    assert call(hi=np.array([np.inf])) == inv
    assert call(jumps_ptr=ctypes.c_void_p(0)) == inv
    torch.cuda.synchronize()
    plan.close()
    with pytest.raises(ValueError):
        _native.require_gpu()
        from ffsubsync_amd import drift_align as da

        da.drift_align_batch(None, 100, max_step=8)
