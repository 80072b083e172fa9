"""Drift-tolerant alignment over a lag range on the device (csrc/ffs_drift_range.h via ffsubsync_amd.drift_range): bit
for bit against the numpy model tests/drift_range_model.py, a path that steps across a tile edge, bit for bit against
ffs_align_split_range_batch at max_step = 0 and against ffs_align_drift_batch at [-W+1, W], the error paths, and
cut_drift_sync on subtitles for another cut that also drift.  That the model's path IS the maximum over all lag paths,
and that the device reaches it at the shapes this module does not run, is pinned in tests/test_gpu_drift_optimum.py
against tests/drift_path_reference.py, which shares nothing with the model."""
import ctypes
import json
import os

import numpy as np
import pytest

import cut_model as cm
import drift_range_model as drm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SETTING = (60.0, 2, 1.0)  # split_penalty, max_step, step_cost of the batched second pass


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _device_pairs(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _small_problems(n=40):
    """Seeded problems of mixed sizes (R < S and R > S, S not a multiple of K), non-default levels, penalties from 0 to
    inf, max_step 0..7, step costs 0..128 and lag ranges of six kinds -- the full overlap range, asymmetric ranges
    around 0, ranges with lag_lo > 0, ranges wider than 262 144 lags reaching past both overlap edges, [-W+1, W], and
    ranges with no overlap at all -- plus six more with L = 1, L = 5 <= max_step and L one less / one more than a
    multiple of 64 and of 2048."""
    out = []
    extra = [(1, 3), (5, 7), (63, 2), (65, 5), (2047, 1), (2049, 2), (4097, 7)]
    for seed in range(n + len(extra)):
        rng = np.random.RandomState(9100 + seed)
        R, S = int(rng.randint(700, 9000)), int(rng.randint(700, 9000))
        if seed < n and seed % 6 == 3:
            S = 700 + S % 1800  # the wide ranges: few blocks, so the model's rows of 263 k lags stay quick
        k = int(rng.choice([256, 512, 1024]))
        p = [0.0, 0.5, 60.0, 900.0, np.inf][seed % 5]
        s = seed % 8
        q = [0.0, 1.0, 16.0, 128.0][(seed // 8 + seed) % 4]
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25)][(seed // 3) % 4]
        seg = np.maximum(1, rng.geometric(1.0 / 50.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        sh0 = int(rng.randint(-S // 2, R // 2))
        # the second half drifts away from the first: one sample every `every` samples, then a break
        every = int(rng.randint(150, 900))
        cut = int(rng.randint(0, S + 1))
        i = np.arange(S)
        idx = i + sh0 + i // every + np.where(i < cut, 0, int(rng.randint(-1500, 1501)))
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        kind = seed % 6
        if seed >= n:
            length, s = extra[seed - n]
            lo = sh0 - int(rng.randint(0, length))  # around the true offset
            hi = lo + length - 1
        elif kind == 0:
            lo, hi = cm.full_range(R, S)
        elif kind == 1:
            lo, hi = -int(rng.randint(1, S)), int(rng.randint(0, 3 * R))
        elif kind == 2:
            lo = int(rng.randint(1, R))
            hi = lo + int(rng.randint(0, 4000))
        elif kind == 3:
            lo = -S - int(rng.randint(0, 2000))
            hi = lo + 262144 + int(rng.randint(1, 3000))
        elif kind == 4:
            w = int(rng.randint(1, 5000))
            lo, hi = -w + 1, w
        else:
            lo = R + int(rng.randint(0, 5000)) if seed % 2 else -S - int(rng.randint(5000, 9000))
            hi = lo + int(rng.randint(0, 5000))
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, k=k, p=p, s=s, q=q, lo=lo, hi=hi))
    return out


SMALL = _small_problems()


def _model(pr, p=None, s=None, q=None):
    return drm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"], pr["p"] if p is None else p,
                     pr["s"] if s is None else s, pr["q"] if q is None else q)


def _same(res, want):
    offs, scores, jump, total = want
    return (np.array_equal(res.block_offsets, offs) and np.array_equal(_bits(res.block_scores), _bits(scores))
            and np.array_equal(res.block_jump, jump) and _bits([res.total])[0] == _bits([total])[0])


def test_device_equals_model_bit_for_bit():
    """Every problem in a call of its own, then all of them per K in one batch of several sub-batches (pairs_in_flight
    3) at one setting."""
    from ffsubsync_amd import drift_range as dr

    lens = [pr["hi"] - pr["lo"] + 1 for pr in SMALL]
    assert any(n > 262144 for n in lens) and any(pr["lo"] > 0 for pr in SMALL)
    assert {1, 5, 63, 65, 2047, 2049} <= set(lens) and any(n <= pr["s"] for n, pr in zip(lens, SMALL))
    assert {pr["s"] for pr in SMALL} == set(range(8)) and {pr["q"] for pr in SMALL} == {0.0, 1.0, 16.0, 128.0}
    bad, stepped, jumped = [], 0, 0
    for i, pr in enumerate(SMALL):
        want = _model(pr)
        stepped += int(((np.diff(want[0]) != 0) & (want[2][1:] == 0)).any())
        jumped += int(want[2].any())
        db = _device_pairs([(pr["ref"], pr["sub"])])
        got = dr.drift_align_range_batch(db, (pr["lo"], pr["hi"]), pr["k"], pr["p"], pr["s"], pr["q"])[0]
        if not _same(got, want):
            bad.append(i)
    assert not bad, bad
    assert stepped >= 8 and jumped >= 8, (stepped, jumped)  # the set exercises both kinds of move
    p, s, q = BATCH_SETTING
    for k in (256, 512, 1024):
        idx = [i for i, pr in enumerate(SMALL) if pr["k"] == k]
        db = _device_pairs([(SMALL[i]["ref"], SMALL[i]["sub"]) for i in idx])
        dr.clear_plan_cache()
        got = dr.drift_align_range_batch(db, [(SMALL[i]["lo"], SMALL[i]["hi"]) for i in idx], k, p, s, q, pairs_in_flight=3)
        for i, g in zip(idx, got):
            assert _same(g, _model(SMALL[i], p, s, q)), (k, i)
    dr.clear_plan_cache()


@pytest.mark.parametrize("direction", [1, -1])
def test_path_steps_across_a_tile_edge(direction):
    """A subtitle whose true offset moves one sample per block from lag index 2040 to 2056 (or back): the path is made
    of steps, no jump, and passes between lag indices 2047 and 2048 -- the edge of a 2048-lag tile and of a wave."""
    from ffsubsync_amd import drift_range as dr

    k, n_blocks = 256, 20
    rng = np.random.RandomState(77)
    rb = rng.rand(12000) < 0.5
    lag_lo = 1000 - 2040
    first = 2040 if direction > 0 else 2056
    j_true = first + direction * np.clip(np.arange(n_blocks) - 1, 0, 16)
    i = np.arange(n_blocks * k)
    sb = rb[i + lag_lo + j_true[i // k]]
    rb[0], rb[1], sb[0], sb[1] = True, False, True, False
    lo, hi = lag_lo, lag_lo + 4095  # two tiles
    want = drm.solve(rb, sb, (0.0, 1.0), (0.0, 1.0), k, lo, hi, 1e6, 2, 1.0)
    db = _device_pairs([(rb.astype(float), sb.astype(float))])
    got = dr.drift_align_range_batch(db, (lo, hi), k, 1e6, 2, 1.0)[0]
    assert _same(got, want)
    j = got.block_offsets.astype(np.int64) - lo
    assert np.array_equal(j, j_true)
    assert not got.block_jump.any() and (np.diff(j) == direction).sum() == 16
    a, b = (2047, 2048) if direction > 0 else (2048, 2047)
    assert any(j[x] == a and j[x + 1] == b for x in range(n_blocks - 1))
    assert len(got.segments) == 1
    dr.clear_plan_cache()


def test_max_step_zero_equals_split_align_range_batch():
    """The small set at max_step = 0: offsets, scores and total byte-identical to the range split's, block_jump = the
    offset changes."""
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr

    for k in (256, 512, 1024):
        idx = [i for i, pr in enumerate(SMALL) if pr["k"] == k]
        db = _device_pairs([(SMALL[i]["ref"], SMALL[i]["sub"]) for i in idx])
        ranges = [(SMALL[i]["lo"], SMALL[i]["hi"]) for i in idx]
        for p in (0.5, 60.0):
            want = ca.split_align_range_batch(db, ranges, k, p)
            got = dr.drift_align_range_batch(db, ranges, k, p, 0, 7.0)
            for i, g, x in zip(idx, got, want):
                assert np.array_equal(g.block_offsets, x.block_offsets), (k, p, i)
                assert np.array_equal(_bits(g.block_scores), _bits(x.block_scores)) and g.total == x.total, (k, p, i)
                assert np.array_equal(g.block_jump[1:], (np.diff(g.block_offsets) != 0).astype(np.uint8)), (k, p, i)
                assert g.block_jump[0] == 0
    ca.clear_plan_cache()
    dr.clear_plan_cache()


def test_symmetric_range_equals_drift_align_batch():
    """workloads/drift.py seeds 0..15, 2 h, W = 6000, drift_align's defaults: all four outputs byte-identical."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import split_align as sa
    from workloads import drift

    probs = [drift.make_problem(seed) for seed in range(16)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    w = 6000
    want = da.drift_align_batch(db, w)
    got = dr.drift_align_range_batch(db, (-w + 1, w), split_penalty=sa.DEFAULT_SPLIT_PENALTY, max_step=da.DEFAULT_MAX_STEP,
                                     step_cost=da.DEFAULT_STEP_COST)
    moved = 0
    for i, (g, x) in enumerate(zip(got, want)):
        assert np.array_equal(g.block_offsets, x.block_offsets) and np.array_equal(g.block_jump, x.block_jump), i
        assert np.array_equal(_bits(g.block_scores), _bits(x.block_scores)), i
        assert _bits([g.total])[0] == _bits([x.total])[0], i
        moved += int((np.diff(g.block_offsets) != 0).sum())
    assert moved > 100  # the paths do drift
    da.clear_plan_cache()
    dr.clear_plan_cache()


def test_refused_calls_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native

    lib = _native.load()
    plan = _native.DriftRangePlan(2, 8, 5000, 4096, 2)
    assert plan.workspace_bytes >= 2 * (8 * 5000 * 3 / 8 + 2 * 5000 * 8)
    words = torch.zeros(256, dtype=torch.int32, device="cuda")
    ptr = np.array([words.data_ptr()], dtype=np.uint64)
    n_r, n_s = np.array([4000], np.int64), np.array([3000], np.int64)
    lo, hi = np.array([0.0]), np.array([1.0])
    mark = 0x5A
    offs = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    scores = torch.full((8,), 77.25, dtype=torch.float64, device="cuda")
    jumps = torch.full((8,), mark, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), 77.25, dtype=torch.float64, device="cuda")

    def call(handle=plan.handle, n=1, n_s=n_s, hi=hi, k=512, rng=(-1000, 2000), p=8192.0, s=2, q=64.0, jumps_ptr=None):
        l0, l1 = np.array([rng[0]], np.int64), np.array([rng[1]], np.int64)
        return lib.ffs_align_drift_range_batch(handle, n, ptr.ctypes.data, n_r.ctypes.data, lo.ctypes.data,
                                               hi.ctypes.data, ptr.ctypes.data, n_s.ctypes.data, lo.ctypes.data,
                                               hi.ctypes.data, k, l0.ctypes.data, l1.ctypes.data, p, s, q, offs.data_ptr(),
                                               scores.data_ptr(), jumps.data_ptr() if jumps_ptr is None else jumps_ptr,
                                               total.data_ptr(), None)

    inv, empty = -1, -5  # FFS_E_INVALID, FFS_E_EMPTY
    assert call(rng=(5, 4)) == inv and b"lag range" in lib.ffs_last_error()  # bad range
    assert call(rng=(-2 ** 31, 0)) == inv
    assert call(rng=(0, 5000)) == inv and b"max_lags" in lib.ffs_last_error()  # 5001 lags: wider than the plan
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
    assert call(jumps_ptr=ctypes.c_void_p(0)) == inv
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((offs == 0x5A5A5A5A).all()) and bool((scores == 77.25).all()) and bool((jumps == mark).all())
    assert float(total[0]) == 77.25
    # and the accepted calls write them
    assert call() == 0 and call(s=0) == 0 and call(q=0.0) == 0 and call(p=float("inf")) == 0 and call(rng=(0, 4999)) == 0
    torch.cuda.synchronize()
    assert int(jumps[:6].max()) <= 1 and float(total[0]) != 77.25  # 6 blocks
    plan.close()
    handle = ctypes.c_void_p()
    assert lib.ffs_drift_range_plan_create(0, 1, 8, 5000, 4096, 8, ctypes.byref(handle)) == inv
    assert lib.ffs_drift_range_plan_create(0, 1, 8, 5000, 4096, -1, ctypes.byref(handle)) == inv
    sizes = []
    for cap in (0, 1, 2, 3, 4, 7):
        pl = _native.DriftRangePlan(1, 64, 64 * 1024, 4096, cap)
        sizes.append(pl.workspace_bytes)
        pl.close()
    planes = np.diff(sizes) // (64 * 64 * 1024 // 8)  # one more plane at 1, 2 and 4
    assert list(planes) == [1, 1, 0, 1, 0], sizes


# Steep subset (eps = +-6e-4, no wobble) of workloads/cut_drift.py, 1 h, full range, the defaults: the first 8 seeds whose
# nominal ratio stays the candidate nearest to the clock's real ratio, ratio * (1 + eps).  On the others (3, 4, 7, 9 ...)
# the residual 6e-4 points at a candidate 1e-3 away, the file is 4e-4 from THAT one, and the seven-ratio solve rightly
# returns it (seed 3 on the device: 1.0 for a clock at 1.0004, nominal 1.001): "the ratio is the true one" has no meaning
# there, and the workload's truth is in samples of the nominal candidate.
# The floor on every seed's gain (range split error / range drift error, blocks more than 2 from a true break) is the
# least gain the CPU model shows on these seeds at the default step cost (profiles/drift_range_calibration.json, set
# "steep"), less 10 % for the seven-ratio solve in front (the device DP equals the model bit for bit).
# The model on these seeds at step cost 64: range split error 18.73 18.97 13.72 17.94 14.94 18.01 14.58 13.28 samples,
# range drift error 3.51 3.20 3.62 2.85 3.36 2.68 4.02 3.57, gain 5.34 5.93 3.79 6.29 4.44 6.72 3.63 3.72: floor
# 0.9 * 3.63 = 3.27.
SYNC_SEEDS = (0, 1, 2, 5, 6, 8, 14, 15)
GAIN_MARGIN = 0.9


def _calibrated_gains():
    from ffsubsync_amd import drift_range as dr

    with open(os.path.join(ROOT, "profiles", "drift_range_calibration.json")) as f:
        doc = json.load(f)
    assert doc["chosen"]["step_cost"] == dr.DEFAULT_RANGE_STEP_COST and doc["chosen"]["max_step"] == 2
    line = [l for l in doc["summary"] if l["step_cost"] == dr.DEFAULT_RANGE_STEP_COST][0]
    return {int(s): g for s, g in line["steep"]["gain_by_seed"].items()}


def test_cut_drift_sync_beats_the_range_split_on_every_seed():
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import cut_drift

    gains = _calibrated_gains()
    assert list(SYNC_SEEDS) == cut_drift.steep_seeds(8)
    assert set(SYNC_SEEDS) <= set(gains) and len(SYNC_SEEDS) >= 8
    floor = GAIN_MARGIN * min(gains[s] for s in SYNC_SEEDS)
    assert floor > 1.0, gains  # the model improves every seed of the subset
    k = dr.DEFAULT_BLOCK_SAMPLES
    probs = [cut_drift.make_problem(seed, fixed=True) for seed in SYNC_SEEDS]
    for p in probs:
        assert abs(p.eps) == 6e-4 and cut_drift.nominal_ratio_is_nearest(p)
        assert np.abs(cut_drift.block_truth(p, (p.sub.size + k - 1) // k, k)).max() > 131072
    items = [(p.ref.astype(float), p.track) for p in probs]
    got = dr.cut_drift_sync(items)
    db, best, _ = ca.solve_ratios_windowless(items, list(candidate_ratios()))
    split = ca.split_align_range_batch(db.select_candidates(best))
    rows = []
    for p, g, x, bi in zip(probs, got, split, best):
        assert g.ratio_index == p.ratio_index == int(bi), p.seed
        assert g.lag_range == ca.full_range(p.ref.size, g.segments[-1].end_sample)
        assert g.cue_start_us.size == p.pair.start_us.size and g.cue_segment.max() < len(g.segments)
        e_split = cut_drift.mean_block_error(p, x.block_offsets, k, exclude=2)
        e_drift = cut_drift.mean_block_error(p, g.block_offsets, k, exclude=2)
        rows.append((p.seed, round(e_split, 2), round(e_drift, 2), round(e_split / e_drift, 2), round(gains[p.seed], 2)))
    print("seed, split error, drift error (samples), gain, the model's gain:", rows, "floor %.2f" % floor)
    assert all(r[2] < r[1] for r in rows), rows
    assert all(r[1] / r[2] >= floor for r in rows), (floor, rows)
    ca.clear_plan_cache()
    dr.clear_plan_cache()


def test_clean_cuts_equal_the_range_split():
    """The inserts without drift: the range drift solve at the defaults returns the range split's block offsets."""
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr
    from workloads import cut_drift

    probs = [cut_drift.make_problem(seed, clean=True) for seed in range(4)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    for p, g, x in zip(probs, dr.drift_align_range_batch(db), ca.split_align_range_batch(db)):
        assert np.array_equal(g.block_offsets, x.block_offsets), p.seed
        assert np.abs(g.block_offsets).max() > 131072
    ca.clear_plan_cache()
    dr.clear_plan_cache()
