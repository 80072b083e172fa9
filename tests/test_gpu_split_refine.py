"""Sample-exact break refinement on the device (csrc/ffs_split_refine.h via ffsubsync_amd.split_refine): bit for bit
against the numpy model tests/split_refine_model.py, the split's outputs untouched by a refine call, fewer wrong-piece
cues than map_cues on the seeded split workloads, refined_split_sync against checked_split_sync on clean problems, and
the error paths."""
import math

import numpy as np
import pytest

import split_refine_model as rm

pytestmark = pytest.mark.gpu


def _device_pairs(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _small_problems(n=64):
    """Seeded small problems: R < S and R > S, S not a multiple of K, lags that send samples past both reference ends,
    non-default levels, penalties from 0 (every block can be its own piece: windows clipped by midpoints) to 2000, radii
    from 1 to the maximum, margins None / 0 / 0.25 / 0.6."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(9100 + seed)
        R, S = int(rng.randint(800, 16000)), int(rng.randint(800, 16000))
        k = int(rng.choice([256, 512, 1024, 2048]))
        w = int(rng.choice([37, 300, 2500, 6000, 20000]))
        p = [0.0, 0.5, 100.0, 2000.0][seed % 4]
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25)][(seed // 3) % 4]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        sh0 = int(rng.randint(-min(w, 3000), min(w, 3000) + 1))
        sh1 = sh0 + int(rng.randint(-400, 401))
        cut = int(rng.randint(0, S + 1))
        idx = np.arange(S) + np.where(np.arange(S) < cut, sh0, sh1)
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        radius = int(rng.choice([1, 37, 300, 3000, 131072]))
        beta = [None, 0.0, 0.25, 0.6][(seed // 2) % 4]
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, k=k, w=w, p=p, radius=radius, beta=beta))
    return out


SMALL = _small_problems()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _records_equal(got, want):
    """Field by field, bit for bit (NaNs included)."""
    return got.shape == want.shape and all(_same_bits(got[f], want[f]) for f in want.dtype.names)


def test_device_equals_model_bit_for_bit():
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_refine as sr

    bad, n_breaks, n_unmatched, n_clipped, multi_k = [], 0, 0, 0, set()
    for i, pr in enumerate(SMALL):
        db = _device_pairs([(pr["ref"], pr["sub"])])
        res = sa.split_align_batch(db, pr["w"], pr["k"], pr["p"])
        recs, counts = sr.refine_breaks_batch(db, res, pr["k"], pr["radius"], pr["beta"], raw=True)
        want = rm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], res[0].block_offsets, pr["k"], pr["radius"],
                         pr["beta"])
        got = recs[0, :int(counts[0])]
        n_breaks += len(want)
        n_unmatched += int((want["flags"] & rm.UNMATCHED != 0).sum())
        n_clipped += int((want["flags"] & rm.CLIPPED != 0).sum())
        if len(want):
            multi_k.add(pr["k"])
        if not (_records_equal(got, want) and not recs[0, int(counts[0]):].tobytes().strip(b"\0")):
            diff = [f for f in want.dtype.names if got.shape != want.shape or not _same_bits(got[f], want[f])]
            bad.append((i, pr["k"], pr["w"], pr["p"], pr["radius"], pr["beta"], len(got), len(want), diff))
    assert not bad, bad[:5]
    assert n_breaks >= 200 and n_unmatched >= 5 and n_clipped >= 50 and len(multi_k) >= 3, (n_breaks, n_unmatched,
                                                                                           n_clipped, multi_k)


def test_batch_and_sub_batches_equal_the_model():
    """40 pairs in one call on a plan of 3 pairs in flight (14 sub-batches), every pair against the model."""
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import split_align as sa

    probs = [pr for pr in SMALL if pr["k"] == 512] or SMALL[:1]
    probs = (probs * 40)[:40]
    subs = [np.roll(pr["sub"], 71 * i) for i, pr in enumerate(probs)]
    db = _device_pairs([(pr["ref"], s) for pr, s in zip(probs, subs)])
    res = sa.split_align_batch(db, 2500, 512, 50.0)
    n = len(probs)
    sl = db.lens[:, 1].astype(np.int64)
    max_b = int((-(-sl // 512)).max())
    offs = np.zeros((n, max_b), np.int32)
    for p, r in enumerate(res):
        offs[p, :r.block_offsets.size] = r.block_offsets
    dev = db.data.device
    rec = torch.zeros(n * max_b * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    plan = _native.SplitPlan(3, 1, 2, 1)
    try:
        base = np.uint64(db.data.data_ptr())
        plan.refine(base + db.offs[:, 0].astype(np.uint64), db.lens[:, 0].astype(np.int64), db.lo[:, 0], db.hi[:, 0],
                    base + db.offs[:, 1].astype(np.uint64), sl, db.lo[:, 1], db.hi[:, 1], 512,
                    torch.from_numpy(offs.reshape(-1)).to(dev), 900, 0.25, rec, cnt)
        recs = rec.cpu().numpy().view(_native.BREAK_REFINE_DTYPE).reshape(n, max_b)
        counts = cnt.cpu().numpy()
    finally:
        plan.close()
    total = 0
    for p, (pr, s) in enumerate(zip(probs, subs)):
        want = rm.refine(pr["rb"], np.asarray(s) != pr["s_lv"][0], pr["r_lv"], pr["s_lv"], res[p].block_offsets, 512, 900,
                         0.25)
        assert _records_equal(recs[p, :int(counts[p])], want), p
        total += len(want)
    assert total >= 40


def test_split_outputs_unchanged_by_a_refine_call():
    """A refine call on the plan that solved the split leaves its outputs alone and the next solve equal; a plan keeps
    its workspace size until it refines."""
    import torch

    from ffsubsync_amd import _native

    pr = SMALL[1]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    base = np.uint64(db.data.data_ptr())
    rp, sp = base + db.offs[:, 0].astype(np.uint64), base + db.offs[:, 1].astype(np.uint64)
    rl, sl = db.lens[:, 0].astype(np.int64), db.lens[:, 1].astype(np.int64)
    k, w = 256, 2500
    mb = int(-(-sl[0] // k))
    dev = db.data.device
    plan = _native.SplitPlan(1, mb, 2 * w, int(sl[0]))
    try:
        outs = [torch.empty(mb, dtype=torch.int32, device=dev), torch.empty(mb, dtype=torch.float64, device=dev),
                torch.empty(1, dtype=torch.float64, device=dev)]
        plan.align(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, sl, db.lo[:, 1], db.hi[:, 1], k, w, 10.0, *outs)
        first = [t.clone() for t in outs]
        ws0 = plan.workspace_bytes
        rec = torch.empty(mb * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        plan.refine(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, sl, db.lo[:, 1], db.hi[:, 1], k, outs[0], 3000, 0.25, rec, cnt)
        torch.cuda.synchronize()
        assert int(cnt[0]) >= 1
        assert all(torch.equal(a, b) for a, b in zip(first, outs))
        assert 0 < plan.workspace_bytes - ws0 < 4096
        plan.align(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, sl, db.lo[:, 1], db.hi[:, 1], k, w, 10.0, *outs)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, outs))
    finally:
        plan.close()


def test_fewer_wrong_piece_cues_than_map_cues_on_split_workloads():
    """32 two-hour workloads/splits.py problems at the defaults.  Cue truth: the subtitle vector's runs of ones against
    the true break intervals.  Bars from the CPU calibration (profiles/split_refine_calibration.json, seeds 0..31 at
    radius 27 000, margin 0.25: 18 wrong-piece cues -> 4, 425 of 514 cut cues found, 8 false unmatched; the device
    equals the model, so these are exact unless the model moves): fewer wrong cues in total and none more on any
    problem, at least 400 cut cues found, at most 16 false unmatched."""
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_refine as sr
    from workloads import splits

    probs = [splits.make_problem(seed) for seed in range(32)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    res = sa.split_align_batch(db, 60000)
    brks = sr.refine_breaks_batch(db, res)
    tot_c = tot_r = found = false = cut_cues = 0
    worse = []
    for p, r, b in zip(probs, res, brks):
        start, end = rm.sub_cues(p.sub)
        s_us, e_us = start * 10000, end * 10000
        _, _, which = sa.map_cues(s_us, e_us, 1.0, r.pieces)
        offs = np.array([pc.offset for pc in r.pieces])
        ec = rm.cue_errors(p, start, offs[which], np.zeros(start.size, bool))
        _, _, which_r, um = sr.map_cues_refined(s_us, e_us, 1.0, r.pieces, b)
        er = rm.cue_errors(p, start, offs[np.where(um, 0, which_r)], um)
        tot_c += ec["wrong"]
        tot_r += er["wrong"]
        found += er["found"]
        false += er["false"]
        cut_cues += er["cut_cues"]
        if er["wrong"] > ec["wrong"]:
            worse.append((p.seed, ec["wrong"], er["wrong"]))
        assert np.all((which_r == sr.UNMATCHED_PIECE) == um)
    assert tot_r < tot_c and not worse, (tot_c, tot_r, worse)
    assert found >= 400 and false <= 16, (found, cut_cues, false)


def _split_tracks(seeds, duration_s, clean):
    """(problem, reference values, the subtitle track as interval records) of workloads/splits.py problems: the track is
    the pair's ratio-1.0 candidate's cues, which the seven-ratio solve maps onto the problem's subtitle vector."""
    from workloads import splits, synth

    out = []
    for seed in seeds:
        pr = splits.make_problem(seed, duration_s=duration_s, clean=clean)
        spec = synth.make_pair_spec(seed, duration_s, max_true_offset_s=min(55.0, (60000 - 1000) / 100 - 1.0))
        j = spec.ratios.index(1.0)
        start, end = spec.cand_starts[j].astype(np.int64) * 10000, spec.cand_ends[j].astype(np.int64) * 10000
        keep = end > start
        out.append((pr, pr.ref.astype(float), (start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8))))
    return out


def _same_result(a, b):
    """Name of the first field of checked_split_sync's result b that a does not equal (NaN-aware: the piece reports hold
    NaN for missing neighbours), or None."""
    import dataclasses

    for f in dataclasses.fields(b):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(y, np.ndarray):
            if not np.array_equal(x, y):
                return f.name
        elif repr(x) != repr(y):
            return f.name
    return None


def test_refined_sync_equals_checked_sync_on_clean_problems():
    from ffsubsync_amd import split_refine as sr
    from ffsubsync_amd import split_report as rep

    tracks = _split_tracks(range(8), 7200.0, True) + _split_tracks(range(8, 16), 600.0, True)
    problems = [(ref, tr) for _, ref, tr in tracks]
    got = sr.refined_split_sync(problems)
    want = rep.checked_split_sync(problems)
    bad = [(i, _same_result(g, w)) for i, (g, w) in enumerate(zip(got, want)) if _same_result(g, w)]
    assert not bad, bad
    assert all(not g.breaks and not g.cue_unmatched.any() and len(g.cue_unmatched) == len(g.cue_start_us) for g in got)


def test_refined_sync_on_split_problems():
    """The decisions of checked_split_sync; "split" results carry one refined break per piece boundary, and the cues
    flagged unmatched are exactly those with piece -2."""
    from ffsubsync_amd import split_refine as sr
    from ffsubsync_amd import split_report as rep

    tracks = _split_tracks(range(4), 7200.0, False)
    problems = [(ref, tr) for _, ref, tr in tracks]
    got = sr.refined_split_sync(problems)
    want = rep.checked_split_sync(problems)
    for g, w in zip(got, want):
        assert g.decision == w.decision == "split"
        assert [(p.first_block, p.offset) for p in g.pieces] == [(p.first_block, p.offset) for p in w.pieces]
        assert len(g.breaks) == len(g.pieces) - 1 >= 1
        assert np.array_equal(g.cue_unmatched, g.cue_piece == sr.UNMATCHED_PIECE)
        assert [b.cut for b in g.breaks] == [p.start_sample for p in g.pieces[1:]]


def test_refused_calls_leave_outputs_untouched():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_refine as sr

    pr = SMALL[0]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    res = sa.split_align_batch(db, 300, 512, 0.0)
    with pytest.raises(ValueError):
        sr.refine_breaks_batch(db, res, 512, 0, 0.25)
    with pytest.raises(ValueError):
        sr.refine_breaks_batch(db, res, 1024, 300, 0.25)  # block offsets of another K
    with pytest.raises(ValueError):
        sr.refine_breaks_batch(db, res + res, 512, 300, 0.25)
    plan = _native.SplitPlan(1, 1, 2, 1)
    try:
        base = np.uint64(db.data.data_ptr())
        rp, sp = base + db.offs[:, 0].astype(np.uint64), base + db.offs[:, 1].astype(np.uint64)
        rl, sl = db.lens[:, 0].astype(np.int64), db.lens[:, 1].astype(np.int64)
        dev = db.data.device
        mb = int(-(-sl[0] // 512))
        offs = torch.from_numpy(res[0].block_offsets.astype(np.int32)).to(dev)
        rec = torch.full((mb * _native.BREAK_REFINE_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
        cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
        before = [t.clone() for t in (offs, rec, cnt)]
        ws0 = plan.workspace_bytes
        cases = [dict(k=300), dict(k=128), dict(radius=0), dict(radius=_native.REFINE_MAX_RADIUS + 1), dict(beta=-1.0),
                 dict(beta=math.inf), dict(sl=np.zeros(1, np.int64)), dict(rl=np.zeros(1, np.int64))]
        for case in cases:
            args = dict(k=512, radius=300, beta=0.25, sl=sl, rl=rl)
            args.update(case)
            with pytest.raises(_native.NativeError) as ei:
                plan.refine(rp, args["rl"], db.lo[:, 0], db.hi[:, 0], sp, args["sl"], db.lo[:, 1], db.hi[:, 1], args["k"],
                            offs, args["radius"], args["beta"], rec, cnt)
            assert ei.value.code == (-5 if "sl" in case or "rl" in case else -1), case  # FFS_E_EMPTY / FFS_E_INVALID
        torch.cuda.synchronize()
        for a, b in zip(before, (offs, rec, cnt)):
            assert torch.equal(a, b)
        assert plan.workspace_bytes == ws0  # the refine scratch is made by the first call that runs
        plan.refine(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, sl, db.lo[:, 1], db.hi[:, 1], 512, offs, 300, math.nan, rec, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes > ws0 and int(cnt[0]) == len(rm.breaks_of(res[0].block_offsets))
    finally:
        plan.close()
    sr.clear_plan_cache()
