"""Per-piece quality report of a split solve on the device (csrc/ffs_split_report.h via ffsubsync_amd.split_report): bit
for bit against the numpy model tests/split_report_model.py, the split outputs bit-identical to split_align_batch, the
infinite penalty against quality_batch, break evidence on the seeded split workloads, checked_split_sync's decisions,
and the error paths."""
import json
import os

import numpy as np
import pytest

import split_report_model as srm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _device_pairs(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _small_problems(n=64):
    """Seeded small problems: R < S and R > S, S not a multiple of K, windows past both ends, non-default levels, penalties
    from 0 to inf, a second true offset in about half of them, top_k 1..8 and exclusion distances from 1 up."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(7000 + seed)
        R, S = int(rng.randint(800, 16000)), int(rng.randint(800, 16000))
        k = int(rng.choice([256, 512, 1024, 2048]))
        w = int(rng.choice([1, 37, 300, 2500, 6000, 20000]))
        p = float(rng.choice([0.0, 0.5, 100.0, 2000.0, 8192.0, np.inf]))
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25)][seed % 4]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        sh0 = int(rng.randint(-min(w, 3000), min(w, 3000) + 1))
        sh1 = sh0 + int(rng.randint(-400, 401)) if rng.rand() < 0.5 else sh0
        cut = int(rng.randint(0, S + 1))
        idx = np.arange(S) + np.where(np.arange(S) < cut, sh0, sh1)
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        top_k = int(rng.randint(1, 9))
        e = int(rng.choice([1, 50, 300, 5000]))
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, k=k, w=w, p=p, top_k=top_k, e=e))
    return out


SMALL = _small_problems()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _records_equal(got, want):
    """Field by field, bit for bit (NaNs included)."""
    return got.shape == want.shape and all(_same_bits(got[f], want[f]) for f in want.dtype.names)


def _report_one(pr):
    from ffsubsync_amd import split_report as sr

    db = _device_pairs([(pr["ref"], pr["sub"])])
    res, recs, counts = sr.split_report_batch(db, pr["w"], pr["k"], pr["p"], pr["top_k"], pr["e"], raw=True)
    return db, res[0], recs[0, :int(counts[0])]


def test_device_equals_model_bit_for_bit():
    from ffsubsync_amd import split_align as sa

    bad, multi = [], 0
    for i, pr in enumerate(SMALL):
        db, res, recs = _report_one(pr)
        (offs, scores, total, pieces), want, _ = srm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"],
                                                             pr["p"], pr["top_k"], pr["e"])
        plain = sa.split_align_batch(db, pr["w"], pr["k"], pr["p"])[0]
        same_split = (np.array_equal(res.block_offsets.astype(np.int64), offs) and _same_bits(res.block_scores, scores)
                      and _same_bits(np.float64(res.total), np.float64(total)))
        same_plain = (_same_bits(plain.block_offsets, res.block_offsets) and _same_bits(plain.block_scores, res.block_scores)
                      and _same_bits(np.float64(plain.total), np.float64(res.total)))
        multi += len(pieces) > 1
        if not (same_split and same_plain and _records_equal(recs, want)):
            diff = [f for f in want.dtype.names if recs.shape != want.shape or not _same_bits(recs[f], want[f])]
            bad.append((i, pr["k"], pr["w"], pr["p"], same_split, same_plain, len(recs), len(want), diff))
    assert not bad, bad[:5]
    assert multi >= 8


def test_every_block_its_own_piece_at_zero_penalty():
    """P = 0 on noise: (almost) every block is a piece of its own, and the workspace holds them all."""
    from ffsubsync_amd import split_report as sr

    rng = np.random.RandomState(5)
    rb, sb = rng.rand(40000) < 0.5, rng.rand(33000) < 0.5
    rb[0], rb[1], sb[0], sb[1] = True, False, True, False
    db = _device_pairs([(rb.astype(float), sb.astype(float))])
    res, recs, counts = sr.split_report_batch(db, 3000, 256, 0.0, 4, 100, raw=True)
    n_blocks = -(-sb.size // 256)
    assert int(counts[0]) == len(res[0].pieces) >= 0.9 * n_blocks
    _, want, _ = srm.report(rb, sb, (0.0, 1.0), (0.0, 1.0), 256, 3000, 0.0, 4, 100)
    assert _records_equal(recs[0, :int(counts[0])], want)
    assert not recs[0, int(counts[0]):].tobytes().strip(b"\0")  # records past the count are zero


def test_batch_call_equals_pairs_one_at_a_time():
    from ffsubsync_amd import split_report as sr

    probs = [pr for pr in SMALL if pr["w"] == 2500] or SMALL[:1]
    probs = (probs * 40)[:40]
    subs = [np.roll(pr["sub"], 53 * i) for i, pr in enumerate(probs)]
    db = _device_pairs([(pr["ref"], s) for pr, s in zip(probs, subs)])
    res, recs, counts = sr.split_report_batch(db, 2500, 512, 300.0, 3, 200, pairs_in_flight=16, raw=True)  # 3 sub-batches
    for i, (pr, s) in enumerate(zip(probs, subs)):
        r1, c1, n1 = sr.split_report_batch(_device_pairs([(pr["ref"], s)]), 2500, 512, 300.0, 3, 200, raw=True)
        assert int(counts[i]) == int(n1[0])
        assert _records_equal(recs[i, :int(counts[i])], c1[0, :int(n1[0])])
        assert _same_bits(res[i].block_scores, r1[0].block_scores)


def test_infinite_penalty_is_the_whole_file_report():
    """Headline seeds 0..63: one piece, peak 1 at the solve's record offset, moments and psr as quality_batch's over the
    same window (the scores' arithmetic differs in the last bits: the records' fused chain against the split's)."""
    from ffsubsync_amd import batch, quality
    from ffsubsync_amd import split_report as sr
    from workloads import synth

    gold = json.load(open(os.path.join(HERE, "golden", "headline_golden.json")))["pairs"][:64]
    specs = [synth.make_pair_spec(g["seed"]) for g in gold]
    db = synth.build_device_batch(specs)
    al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=64)
    try:
        _, pres = al.solve(db)
    finally:
        al.close()
    one = db.select_candidates(pres["best_cand"].astype(np.int64))
    reps = sr.split_report_batch(one, 6000, 1024, float("inf"))
    qs = quality.quality_batch(one, 6000)
    rel = lambda a, b: abs(a - b) <= 1e-9 * abs(b)
    bad = [(g["seed"], len(r.pieces), r.pieces[0].peaks[:1], int(p["offset"]), r.pieces[0].mean, q.mean)
           for g, r, q, p in zip(gold, reps, qs, pres)
           if len(r.pieces) != 1 or r.pieces[0].peaks[0][1] != int(p["offset"]) or r.pieces[0].n_lags != q.n_lags
           or not (rel(r.pieces[0].mean, q.mean) and rel(r.pieces[0].std, q.std) and rel(r.pieces[0].psr, q.psr))
           or not r.pieces[0].own_is_peak]
    assert not bad, bad[:5]


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


def test_true_breaks_are_supported_and_checked_sync_splits():
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_report as sr
    from workloads import splits

    probs = [splits.make_problem(seed) for seed in range(32)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    reps = sr.split_report_batch(db, 60000)
    unsupported = [(p.seed, sr.break_support(r.pieces), [(q.gain_prev, q.gain_next, q.psr) for q in r.pieces])
                   for p, r in zip(probs, reps) if not all(sr.break_support(r.pieces)) or sr.assess_split(r.pieces)]
    assert not unsupported, unsupported[:3]
    assert sum(len(r.pieces) - 1 for r in reps) == sum(len(p.breaks) for p in probs)
    tracks = _split_tracks(range(32), 7200.0, False)
    got = sr.checked_split_sync([(ref, tr) for _, ref, tr in tracks])
    want = sa.split_sync([(ref, tr) for _, ref, tr in tracks])
    bad = [(i, g.decision, g.reasons) for i, (g, w) in enumerate(zip(got, want))
           if g.decision != "split" or [(p.first_block, p.end_block, p.offset) for p in g.pieces]
           != [(p.first_block, p.end_block, p.offset) for p in w.pieces]
           or not np.array_equal(g.cue_start_us, w.cue_start_us) or not np.array_equal(g.cue_end_us, w.cue_end_us)]
    assert not bad, bad[:5]


def test_spurious_pieces_are_flagged_at_low_penalty():
    """Clean 2 h problems solved at P = 1000: every break the DP makes is unsupported, and the result lands at the true
    offset -- "single", or "split" with one piece where the DP made none."""
    from ffsubsync_amd import split_report as sr

    tracks = _split_tracks(range(32), 7200.0, True)
    db = _device_pairs([(ref, pr.sub.astype(float) * pr.sub_hi) for pr, ref, _ in tracks])
    reps = sr.split_report_batch(db, 60000, split_penalty=1000.0)
    assert sum(len(r.pieces) > 1 for r in reps) >= 8  # the low penalty does provoke spurious pieces
    supported = [(pr.seed, i) for (pr, _, _), r in zip(tracks, reps) for i, ok in enumerate(sr.break_support(r.pieces)) if ok]
    assert not supported, supported[:5]
    got = sr.checked_split_sync([(ref, tr) for _, ref, tr in tracks], split_penalty=1000.0)
    bad = []
    for (pr, _, _), r, g in zip(tracks, reps, got):
        want = pr.offsets[0]
        if g.decision == "single":
            ok = abs(g.global_offset - want) <= 2 and np.all(g.cue_piece == 0)
        else:
            ok = g.decision == "split" and len(r.pieces) == 1 and len(g.pieces) == 1 and abs(g.pieces[0].offset - want) <= 2
        if not ok:
            bad.append((pr.seed, g.decision, g.reasons, [p.offset for p in g.pieces], g.global_offset, want))
    assert not bad, bad[:5]


@pytest.mark.parametrize("duration_s", [600.0, 7200.0])
def test_wrong_pairs_are_untrusted(duration_s):
    """The subtitle of seed i against the reference of seed i+1: no split and no single offset is trusted, and the cues
    come back unmodified."""
    from ffsubsync_amd import split_report as sr

    tracks = _split_tracks(range(17), duration_s, True)
    got = sr.checked_split_sync([(tracks[i + 1][1], tracks[i][2]) for i in range(16)])
    bad = [(i, g.decision, [q.psr for q in g.piece_quality], g.supported, g.quality.psr) for i, g in enumerate(got)
           if g.decision != "untrusted" or not np.array_equal(g.cue_start_us, tracks[i][2][0])
           or not np.array_equal(g.cue_end_us, tracks[i][2][1]) or not np.all(g.cue_piece == -1)]
    assert not bad, bad[:5]


def test_error_paths_raise_before_any_kernel():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_report as sr

    pr = SMALL[0]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    with pytest.raises(ValueError):
        sr.split_report_batch(db, 100, 512, 10.0, top_k=0)
    with pytest.raises(ValueError):
        sr.split_report_batch(db, 100, 512, 10.0, exclusion_samples=0)
    with pytest.raises(ValueError):
        sr.split_report_batch(db, 100, 500, 10.0)
    # the C ABI itself: every bad argument is refused before a launch, and the output buffers keep their contents
    plan = _native.SplitPlan(1, 64, 2 * 100, 20000)
    try:
        base = np.uint64(db.data.data_ptr())
        rp, sp = base + db.offs[:, 0].astype(np.uint64), base + db.offs[:, 1].astype(np.uint64)
        rl, sl = db.lens[:, 0].astype(np.int64), db.lens[:, 1].astype(np.int64)
        dev = db.data.device
        mb = int(-(-sl[0] // 512))
        offs = torch.full((mb,), 7, dtype=torch.int32, device=dev)
        scores = torch.full((mb,), 3.5, dtype=torch.float64, device=dev)
        totals = torch.full((1,), 3.5, dtype=torch.float64, device=dev)
        rep = torch.full((mb * _native.PIECE_REPORT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
        cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
        before = [t.clone() for t in (offs, scores, totals, rep, cnt)]
        ws0 = plan.workspace_bytes
        cases = [dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0), dict(w=101), dict(k=300), dict(p=-1.0),
                 dict(sl=np.zeros(1, np.int64))]
        for case in cases:
            args = dict(top_k=3, exclusion_samples=300, w=100, k=512, p=10.0, sl=sl)
            args.update(case)
            with pytest.raises(_native.NativeError) as ei:
                plan.align_report(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, args["sl"], db.lo[:, 1], db.hi[:, 1], args["k"],
                                  args["w"], args["p"], args["top_k"], args["exclusion_samples"], offs, scores, totals,
                                  rep, cnt)
            assert ei.value.code == (-5 if "sl" in case else -1)  # FFS_E_EMPTY / FFS_E_INVALID
        torch.cuda.synchronize()
        for a, b in zip(before, (offs, scores, totals, rep, cnt)):
            assert torch.equal(a, b)
        assert plan.workspace_bytes == ws0  # the report workspace is made by the first call that runs, not by refusals
        plan.align_report(rp, rl, db.lo[:, 0], db.hi[:, 0], sp, sl, db.lo[:, 1], db.hi[:, 1], 512, 100, 10.0, 3, 300,
                          offs, scores, totals, rep, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes > ws0 and int(cnt[0]) >= 1
    finally:
        plan.close()
    sa.clear_plan_cache()
