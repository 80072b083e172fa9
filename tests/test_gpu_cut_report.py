"""Per-piece quality report over a lag range on the device (csrc/ffs_cut_report.h via ffsubsync_amd.cut_report): bit for
bit against split_report_batch at [-W+1, W], bit for bit against the numpy model tests/cut_report_model.py on small
problems, every block its own piece at 2 h over the full range (rounds), checked_cut_sync on cut, wrong and clean
problems, and the refused calls."""
import json
import os

import numpy as np
import pytest

import cut_model as cm
import cut_report_model as crm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_pairs(problems, packed=True):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs, packed=packed)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _small_problems(n=40):
    """Seeded problems: R < S and R > S, tails of 1..K-1 samples, K 256..2048, non-default levels, penalties 0..inf, lag
    ranges of five kinds (full, asymmetric, lag_lo > 0, past both overlap edges, [-W+1, W]), top_k 1..8, several E."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(7700 + seed)
        R, S = int(rng.randint(700, 7000)), int(rng.randint(700, 7000))
        k = int(rng.choice([256, 512, 1024, 2048]))
        p = [0.0, 0.5, 60.0, 900.0, np.inf][seed % 5]
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25)][(seed // 3) % 4]
        seg = np.maximum(1, rng.geometric(1.0 / 50.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        sh0 = int(rng.randint(-S // 2, R // 2))
        sh1 = sh0 + int(rng.randint(-1500, 1501))
        cut = int(rng.randint(0, S + 1))
        idx = np.arange(S) + np.where(np.arange(S) < cut, sh0, sh1)
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        kind = seed % 5
        if kind == 0:
            lo, hi = cm.full_range(R, S)
        elif kind == 1:
            lo, hi = -int(rng.randint(1, S)), int(rng.randint(0, 3 * R))
        elif kind == 2:
            lo = int(rng.randint(1, R))
            hi = lo + int(rng.randint(0, 4000))
        elif kind == 3:
            lo, hi = -S - int(rng.randint(0, 3000)), R + int(rng.randint(0, 3000))
        else:
            w = int(rng.randint(1, 5000))
            lo, hi = -w + 1, w
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, k=k, p=p, lo=lo, hi=hi, top_k=int(rng.randint(1, 9)),
                        e=int(rng.choice([1, 50, 300, 5000])), packed=bool(seed % 4)))
    return out


def test_symmetric_range_equals_split_report_batch():
    """The 64 workloads/splits.py seeds at W = 60 000, fed split_report_batch's block offsets: every record identical."""
    from ffsubsync_amd import cut_report as cr
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_report as sr
    from workloads import splits

    probs = [splits.make_problem(seed) for seed in range(64)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    w = 60000
    res, want, want_n = sr.split_report_batch(db, w, raw=True)
    got, got_n = cr.report_batch(db, [r.block_offsets for r in res], (-w + 1, w))
    assert np.array_equal(got_n, want_n)
    assert got.tobytes() == want.tobytes()
    assert sum(int(n) > 1 for n in got_n) >= 32
    sa.clear_plan_cache()
    cr.clear_plan_cache()


def test_device_equals_model_bit_for_bit():
    from ffsubsync_amd import cut_report as cr

    bad, multi = [], 0
    for i, pr in enumerate(_small_problems()):
        db = _device_pairs([(pr["ref"], pr["sub"])], packed=pr["packed"])
        res, recs, counts = cr.split_range_report_batch(db, (pr["lo"], pr["hi"]), pr["k"], pr["p"], pr["top_k"], pr["e"],
                                                        raw=True)
        offs, scores, total = cm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"], pr["p"])
        want, _ = crm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"], offs, pr["top_k"],
                             pr["e"])
        n = int(counts[0])
        multi += n > 1
        same_split = np.array_equal(res[0].block_offsets, offs) and _same_bits(res[0].block_scores, scores)
        if not (same_split and n == want.size and recs[0, :n].tobytes() == want.tobytes()
                and not recs[0, n:].tobytes().strip(b"\0")):
            diff = [f for f in want.dtype.names if n != want.size or not _same_bits(recs[0, :n][f], want[f])]
            bad.append((i, pr["k"], pr["lo"], pr["hi"], pr["p"], same_split, n, want.size, diff))
    assert not bad, bad[:5]
    assert multi >= 8
    cr.clear_plan_cache()


def test_every_block_its_own_piece_at_2h_full_range():
    """P = 0 on a 2 h cut problem over the full range: about 700 pieces, reported 8 per pair and round, within the
    stated workspace; a sample of the pieces equals the model."""
    from ffsubsync_amd import cut_report as cr
    from workloads import cuts

    pr = cuts.make_problem(0)
    sub = pr.sub.astype(float) * pr.sub_hi
    db = _device_pairs([(pr.ref.astype(float), sub)])
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size)
    res, recs, counts = cr.split_range_report_batch(db, None, 1024, 0.0, raw=True)
    n = int(counts[0])
    n_blocks = -(-pr.sub.size // 1024)
    assert n == len(res[0].pieces) >= 0.5 * n_blocks
    plan = cr._plans.plans[(__import__("torch").cuda.current_device(), "report")]
    L = hi - lo + 1
    split_bytes = n_blocks * (L + 63) // 64 * 8 + 2 * L * 8 + 4 * (pr.ref.size // 32 + 2) * 4 + (1 << 20)
    assert plan.workspace_bytes <= split_bytes + cr.ROUND_PIECES * (L + 64) * 4 + (1 << 20)
    which = sorted({0, 1, 7, 8, 9, n // 2, n - 2, n - 1})
    want, _ = crm.report(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), 1024, lo, hi, res[0].block_offsets, 3, 300,
                         which=which)
    for i in which:
        assert recs[0, i].tobytes() == want[i].tobytes(), i
    assert not recs[0, n:].tobytes().strip(b"\0")
    cr.clear_plan_cache()


def _calibration():
    return json.load(open(os.path.join(ROOT, "profiles", "cut_report_calibration.json")))


def _clean_tracks(seeds):
    from workloads import splits, synth

    out = []
    for seed in seeds:
        pr = splits.make_problem(seed, duration_s=7200.0, clean=True)
        spec = synth.make_pair_spec(seed, 7200.0, max_true_offset_s=min(55.0, (60000 - 1000) / 100 - 1.0))
        j = spec.ratios.index(1.0)
        start, end = spec.cand_starts[j].astype(np.int64) * 10000, spec.cand_ends[j].astype(np.int64) * 10000
        keep = end > start
        out.append((pr, (pr.ref.astype(float), (start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)))))
    return out


def test_checked_cut_sync_on_cut_wrong_and_clean_problems():
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import cut_report as cr
    from workloads import cuts

    cal = _calibration()
    probs = [cuts.make_problem(seed) for seed in range(9)]
    problems = [(p.ref.astype(float), p.track) for p in probs[:8]]
    got = cr.checked_cut_sync(problems)
    want = ca.cut_sync(problems)
    share = sum(g.decision == "cut" for g in got) / 8.0
    assert share >= cal["summary"]["cut"]["cut_share_seeds_0_7"] - 0.1, [(g.decision, g.reasons) for g in got]
    for g, w in zip(got, want):
        assert [(p.first_block, p.offset) for p in g.pieces] == [(p.first_block, p.offset) for p in w.pieces]
        assert len(g.piece_quality) == len(g.pieces) and len(g.verified) == len(g.pieces)
        if g.decision != "untrusted":
            assert np.array_equal(g.cue_start_us, w.cue_start_us) and np.array_equal(g.cue_end_us, w.cue_end_us)
            assert np.array_equal(g.cue_piece, w.cue_piece)
    # the subtitle of seed i against the reference of seed i+1
    wrong = cr.checked_cut_sync([(probs[i + 1].ref.astype(float), probs[i].track) for i in range(8)])
    for i, g in enumerate(wrong):
        assert g.decision == "untrusted", (i, g.reasons)
        assert np.array_equal(g.cue_start_us, probs[i].track[0]) and np.array_equal(g.cue_end_us, probs[i].track[1])
        assert np.all(g.cue_piece == -1) and not g.cue_verified.any()
    # clean problems (one true offset): no verified piece is more than 2 samples off
    clean = _clean_tracks(range(8))
    res = cr.checked_cut_sync([t for _, t in clean])
    for (pr, _), g in zip(clean, res):
        off = [q.offset for q, v in zip(g.piece_quality, g.verified) if v]
        assert all(abs(o - pr.offsets[0]) <= 2 for o in off), (pr.seed, off, pr.offsets[0])
        if cal["summary"]["clean"]["one_piece_every_seed"]:
            assert g.decision == "single", (pr.seed, g.reasons)
    ca.clear_plan_cache()
    cr.clear_plan_cache()


def test_refused_calls_leave_outputs_untouched():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import cut_report as cr

    pr = _small_problems(1)[0]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    with pytest.raises(ValueError):
        cr.split_range_report_batch(db, None, 1024, 10.0, top_k=0)
    with pytest.raises(ValueError):
        cr.split_range_report_batch(db, None, 1024, 10.0, exclusion_samples=0)
    with pytest.raises(ValueError):
        cr.split_range_report_batch(db, (5, 4))
    with pytest.raises(ValueError):
        cr.checked_cut_sync([(pr["ref"], (np.array([0]), np.array([10 ** 6]), np.zeros(1, np.uint8)))], min_coverage=2.0)
    plan = _native.SplitRangePlan(1, 64, 20000, 10000)
    try:
        rp, rl, rlo, rhi, sp, sl, slo, shi = db.pair_arrays()
        dev = db.data.device
        mb = int(-(-sl[0] // 512))
        one = lambda v: np.array([v], np.int64)
        offs = torch.full((mb,), 7, dtype=torch.int32, device=dev)
        rep = torch.full((mb * _native.PIECE_REPORT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
        cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
        before = [t.clone() for t in (offs, rep, cnt)]
        ws0 = plan.workspace_bytes
        cases = [dict(top_k=0), dict(top_k=9), dict(e=0), dict(k=300), dict(lo=one(5), hi=one(4)), dict(lo=one(8)),
                 dict(hi=one(6)), dict(lo=one(0), hi=one(20000)), dict(sl=np.zeros(1, np.int64))]
        for case in cases:
            args = dict(top_k=3, e=300, k=512, lo=one(-100), hi=one(100), sl=sl)
            args.update(case)
            with pytest.raises(_native.NativeError) as ei:
                plan.report(rp, rl, rlo, rhi, sp, args["sl"], slo, shi, args["k"], args["lo"], args["hi"], offs,
                            args["top_k"], args["e"], rep, cnt)
            assert ei.value.code == (-5 if "sl" in case else -1), case  # FFS_E_EMPTY / FFS_E_INVALID
        torch.cuda.synchronize()
        for a, b in zip(before, (offs, rep, cnt)):
            assert torch.equal(a, b)
        assert plan.workspace_bytes == ws0  # the report workspace is made by the first call that runs
        plan.report(rp, rl, rlo, rhi, sp, sl, slo, shi, 512, one(-100), one(100), offs, 3, 300, rep, cnt)
        torch.cuda.synchronize()
        ws1 = plan.workspace_bytes
        assert ws1 > ws0 and int(cnt[0]) == 1
        plan.report(rp, rl, rlo, rhi, sp, sl, slo, shi, 512, one(-100), one(100), offs, 3, 300, rep, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes == ws1
    finally:
        plan.close()
