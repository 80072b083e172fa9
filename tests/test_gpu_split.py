"""Split-aware alignment on the device (csrc/ffs_split.h via ffsubsync_amd.split_align): bit for bit against the numpy
model, the infinite penalty against the unmodified reference's FFTAligner(6000) records, break recovery on the seeded
split workloads at the defaults, batching, and split_sync end to end."""
import json
import os

import numpy as np
import pytest

import split_model as sm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _device_pairs(problems):
    """DeviceBatch (one candidate per pair) from host (ref values, sub values) pairs of two-level float vectors."""
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _small_problems(n=64):
    """Seeded small problems: R < S and R > S, S not a multiple of K, windows past both ends, non-default levels,
    amplitudes of ratios > 1, penalties from 0 to inf."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(1000 + seed)
        R, S = int(rng.randint(800, 20000)), int(rng.randint(800, 20000))
        k = int(rng.choice([256, 512, 1024, 2048]))
        w = int(rng.choice([1, 37, 300, 2500, 6000, 30000]))
        p = float(rng.choice([0.0, 0.5, 100.0, 2000.0, 8192.0, np.inf]))
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25)][seed % 4]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        shift = int(rng.randint(-min(w, 3000), min(w, 3000) + 1))
        idx = np.arange(S) + shift
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        r_val = np.where(rb, r_lv[1], r_lv[0])
        s_val = np.where(sb, s_lv[1], s_lv[0])
        out.append(dict(ref=r_val, sub=s_val, rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, k=k, w=w, p=p))
    return out


SMALL = _small_problems()


def _solve_one(pr):
    from ffsubsync_amd import split_align as sa

    db = _device_pairs([(pr["ref"], pr["sub"])])
    return sa.split_align_batch(db, pr["w"], pr["k"], pr["p"])[0]


def test_device_equals_model_bit_for_bit():
    bad = []
    for i, pr in enumerate(SMALL):
        res = _solve_one(pr)
        offs, scores, total, pieces = sm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], pr["p"])
        same = (np.array_equal(res.block_offsets.astype(np.int64), offs)
                and np.array_equal(res.block_scores.view(np.int64), scores.view(np.int64))
                and np.float64(res.total).view(np.int64) == np.float64(total).view(np.int64)
                and [(p.first_block, p.end_block, p.start_sample, p.end_sample, p.offset, p.score) for p in res.pieces] == pieces)
        if not same:
            bad.append((i, pr["k"], pr["w"], pr["p"], res.total, total, len(res.pieces), len(pieces)))
    assert not bad, bad[:5]


def test_batch_call_equals_pairs_one_at_a_time():
    from ffsubsync_amd import split_align as sa

    probs = [pr for pr in SMALL if pr["w"] == 2500] or SMALL[:1]
    probs = (probs * 64)[:64]
    for i, pr in enumerate(probs):  # one shared (K, W, P) per call; vary the pairs
        probs[i] = dict(pr, sub=np.roll(pr["sub"], 37 * i))
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    many = sa.split_align_batch(db, 2500, 512, 300.0, pairs_in_flight=24)  # three sub-batches
    for pr, got in zip(probs, many):
        one = sa.split_align_batch(_device_pairs([(pr["ref"], pr["sub"])]), 2500, 512, 300.0)[0]
        assert np.array_equal(got.block_offsets, one.block_offsets)
        assert np.array_equal(got.block_scores.view(np.int64), one.block_scores.view(np.int64))
        assert got.total == one.total


def test_infinite_penalty_equals_reference_fft_aligner():
    """headline seeds 0..63, every one of the seven candidates: the unmodified reference's FFTAligner(6000) records."""
    from ffsubsync_amd import split_align as sa
    from workloads import synth

    gold = json.load(open(os.path.join(HERE, "golden", "headline_golden.json")))["pairs"][:64]
    specs = [synth.make_pair_spec(g["seed"]) for g in gold]
    db = synth.build_device_batch(specs)
    bad, ties = [], 0
    for j in range(7):
        res = sa.split_align_batch(db.select_candidates([j] * len(specs)), 6000, 1024, float("inf"))
        for g, r in zip(gold, res):
            score, off = float(g["per_candidate"][j][0]), int(g["per_candidate"][j][1])
            tie = g["per_candidate_top2_gap"][j] <= 0.5
            ties += tie
            if len(r.pieces) != 1 or (r.pieces[0].offset != off and not tie) or \
                    abs(r.pieces[0].score - score) > 1e-5 * abs(score) or abs(r.total - score) > 1e-5 * abs(score):
                bad.append((g["seed"], j, [(p.offset, p.score) for p in r.pieces], (off, score)))
    assert not bad, bad[:5]
    assert ties < 0.2 * 7 * len(gold)


def test_breaks_recovered_at_the_defaults():
    """2 h problems of workloads/splits.py, +-10 min, K = 1024, P = 8192: the right number of pieces and every piece's
    offset within 2 samples on all 32; every break within one block on all but one, and within four blocks on all.
    The one exception (seed 29, a 145 s insertion) is the data, not the solver: the subtitle track lost two lines in the
    20 s before the break (synth drops 15 % of them), the blocks there score higher at the new offset, and the DP's
    objective -- which the device meets bit for bit, test_device_equals_model_bit_for_bit -- puts the break 4 blocks early."""
    from ffsubsync_amd import split_align as sa
    from workloads import splits

    probs = [splits.make_problem(seed) for seed in range(32)]
    db = _device_pairs([(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in probs])
    res = sa.split_align_batch(db, 60000)
    strict = [(p.seed, p.kinds, p.breaks, p.offsets, splits.check_recovery(p, r.block_offsets, 1024))
              for p, r in zip(probs, res) if splits.check_recovery(p, r.block_offsets, 1024)]
    loose = [(p.seed, splits.check_recovery(p, r.block_offsets, 1024, block_tol=4))
             for p, r in zip(probs, res) if splits.check_recovery(p, r.block_offsets, 1024, block_tol=4)]
    assert not loose, loose[:5]
    assert [x[0] for x in strict] in ([], [29]), strict[:5]


def _spec_track(spec):
    """The subtitle track of a synth pair as interval records (its ratio-1.0 candidate's samples, 10 ms each)."""
    j = spec.ratios.index(1.0)
    start = spec.cand_starts[j].astype(np.int64) * 10000
    end = spec.cand_ends[j].astype(np.int64) * 10000
    keep = end > start
    return start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)


def test_split_sync_without_breaks_is_one_piece_at_the_seven_ratio_solve():
    from ffsubsync_amd import batch
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd.constants import candidate_ratios
    from ffsubsync_amd.subtitle_raster import DeviceRaster, rasterize_candidates
    from workloads import synth

    specs = [synth.make_pair_spec(seed) for seed in range(64)]
    refs = [synth.rasterize(sp.ref_len, sp.ref_starts, sp.ref_ends).astype(float) for sp in specs]
    tracks = [_spec_track(sp) for sp in specs]
    got = sa.split_sync(list(zip(refs, tracks)))
    ratios = candidate_ratios()
    pairs = [(DeviceRaster.from_host(r, lists=False), rasterize_candidates(t[0], t[1], t[2], ratios)) for r, t in zip(refs, tracks)]
    db = batch.pack_pairs(pairs)
    al = batch.BatchAligner(db.required_fft_length(60000), 7, 60000, pairs_in_flight=64)
    _, pres = al.solve(db)
    al.close()
    bad = [(i, [(p.offset, p.first_block, p.end_block) for p in g.pieces], g.ratio_index, int(pres[i]["best_cand"]),
            int(pres[i]["offset"]))
           for i, g in enumerate(got)
           if len(g.pieces) != 1 or g.pieces[0].offset != int(pres[i]["offset"]) or g.ratio_index != int(pres[i]["best_cand"])
           or g.global_offset != int(pres[i]["offset"])]
    assert not bad, bad[:5]


def test_split_sync_cue_times_equal_the_model_mapping():
    """Interval records in, cue times out: a 25 min subtitle track against a reference with an inserted 75 s break."""
    from ffsubsync_amd import split_align as sa
    from oracle import raster_oracle as ro
    from workloads import synth

    start, end, meta = synth.make_subtitle_records(5, duration_s=1500.0)
    base = ro.rasterize(start, end, meta, 1.0)
    d0, q, n_ins = 1234, 80000, 7500
    rng = np.random.RandomState(9)
    shifted = np.concatenate([np.zeros(d0), base])  # reference sample i + d0 = subtitle sample i
    filler = (np.repeat(rng.rand(n_ins // 150 + 1) < 0.4, 150)[:n_ins]).astype(float)
    ref = np.concatenate([shifted[:q + d0], filler, shifted[q + d0:]])
    res = sa.split_sync([(ref, (start, end, meta))], max_offset_seconds=150.0)[0]
    assert res.ratio == 1.0
    sub = ro.rasterize(start, end, meta, res.ratio)
    _, _, _, pieces = sm.solve(ref != 0, sub != 0, (0.0, 1.0), (0.0, 1.0), 1024, 15000, sa.DEFAULT_SPLIT_PENALTY)
    assert [(p.first_block, p.end_block, p.offset) for p in res.pieces] == [(p[0], p[1], p[4]) for p in pieces]
    assert [p.offset for p in res.pieces] == [d0, d0 + n_ins]
    model_pieces = [sa.Piece(p[0], p[1], p[2], p[3], p[4], p[5]) for p in pieces]
    want_s, want_e, want_k = sa.map_cues(start, end, res.ratio, model_pieces)
    assert np.array_equal(res.cue_start_us, want_s) and np.array_equal(res.cue_end_us, want_e)
    assert np.array_equal(res.cue_piece, want_k)
