"""Calibration of checked_cut_sync's thresholds over the full lag range: the device report
(ffsubsync_amd.cut_report.split_range_report_batch, bit-identical to the numpy model tests/cut_report_model.py) on 2 h
problems, every pair's full overlap range, K = 1024, the default penalty, top_k 3, E = 300, in three classes:
  - cut:   workloads/cuts.py seeds 0..n-1 as generated (the true-ratio subtitle vector, what the windowless seven-ratio
           solve picks on every seed here);
  - clean: workloads/splits.py problems with clean=True (one true offset);
  - wrong: the subtitle of cut seed i against the reference of cut seed i+1.
Per piece: psr by length and by correctness (offset within 10 samples of the truth at the piece's middle sample); per
break: min(gain_next_i, gain_prev_{i+1}), true (both sides correct, different true offsets) or spurious; per problem:
coverage and the decision at the chosen thresholds.

    python profiles/cut_report_calibration.py [n_seeds=32] [out=profiles/cut_report_calibration.json]
    python profiles/cut_report_calibration.py --rescore profiles/cut_report_calibration.json   # new thresholds, no GPU
"""
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, TOL = 1024, 10


def _truth_cut(pr, q):
    from workloads import cuts

    t = pr.true_offset((q.start_sample + q.end_sample) // 2)
    return None if t is cuts.UNMATCHED else int(t)


def _run(cls, pairs, truths, cr):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    db = batch.pack_pairs([(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)])
                           for r, s in pairs])
    reps = cr.split_range_report_batch(db)
    out = []
    for i, (rep, truth) in enumerate(zip(reps, truths)):
        pieces = []
        for q in rep.pieces:
            t = truth(q)
            pieces.append({"start": q.start_sample, "end": q.end_sample, "minutes": (q.end_sample - q.start_sample) / 6000.0,
                           "offset": q.offset, "truth": t, "correct": t is not None and abs(q.offset - t) <= TOL,
                           "psr": q.psr, "flat": q.flat, "gain_prev": q.gain_prev, "gain_next": q.gain_next})
        breaks = []
        for a, b in zip(pieces[:-1], pieces[1:]):
            true = a["correct"] and b["correct"] and a["truth"] != b["truth"]
            breaks.append({"gain": min(a["gain_next"], b["gain_prev"]), "true": bool(true)})
        out.append({"class": cls, "index": i, "pieces": pieces, "breaks": breaks, "S": rep.pieces[-1].end_sample})
    return out


def _decide(rec, psr, gain, cov, cr):
    class Q:  # the fields assess_cut reads
        pass

    qs = []
    for p in rec["pieces"]:
        q = Q()
        q.flat, q.psr, q.gain_prev, q.gain_next = p["flat"], p["psr"], p["gain_prev"], p["gain_next"]
        q.start_sample, q.end_sample, q.first_block = p["start"], p["end"], p["start"] // K
        qs.append(q)
    _, verified, supported, coverage = cr.assess_cut(qs, psr, gain, cov)
    return cr.decide(verified, supported, coverage, cov), coverage, verified


def main() -> None:
    if len(sys.argv) > 2 and sys.argv[1] == "--rescore":  # the recorded device reports, the current thresholds
        from ffsubsync_amd import cut_report as cr

        d = json.load(open(sys.argv[2]))
        _write(d["problems"], d["seeds"], sys.argv[2], cr)
        return
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "cut_report_calibration.json")
    from ffsubsync_amd import cut_report as cr
    from workloads import cuts, splits

    cut = [cuts.make_problem(seed) for seed in range(n + 1)]
    recs = _run("cut", [(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in cut[:n]],
                [lambda q, p=p: _truth_cut(p, q) for p in cut[:n]], cr)
    for r, p in zip(recs, cut):
        r["true_pieces"] = len(p.scenes) + 1
    clean = [splits.make_problem(seed, duration_s=7200.0, clean=True) for seed in range(n)]
    recs += _run("clean", [(p.ref.astype(float), p.sub.astype(float) * p.sub_hi) for p in clean],
                 [lambda q, p=p: int(p.offsets[0]) for p in clean], cr)
    recs += _run("wrong", [(cut[i + 1].ref.astype(float), cut[i].sub.astype(float) * cut[i].sub_hi) for i in range(n)],
                 [lambda q: None for _ in range(n)], cr)
    _write(recs, n, out_path, cr)


def _write(recs, n, out_path, cr):
    """Decisions at the library's default thresholds and the per-class summary of the records, into ``out_path``."""
    psr, gain, cov = cr.DEFAULT_MIN_PIECE_PSR, cr.DEFAULT_MIN_GAIN, cr.DEFAULT_MIN_COVERAGE
    summary = {}
    for cls in ("cut", "clean", "wrong"):
        rs = [r for r in recs if r["class"] == cls]
        ps = [p for r in rs for p in r["pieces"]]
        bs = [b for r in rs for b in r["breaks"]]
        dec = [_decide(r, psr, gain, cov, cr) for r in rs]
        for r, (d, c, v) in zip(rs, dec):
            r["decision"], r["coverage"], r["verified"] = d, c, v
        rng = lambda xs: [min(xs), max(xs)] if xs else None
        s = {"problems": len(rs), "pieces": len(ps), "pieces_per_problem": rng([len(r["pieces"]) for r in rs]),
             "psr_correct": rng([p["psr"] for p in ps if p["correct"]]),
             "psr_wrong": rng([p["psr"] for p in ps if not p["correct"]]),
             "psr_correct_under_10_min": rng([p["psr"] for p in ps if p["correct"] and p["minutes"] < 10]),
             "psr_correct_10_min_or_more": rng([p["psr"] for p in ps if p["correct"] and p["minutes"] >= 10]),
             "gain_true_breaks": rng([b["gain"] for b in bs if b["true"]]),
             "gain_spurious_breaks": rng([b["gain"] for b in bs if not b["true"]]),
             "coverage": rng([r["coverage"] for r in rs]),
             "decisions": {d: sum(r["decision"] == d for r in rs) for d in cr.DECISIONS},
             "verified_wrong_pieces": sum(1 for r in rs for p, v in zip(r["pieces"], r["verified"]) if v and not p["correct"])}
        if cls == "cut":
            s["cut_share"] = s["decisions"]["cut"] / len(rs)
            s["cut_share_seeds_0_7"] = sum(r["decision"] == "cut" for r in rs[:8]) / 8.0
            s["pieces_equal_truth"] = sum(len(r["pieces"]) == r["true_pieces"] for r in rs)
        if cls == "clean":
            s["one_piece_every_seed"] = all(len(r["pieces"]) == 1 for r in rs)
            s["single_at_true_offset"] = sum(r["decision"] == "single" and r["pieces"][0]["correct"] for r in rs)
        if cls == "wrong":
            s["max_psr"] = max(p["psr"] for p in ps)
        summary[cls] = s
        print(cls, json.dumps(s), flush=True)
    with open(out_path, "w") as f:
        json.dump({"generator": "profiles/cut_report_calibration.py", "block_samples": K, "tolerance_samples": TOL,
                   "thresholds": {"min_piece_psr": psr, "min_gain": gain, "min_coverage": cov}, "seeds": n,
                   "summary": summary, "problems": recs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
