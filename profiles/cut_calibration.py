"""CPU calibration of cut_sync's split penalty over the full lag range: the numpy models
(tests/cut_model.py, tests/split_refine_model.py) on workloads/cuts.py problems, 2 h, K = 1024, every pair's full
overlap range [-(S-1), R-1], the refine defaults, P = 8192 (split_align's default; a first sweep over 5 seeds put
P = 2048 at about three times the true piece count and P >= 32768 at a quarter of it or less).  Per seed: matched cues
at their exact true offset and within 2 samples of it (the synthetic cues' edges are jittered by up to 10 samples, so a
short piece's correlation peak can sit a sample or two off), cut-scene cues reported unmatched, false unmatched cues,
and pieces found against true pieces.

    python profiles/cut_calibration.py [n_seeds=32] [procs=8] [out=profiles/cut_calibration.json]

Seeds alternate direction (even: theatrical subtitle on the extended video, odd: the other way round).  The model's
subtitle vector is the true-ratio candidate (what the windowless seven-ratio solve picks on every seed here)."""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cut_model as cm  # noqa: E402
import split_refine_model as rm  # noqa: E402
from workloads import cuts  # noqa: E402

K = 1024
PENALTIES = [8192.0]
RADIUS, BETA = 27000, 0.25


def solve_multi(p, penalties):
    """cut_model.solve for several penalties, sharing the score rows: [(block offsets, total)] per penalty."""
    n_blocks = p.n_blocks
    m0 = p.scores(0)
    vs = [m0.copy() for _ in penalties]
    stays = [[] for _ in penalties]
    args = [np.zeros(n_blocks, np.int64) for _ in penalties]
    for b in range(1, n_blocks):
        m = p.scores(b)
        for i, pen in enumerate(penalties):
            v = vs[i]
            j = cm._last_argmax(v)
            args[i][b - 1] = j
            t = v[j] - np.float64(pen)
            st = v >= t
            stays[i].append(np.packbits(st))
            vs[i] = np.where(st, v, t) + m
    out = []
    for i in range(len(penalties)):
        end = cm._last_argmax(vs[i])
        o = np.zeros(n_blocks, np.int64)
        o[-1] = end
        for b in range(n_blocks - 1, 0, -1):
            row = stays[i][b - 1]
            bit = (row[o[b] >> 3] >> (7 - (o[b] & 7))) & 1
            o[b - 1] = o[b] if bit else args[i][b - 1]
        out.append((o + p.lo, float(vs[i][end])))
    return out


def one(seed):
    pr = cuts.make_problem(seed)
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size)
    lv_r, lv_s = (0.0, 1.0), (0.0, pr.sub_hi)
    p = cm._Pair(pr.ref, pr.sub, lv_r, lv_s, K, lo, hi)
    samples = cuts.cue_samples(pr.track, pr.ratio)
    rec = {"seed": seed, "direction": pr.direction, "scenes": len(pr.scenes), "total_scene_s": sum(l for _, l in pr.scenes) / 100.0,
           "true_pieces": len(pr.scenes) + 1, "per_penalty": {}}
    for pen, (offs, total) in zip(PENALTIES, solve_multi(p, PENALTIES)):
        recs = rm.refine(pr.ref, pr.sub, lv_r, lv_s, offs, K, RADIUS, BETA)
        t1 = np.array([int(r["t1"]) for r in recs], np.int64)
        t2 = np.array([int(r["t2"]) for r in recs], np.int64)
        starts = [0] + [int(b) * K for b in rm.breaks_of(offs)]
        piece_off = [int(offs[s // K]) for s in starts]
        got_off = np.zeros(samples.size, np.int64)
        got_um = np.zeros(samples.size, bool)
        for i, x in enumerate(samples):
            k = int(np.searchsorted(t2, x, side="right"))
            got_um[i] = k < t1.size and x >= t1[k]
            got_off[i] = piece_off[k]
        sc = cuts.score_cues(pr, got_off, got_um)
        m = ~pr.cue_unmatched
        sc["within2"] = int(np.sum(m & ~got_um & (np.abs(got_off - pr.cue_offset) <= 2)))
        sc["pieces"] = len(starts)
        sc["offsets"] = [int(x) for x in sorted(set(piece_off))][:64]
        rec["per_penalty"]["%g" % pen] = sc
    print(seed, pr.direction, {k: (v["exact"], v["within2"], v["matched_cues"], v["found"], v["cut_cues"], v["pieces"])
                               for k, v in rec["per_penalty"].items()}, "true pieces", rec["true_pieces"], flush=True)
    return rec


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    out = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cut_calibration.json")
    with Pool(procs) as pool:
        recs = pool.map(one, range(n))
    summary = {}
    for pen in PENALTIES:
        key = "%g" % pen
        tot = {f: sum(r["per_penalty"][key][f] for r in recs) for f in ("matched_cues", "exact", "cut_cues", "found",
                                                                          "false_unmatched", "missed", "within2")}
        for d in ("up", "down"):
            rs = [r for r in recs if r["direction"] == d]
            tot["exact_share_" + d] = sum(r["per_penalty"][key]["exact"] for r in rs) / max(1, sum(
                r["per_penalty"][key]["matched_cues"] for r in rs))
        tot["exact_share"] = tot["exact"] / tot["matched_cues"]
        tot["within2_share"] = tot["within2"] / tot["matched_cues"]
        tot["found_share"] = tot["found"] / max(1, tot["cut_cues"])
        tot["pieces_equal_truth"] = sum(r["per_penalty"][key]["pieces"] == r["true_pieces"] for r in recs)
        tot["min_exact_share_per_seed"] = min(r["per_penalty"][key]["exact"] / r["per_penalty"][key]["matched_cues"] for r in recs)
        summary[key] = tot
    json.dump({"generator": "profiles/cut_calibration.py", "block_samples": K, "radius": RADIUS, "beta": BETA,
               "penalties": PENALTIES, "seeds": n, "summary": summary, "per_seed": recs}, open(out, "w"), indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
