"""Calibration of the break refinement's defaults (split_refine.DEFAULT_UNMATCHED_MARGIN / DEFAULT_RADIUS_SAMPLES) on the
CPU models (tests/split_model.py for the DP's coarse breaks, tests/split_refine_model.py for the refinement) and the
seeded workloads of workloads/splits.py.  No GPU.

Per seed: make_problem(seed), 2 h, +-10 min (W = 60 000), K = 1024, P = 8192 (the split's defaults).  The DP's own
block offsets give the coarse breaks; every margin beta (None = a single cut) refines them at each radius.  The cues are
the subtitle vector's runs of ones, mapped as map_cues does (a cue goes to the piece that holds its start sample) with
the coarse pieces, and as map_cues_refined does with the refined cuts.  Per (radius, beta), summed over the seeds:
  wrong   cues outside cut stretches mapped to the wrong piece (coarse and refined)
  found   cues inside cut stretches marked unmatched (of cut_cues)
  false   cues outside cut stretches marked unmatched

    python profiles/split_refine_calibration.py [--seeds 64] [--jobs 8] [--out profiles/split_refine_calibration.json]
"""
import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import split_model as sm  # noqa: E402
import split_refine_model as rm  # noqa: E402
from workloads import splits  # noqa: E402

W, K, P = 60000, 1024, 8192.0
RADII = (13500, 27000, 54000)
BETAS = (None, 0.0, 0.1, 0.25, 0.4, 0.6, 1.0)


def _assign(offsets_by_piece, cuts_t1, cuts_t2, start):
    """Offset and unmatched flag of every cue start with the cuts (t1, t2) per break."""
    t1, t2 = np.asarray(cuts_t1, np.int64), np.asarray(cuts_t2, np.int64)
    k = np.searchsorted(t2, start, side="right")
    lost = start >= np.append(t1, np.iinfo(np.int64).max)[k]  # inside [t1, t2) of the next break
    return np.asarray(offsets_by_piece, np.int64)[k], lost


def _one(seed):
    pr = splits.make_problem(seed)
    offs, _, _, pieces = sm.solve(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, W, P)
    start, _ = rm.sub_cues(pr.sub)
    piece_off = [p[4] for p in pieces]
    cuts = [p[2] for p in pieces[1:]]
    coarse_off, coarse_um = _assign(piece_off, cuts, cuts, start)
    row = dict(seed=seed, n_true=len(pr.breaks), n_found=len(pieces) - 1, kinds=pr.kinds, breaks=pr.breaks,
               dp_cuts=cuts, coarse=rm.cue_errors(pr, start, coarse_off, coarse_um), refined={})
    for radius in RADII:
        for beta in BETAS:
            recs = rm.refine(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), offs, K, radius, beta)
            off, um = _assign(piece_off, recs["t1"], recs["t2"], start)
            e = rm.cue_errors(pr, start, off, um)
            e["cuts"] = [[int(a), int(b)] for a, b in zip(recs["t1"], recs["t2"])]
            e["at_edge"] = int(((recs["flags"] & rm.AT_EDGE) != 0).sum())
            row["refined"]["%d/%s" % (radius, beta)] = e
    return row


def summarize(rows):
    table = {}
    coarse_wrong = sum(r["coarse"]["wrong"] for r in rows)
    for key in rows[0]["refined"]:
        es = [r["refined"][key] for r in rows]
        table[key] = dict(coarse_wrong=coarse_wrong, wrong=sum(e["wrong"] for e in es),
                          worse_problems=sum(e["wrong"] > r["coarse"]["wrong"] for e, r in zip(es, rows)),
                          cut_cues=sum(e["cut_cues"] for e in es), found=sum(e["found"] for e in es),
                          false=sum(e["false"] for e in es), max_false_per_problem=max(e["false"] for e in es),
                          at_edge=sum(e["at_edge"] for e in es))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_refine_calibration.json"))
    a = ap.parse_args()
    with Pool(a.jobs) as pool:
        rows = pool.map(_one, range(a.seeds), chunksize=1)
    res = dict(config=dict(W=W, K=K, P=P, radii=list(RADII), betas=[str(b) for b in BETAS], seeds=a.seeds),
               recovered=sum(r["n_true"] == r["n_found"] for r in rows), table=summarize(rows), rows=rows)
    with open(a.out, "w") as f:  # the summary indented, then one line per seed
        head = json.dumps({k: v for k, v in res.items() if k != "rows"}, indent=1)
        f.write(head[:-2] + ',\n "rows": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in res["rows"])
                + "\n ]\n}\n")
    print(json.dumps(dict(recovered=res["recovered"], table=res["table"]), indent=1))


if __name__ == "__main__":
    main()
