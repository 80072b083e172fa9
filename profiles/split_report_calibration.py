"""Calibration of the split report's default thresholds (split_report.DEFAULT_MIN_GAIN / DEFAULT_MIN_PIECE_PSR) on the CPU
model (tests/split_report_model.py) and the seeded workloads of workloads/splits.py.  No GPU.

Classes, 64 seeds each, +-10 min (W = 60 000), K = 1024, top_k 3, E = 300:
  split        make_problem(seed), 2 h, P = 8192 (the default): every found break should be supported
  clean_lowP   make_problem(seed, clean=True), 10 min and 2 h, P = 1000 (low, to provoke spurious pieces)
  wrong        the subtitle of seed i against the reference of seed i+1, 10 min and 2 h, P = 8192
Per class: the range of the piece psr, and of the break gain min(gain_next_i, gain_prev_{i+1}) over all breaks.

    python profiles/split_report_calibration.py [--seeds 64] [--jobs 8] [--out profiles/split_report_calibration.json]
"""
import argparse
import json
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import split_report_model as srm  # noqa: E402
from ffsubsync_amd import split_report  # noqa: E402
from workloads import splits  # noqa: E402

W, K, TOP_K, E = 60000, 1024, 3, 300
LOW_P, DEFAULT_P = 1000.0, 8192.0


def _one(job):
    cls, dur, seed = job
    if cls == "split":
        pr = splits.make_problem(seed, duration_s=dur)
        ref, sub, hi, p = pr.ref, pr.sub, pr.sub_hi, DEFAULT_P
    elif cls == "clean_lowP":
        pr = splits.make_problem(seed, duration_s=dur, clean=True)
        ref, sub, hi, p = pr.ref, pr.sub, pr.sub_hi, LOW_P
    else:
        a = splits.make_problem(seed, duration_s=dur, clean=True)
        b = splits.make_problem(seed + 1, duration_s=dur, clean=True)
        ref, sub, hi, p = b.ref, a.sub, a.sub_hi, DEFAULT_P
    (offs, _, _, _), recs, _ = srm.report(ref, sub, (0.0, 1.0), (0.0, hi), K, W, p, TOP_K, E)
    pq = [split_report.from_record(r) for r in recs]
    gains = [min(x.gain_next, y.gain_prev) for x, y in zip(pq[:-1], pq[1:])]
    out = dict(cls=cls, duration_s=dur, seed=seed, n_pieces=len(pq), psr=[x.psr for x in pq], break_gain=gains,
               offsets=[x.offset for x in pq], own_is_peak=[x.own_is_peak for x in pq])
    if cls == "split":
        out["truth_offsets"] = pr.offsets
        out["recovered"] = not splits.check_recovery(pr, offs, K, block_tol=4)
    elif cls == "clean_lowP":
        out["truth_offsets"] = pr.offsets
    return out


def _rng(v):
    v = [x for x in v if not math.isnan(x)]
    return [min(v), max(v)] if v else None


def summarize(rows):
    table = {}
    for key in sorted({(r["cls"], r["duration_s"]) for r in rows}):
        rs = [r for r in rows if (r["cls"], r["duration_s"]) == key]
        table["%s_%dmin" % (key[0], key[1] // 60)] = dict(
            n=len(rs), pieces=[min(r["n_pieces"] for r in rs), max(r["n_pieces"] for r in rs)],
            with_breaks=sum(r["n_pieces"] > 1 for r in rs),
            piece_psr=_rng([x for r in rs for x in r["psr"]]),
            break_gain=_rng([x for r in rs for x in r["break_gain"]]),
            # the psr of the pieces of problems the DP did not split: what "split" with one piece rests on
            one_piece_psr=_rng([r["psr"][0] for r in rs if r["n_pieces"] == 1]),
            recovered=sum(r.get("recovered", False) for r in rs) if key[0] == "split" else None)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_report_calibration.json"))
    a = ap.parse_args()
    jobs = [("split", 7200.0, s) for s in range(a.seeds)]
    for dur in (600.0, 7200.0):
        jobs += [("clean_lowP", dur, s) for s in range(a.seeds)] + [("wrong", dur, s) for s in range(a.seeds)]
    jobs.sort(key=lambda j: -j[1])  # the 2 h problems first
    with Pool(a.jobs) as pool:
        rows = pool.map(_one, jobs, chunksize=1)
    res = dict(config=dict(W=W, K=K, top_k=TOP_K, E=E, low_P=LOW_P, default_P=DEFAULT_P, seeds=a.seeds),
               table=summarize(rows), rows=rows)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["table"], indent=1))


if __name__ == "__main__":
    main()
