"""Calibration table of drift_refine's radius_samples / unmatched_margin on the CPU models (tests/drift_range_model.py,
tests/drift_range_smooth_model.py, tests/drift_refine_model.py) over the SYNTHETIC problems of workloads/drift_cuts.py.
No GPU: the device equals the models bit for bit (tests/test_gpu_drift_refine.py), so these figures are the device's.

One-hour steep problems (eps = +-6e-4) with 22.5-30 min of inserted scenes and one stretch of 60-240 s removed from the
reference, K = 1024, each pair's full overlap range, the drift solve at DESIGN 3.14's defaults (P = 8192, max_step 2,
step_cost 64), the smooth fit at DESIGN 3.15's (16, 16, 64).  Seeds: ``drift_cuts.seeds(N_SEEDS)``, the first steep
seeds whose removed stretch holds at least 5 cues.  Cues are the runs of ones of the subtitle vector.

Per seed, per path (the DP's block offsets; the smooth fit's) and per beta in (none, 0.1, 0.25, 0.4), at
radius_samples = 27 000: wrong / found / false (``drift_cuts.score_cues``, tolerance 50 samples) of
  block    every cue gets the lag of the block that holds its start (``map_cues_drift``), or the segment's polyline
           there (``map_cues_smooth``); no cue is unmatched
  refined  ``map_cues_drift_refined`` / ``map_cues_smooth_refined`` with the model's records
``totals`` sums them over the seeds, and ``first_four`` over the four seeds tests/test_gpu_drift_refine.py solves.

    python profiles/drift_refine_calibration.py [processes] [--cache DIR]
    # writes profiles/drift_refine_calibration.json
"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cut_model as cm  # noqa: E402
import drift_range_model as drg  # noqa: E402
import drift_range_smooth_model as drsm  # noqa: E402
import drift_refine_model as drm  # noqa: E402
from ffsubsync_amd.drift_align import DriftResult, segments_from_blocks  # noqa: E402
from ffsubsync_amd.drift_smooth import polyline_shift, smooth_segments_from_blocks  # noqa: E402
from workloads import drift_cuts  # noqa: E402

K, P = 1024, 8192.0
MAX_STEP, STEP_COST = 2, 64.0
KNOT_BLOCKS, FIT_RADIUS, BEND_COST = 16, 16, 64.0
RADIUS = 27000
BETAS = (None, 0.1, 0.25, 0.4)
N_SEEDS = 8
CACHE = None


def drift_path(pr):
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size)
    path = CACHE and os.path.join(CACHE, "drift_cuts_%d.npz" % pr.seed)
    if path and os.path.exists(path):
        z = np.load(path)
        return z["off"], z["score"], z["jump"]
    off, score, jump, _ = drg.solve(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, lo, hi, P, MAX_STEP, STEP_COST)
    if path:
        os.makedirs(CACHE, exist_ok=True)
        np.savez(path, off=off, score=score, jump=jump)
    return off, score, jump


def block_mapping(x, segs, lag_of):
    """(offsets, unmatched) of the unrefined mapping: the segment of the block that holds the cue's start."""
    first = np.array([s.first_block for s in segs])
    nb = segs[-1].end_block
    out = np.zeros(x.size)
    for i, xs in enumerate(x):
        b = min(max(int(xs) // K, 0), nb - 1)
        out[i] = lag_of(int(np.searchsorted(first, b, side="right")) - 1, int(xs), b)
    return out, np.zeros(x.size, bool)


def refined_mapping(x, segs, recs, lag_of):
    """(offsets, unmatched) by the refined cuts, as drift_refine._refined_cues."""
    t1, t2 = recs["t1"].astype(np.int64), recs["t2"].astype(np.int64)
    out, um = np.zeros(x.size), np.zeros(x.size, bool)
    for i, xs in enumerate(x):
        k = int(np.searchsorted(t2, xs, side="right"))
        um[i] = k < len(recs) and xs >= t1[k]
        b = min(max(int(xs) // K, segs[k].first_block), segs[k].end_block - 1)
        out[i] = lag_of(k, int(xs), b)
    return out, um


def one_problem(seed):
    pr = drift_cuts.make_problem(seed)
    off, score, jump = drift_path(pr)
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size)
    lv = ((0.0, 1.0), (0.0, pr.sub_hi))
    drift = DriftResult(segments_from_blocks(off, score, jump, K, pr.sub.size), 0.0, off, score, jump)
    cnt = drsm.RangeCounts(pr.ref, pr.sub, lv[0], lv[1], K, lo, hi)
    smooth, knot, srec = drsm.fit(cnt, off, jump, KNOT_BLOCKS, FIT_RADIUS, BEND_COST)
    ssegs = smooth_segments_from_blocks(drift, smooth, knot, srec, K)
    x = pr.cue_start
    paths = (("dp", off, lambda k, xs, b: float(off[b])),
             ("smooth", smooth, lambda k, xs, b: polyline_shift(ssegs[k], float(xs), K)))
    row = dict(seed=seed, ratio=pr.ratio, eps=pr.base.eps, cut_ref=pr.cut_ref, cut_len=pr.cut_len,
               jumps=int(np.asarray(jump)[1:].astype(bool).sum()), cues=int(x.size),
               cut_cues=int(pr.cue_unmatched.sum()), paths={})
    for name, o, lag_of in paths:
        cell = dict(block=drift_cuts.score_cues(pr, x, *block_mapping(x, drift.segments, lag_of)), refined={})
        for beta in BETAS:
            recs = drm.refine(pr.ref, pr.sub, lv[0], lv[1], o, jump, K, RADIUS, beta)
            sc = drift_cuts.score_cues(pr, x, *refined_mapping(x, drift.segments, recs, lag_of))
            sc["at_edge"] = int(((recs["flags"] & drm.AT_EDGE) != 0).sum())
            cell["refined"]["none" if beta is None else "%g" % beta] = sc
        row["paths"][name] = cell
    return row


def total(rows):
    out = {}
    for name in ("dp", "smooth"):
        add = lambda cells: {f: int(sum(c[f] for c in cells)) for f in ("cues", "cut_cues", "wrong", "found", "false")}
        out[name] = dict(block=add([r["paths"][name]["block"] for r in rows]),
                         refined={b: add([r["paths"][name]["refined"][b] for r in rows])
                                  for b in rows[0]["paths"][name]["refined"]})
    return out


def main():
    global CACHE
    args = sys.argv[1:]
    if "--cache" in args:
        i = args.index("--cache")
        CACHE = args[i + 1]
        del args[i:i + 2]
    procs = min(int(args[0]) if args else 8, 16)
    seeds = drift_cuts.seeds(N_SEEDS)
    with multiprocessing.Pool(procs, initializer=_init, initargs=(CACHE,)) as pool:
        rows = pool.map(one_problem, seeds, chunksize=1)
    out = dict(data="SYNTHETIC (workloads/drift_cuts.py)", block_samples=K, split_penalty=P, max_step=MAX_STEP,
               step_cost=STEP_COST, smooth_fit=[KNOT_BLOCKS, FIT_RADIUS, BEND_COST], radius_samples=RADIUS,
               offset_tolerance=drift_cuts.OFFSET_TOL, seeds=seeds, rows=rows, totals=total(rows),
               first_four=total(rows[:4]))
    with open(os.path.join(ROOT, "profiles", "drift_refine_calibration.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(totals=out["totals"], first_four=out["first_four"]), indent=1, sort_keys=True))


def _init(cache):
    global CACHE
    CACHE = cache


if __name__ == "__main__":
    main()
