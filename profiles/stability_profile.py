"""Cost of the half-sample stability test against the solves it feeds -> profiles/stability_profile.json.

GPU script: HIP events around whole calls, one warm call first, best and median of several.  On 1 and on 64 two-hour `seven`
problems (workloads/unknown_ratio.py), K = 64, block_runs = 1, window 6000 samples, references and tracks prepared once
(``batch_gss.PreparedRatioSolve``; every track rasterised to a boundary list at ratio 1) it times

    lists      ``stability.subsample_lists(..., raw=True)`` alone: K thinned lists per file
    stability  ``stability.stability_test_lists(..., raw=True)``: lists, files * (K + 1) solves, ``ffs_offset_stats``
    null_test  ``surrogate.null_test_lists(..., raw=True)`` on the same files: a figure, not a bar
    evaluate   ``PreparedRatioSolve.evaluate`` of the files * K vectors the lists feed: rasteriser + solves
    stats      ``stability.offset_stats(..., raw=True)`` alone on the table of the last stability call
    queued     ``subsample_lists`` QUEUE calls back to back between one pair of events, per call, at block_runs 1 and 8

The only bar: ``lists`` must cost less than ``evaluate`` of the vectors it feeds, by best and by median.  Not measured:
hardware counters, real files.  Every track is rasterised at ratio 1 whatever its true ratio, so ``max_dev_max`` and
``interval_width_max`` of a row describe the workload, not the stability of a sync.

    python profiles/stability_profile.py [--files 1 64] [--repeats 20] [--duration 7200] [--out profiles/stability_profile.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffsubsync_amd import stability, surrogate  # noqa: E402
from ffsubsync_amd.aligners import _Vec  # noqa: E402
from ffsubsync_amd.batch_gss import PreparedRatioSolve  # noqa: E402
from workloads import unknown_ratio as ur  # noqa: E402

W, K, QUEUE, TOL = 6000, 64, 16, 8


def timed_ms(fn, repeats, calls=1):
    """(best, median) milliseconds per call of ``fn``, ``calls`` of them queued between one pair of events."""
    fn()  # warm: plans, allocator, code objects
    torch.cuda.synchronize()
    took = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        took.append(a.elapsed_time(b) / calls)
    return min(took), float(np.median(took))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--duration", type=float, default=7200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stability_profile.json"))
    args = ap.parse_args()
    rows = []
    for n in args.files:
        probs = [ur.make_problem("seven", seed, args.duration) for seed in range(n)]
        solver = PreparedRatioSolve([_Vec(p.reference) for p in probs], [p.track for p in probs], W, 100, 0, 1.1, n * (K + 1),
                                    max_cand=1)
        assert solver.use_lists
        data, offs, lens, bounds = solver.tracks.rasterize_runs(np.arange(n), np.ones(n), 100, 0)
        sub_ptr = np.uint64(data.data_ptr()) + offs.astype(np.uint64)
        seeds = [surrogate.file_seed(0, i) for i in range(n)]
        table = torch.empty(n * K * 24, dtype=torch.uint8, device="cuda")
        which = np.repeat(np.arange(n), K)  # the vectors the lists feed
        box = {}

        def lists(block_runs=1):
            box["lists"] = stability.subsample_lists(sub_ptr, bounds, lens, seeds, K, block_runs, raw=True)

        def stab():
            box["test"] = stability.stability_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, sub_ptr, lens, bounds, W, K,
                                                         1, tol=TOL, seeds=seeds, raw=True)

        def null_test():
            box["null"] = surrogate.null_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, sub_ptr, lens, bounds, W, K, 1,
                                                    seeds=seeds, raw=True)

        def evaluate():
            solver.evaluate(which, np.ones(which.size), table)

        def stats():
            box["stats"] = stability.offset_stats(box["test"].table, n, K, TOL, raw=True)

        t = {name: timed_ms(f, args.repeats) for name, f in (("lists", lists), ("stability", stab), ("null_test", null_test),
                                                             ("evaluate", evaluate), ("stats", stats))}
        queued = {b: timed_ms(lambda: lists(b), args.repeats, QUEUE) for b in (1, 8)}
        recs = box["test"].records.cpu().numpy().view(stability._native.STABILITY_RESULT_DTYPE)[:n]
        row = {"files": n, "duration_s": args.duration, "solves": n * (K + 1), "vectors_fed": n * K,
               "boundaries_per_list_max": int(bounds.max()), "chunks": box["test"].stats["chunks"],
               "lists_us_per_list": 1e3 * t["lists"][0] / (n * K),
               "lists_queued_us_per_call": {"block_runs_%d" % b: {"best": 1e3 * q[0], "median": 1e3 * q[1]} for b, q in queued.items()},
               "stability_over_null_test": t["stability"][0] / t["null_test"][0],
               "max_dev_max": int(recs["max_dev"].max()), "interval_width_max": int((recs["off_hi"] - recs["off_lo"]).max()),
               "lists_cheaper_than_evaluate": bool(t["lists"][0] < t["evaluate"][0]),
               "lists_cheaper_than_evaluate_median": bool(t["lists"][1] < t["evaluate"][1])}
        for name, (best, med) in t.items():
            row[name + "_ms"], row[name + "_ms_median"] = best, med
        rows.append(row)
        print(json.dumps(row))
    out = {"what": "whole calls between HIP events on one MI355X, warm, best and median of %d; K = %d, block_runs 1, window %d "
                   "samples; queued: %d subsample_lists calls back to back between one pair of events, per call; not measured: "
                   "hardware counters, real files" % (args.repeats, K, W, QUEUE),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
