"""Cost of the shuffled-cue null against the solves it feeds -> profiles/null_profile.json.

GPU script: HIP events around whole calls, one warm call first, best and median of several.  On 1 and on 64 two-hour `seven`
problems (workloads/unknown_ratio.py), K = 64, block_units = 1, window 6000 samples, references and tracks prepared once
(``batch_gss.PreparedRatioSolve``; every track rasterised to a boundary list at ratio 1) it times

    lists      ``surrogate.surrogate_lists`` alone: K shuffled lists per file
    null_test  ``surrogate.null_test_lists(..., raw=True)``: lists, files * (K + 1) solves, ``ffs_null_stats``
    evaluate   ``PreparedRatioSolve.evaluate`` of the same number of (file, ratio 1) vectors: rasteriser + solves
    queued     ``surrogate_lists`` QUEUE calls back to back between one pair of events, per call, at block_units 1 and 8:
               what the list kernel costs the device once the host's submission latency is hidden behind it

The only bar: list generation must cost less than the solves it feeds (``null_test`` minus ``lists``).

    python profiles/null_profile.py [--files 1 64] [--repeats 20] [--duration 7200] [--out profiles/null_profile.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffsubsync_amd import surrogate  # noqa: E402
from ffsubsync_amd.aligners import _Vec  # noqa: E402
from ffsubsync_amd.batch_gss import PreparedRatioSolve  # noqa: E402
from workloads import unknown_ratio as ur  # noqa: E402

W, K, QUEUE = 6000, 64, 16


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "null_profile.json"))
    args = ap.parse_args()
    rows = []
    for n in args.files:
        probs = [ur.make_problem("seven", seed, args.duration) for seed in range(n)]
        solver = PreparedRatioSolve([_Vec(p.reference) for p in probs], [p.track for p in probs], W, 100, 0, 1.1, n * (K + 1),
                                    max_cand=1)
        assert solver.use_lists
        ones = np.ones(n)
        data, offs, lens, bounds = solver.tracks.rasterize_runs(np.arange(n), ones, 100, 0)
        sub_ptr = np.uint64(data.data_ptr()) + offs.astype(np.uint64)
        seeds = [surrogate.file_seed(0, i) for i in range(n)]
        table = torch.empty(n * (K + 1) * 24, dtype=torch.uint8, device="cuda")
        which = np.repeat(np.arange(n), K + 1)
        box = {}

        def lists(block_units=1):
            box["lists"] = surrogate.surrogate_lists(sub_ptr, bounds, lens, seeds, K, block_units)

        def null_test():
            box["test"] = surrogate.null_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, sub_ptr, lens, bounds, W, K, 1,
                                                    seeds=seeds, raw=True)

        def evaluate():
            solver.evaluate(which, np.ones(which.size), table)

        (lists_ms, lists_med), (null_ms, null_med), (eval_ms, eval_med) = (timed_ms(f, args.repeats) for f in (lists, null_test, evaluate))
        queued = {b: timed_ms(lambda: lists(b), args.repeats, QUEUE) for b in (1, 8)}
        recs = box["test"].records.cpu().numpy().view(surrogate._native.NULL_RESULT_DTYPE)[:n]
        solves = n * (K + 1)
        rows.append({"files": n, "duration_s": args.duration, "solves": solves, "boundaries_per_list_max": int(bounds.max()),
                     "lists_ms": lists_ms, "lists_ms_median": lists_med, "lists_us_per_list": 1e3 * lists_ms / (n * K),
                     "null_test_ms": null_ms, "null_test_ms_median": null_med, "null_test_us_per_solve": 1e3 * null_ms / solves,
                     "evaluate_ms": eval_ms, "evaluate_ms_median": eval_med, "evaluate_us_per_solve": 1e3 * eval_ms / solves,
                     "lists_queued_us_per_call": {"block_units_%d" % b: {"best": 1e3 * q[0], "median": 1e3 * q[1]}
                                                  for b, q in queued.items()},
                     "chunks": box["test"].stats["chunks"],
                     "trusted": "%d of %d" % (sum(surrogate.trusted(surrogate.record_of(r)) for r in recs), n),
                     "lists_cheaper_than_their_solves": bool(lists_ms < null_ms - lists_ms),
                     "lists_cheaper_than_their_solves_median": bool(lists_med < null_med - lists_med)})
        print(json.dumps(rows[-1]))
    out = {"what": "whole calls between HIP events on one MI355X, warm, best and median of %d; K = %d, block_units 1, window %d "
                   "samples; queued: %d surrogate_lists calls back to back between one pair of events, per call"
                   % (args.repeats, K, W, QUEUE),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
