"""Timing of the drift-tolerant aligner (ffsubsync_amd.drift_align, csrc/ffs_drift.h) against the split aligner in ONE
process, alternating: the problems of profiles/split_profile.py (2 h problems of workloads/splits.py, +-10 min window,
K = 1024, P = 8192), one call of 1 pair and one of 256 pairs (32 distinct problems, tiled).  Per round every variant --
split_align_batch, then drift_align_batch at max_step 0, 2 and 7 -- is called once, HIP events around the call (the host
read-back of the results is inside the window); best of the rounds, after one untimed warm round.  Kernel times come
from a separate run of this script under ``rocprofv3 --kernel-trace --stats`` with ``--repeats 1``; its stats CSV has
ONE k_drift_dp row for the three max_step values, so ``--by-variant`` splits the kernel trace by dispatch order.

    python profiles/drift_profile.py [--out profiles/drift_profile.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o drift -- python profiles/drift_profile.py --repeats 1 --out /dev/null
    python profiles/drift_profile.py --by-variant DIR/.../drift_kernel_trace.csv --out profiles/drift_kernel_by_variant.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def by_variant(trace_csv: str, out: str) -> None:
    """DP kernel times of a traced ``--repeats 1`` run at the default ``--pairs``, by variant.  Dispatch order: 1 pair --
    two rounds of (split, step 0, 2, 7), one dispatch each; 256 pairs at 56 in flight -- two rounds of five dispatches
    per variant.  The first round of either is the warm one and is left out."""
    import csv

    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    ns = lambda name: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if name in r["Kernel_Name"]]
    dr, sp = ns("k_drift_dp"), ns("k_split_dp")
    assert len(dr) == 36 and len(sp) == 12, (len(dr), len(sp))
    res = {"1": {"k_split_dp_ns": sp[1]}, "256": {"k_split_dp_ns_per_call": sum(sp[7:12])}}
    for i, name in enumerate(("step0", "step2", "step7")):
        res["1"]["k_drift_dp_%s_ns" % name] = dr[3 + i]
        res["256"]["k_drift_dp_%s_ns_per_call" % name] = sum(dr[21 + 5 * i: 26 + 5 * i])
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--by-variant", metavar="KERNEL_TRACE_CSV", help="split a traced run's DP kernel times by variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 256])
    args = ap.parse_args()
    if args.by_variant:
        by_variant(args.by_variant, args.out)
        return
    import torch

    from ffsubsync_amd import batch, drift_align as da, split_align as sa
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import splits

    w, k = 60000, sa.DEFAULT_BLOCK_SAMPLES
    probs = [splits.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    variants = [("split", None), ("drift_step0", 0), ("drift_step2", 2), ("drift_step7", 7)]
    result = {"window_samples": w, "block_samples": k, "split_penalty": sa.DEFAULT_SPLIT_PENALTY,
              "step_cost": da.DEFAULT_STEP_COST, "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in args.pairs:
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        blocks = int(((db.lens[:, 1] + k - 1) // k).sum())
        # one pairs_in_flight for both plans (the drift workspace is the larger), so the sub-batches are the same
        pif = da._get_plan(n_pairs, int(((db.lens[:, 1] + k - 1) // k).max()), 2 * w, int(db.lens[:, 1].max()), None).pairs_in_flight

        def call(step):
            if step is None:
                return sa.split_align_batch(db, w, pairs_in_flight=pif)
            return da.drift_align_batch(db, w, max_step=step, pairs_in_flight=pif)

        times = {name: [] for name, _ in variants}
        res = {}
        for rnd in range(args.repeats + 1):
            for name, step in variants:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                res[name] = call(step)
                stop.record()
                torch.cuda.synchronize()
                if rnd:  # round 0 warms plans and code objects
                    times[name].append(start.elapsed_time(stop))
        same0 = all(np.array_equal(a.block_offsets, b.block_offsets) and a.total == b.total
                    for a, b in zip(res["split"], res["drift_step0"]))
        entry = {"cells": blocks * 2 * w, "pairs_in_flight": pif, "step0_equals_split": bool(same0),
                 "split_workspace_bytes": next(iter(sa._plans.plans.values())).workspace_bytes,
                 "drift_workspace_bytes": next(iter(da._plans.plans.values())).workspace_bytes, "variants": {}}
        base = min(times["split"])
        for name, _ in variants:
            ms = min(times[name])
            entry["variants"][name] = {"ms_per_call": ms, "times_ms": times[name], "ratio_to_split": ms / base,
                                       "cells_per_s_end_to_end": blocks * 2 * w / (ms * 1e-3)}
        entry["recovered_split"] = sum(not splits.check_recovery(probs[i % len(probs)], r.block_offsets, k)
                                       for i, r in enumerate(res["split"]))
        entry["pairs_with_a_step_at_2"] = sum(bool(np.any((np.diff(r.block_offsets) != 0) & (r.block_jump[1:] == 0)))
                                              for r in res["drift_step2"])
        result["calls"][str(n_pairs)] = entry
        print(json.dumps({str(n_pairs): entry}), flush=True)
        sa.clear_plan_cache()
        da.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
