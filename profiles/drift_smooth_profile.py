"""Timing of the smooth drift fit (ffsubsync_amd.drift_smooth, csrc/ffs_drift_smooth.h) against drift_align_batch on the
same problems and the same pairs in flight, in ONE process, alternating: drifting 2 h problems of workloads/drift.py,
+-10 min window, K = 1024, the defaults; one call of 1 pair and one of 256 pairs (32 distinct problems, tiled).  Per
round each variant is called once, HIP events around the call (the host read-back of the results is inside the window);
best of the rounds, after one untimed warm round.  The yardstick is drift_align_batch in the same run, never the smooth
call itself.  Kernel times come from a separate run under ``rocprofv3 --kernel-trace --stats`` with ``--repeats 1``
(profiles/drift_smooth_kernel_stats.csv).

    python profiles/drift_smooth_profile.py [--out profiles/drift_smooth_profile.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o drift_smooth -- \\
        python profiles/drift_smooth_profile.py --repeats 1 --out /dev/null
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_smooth_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 256])
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import batch, drift_align as da, drift_smooth as ds
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import drift

    w, k = 60000, da.DEFAULT_BLOCK_SAMPLES
    probs = [drift.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    variants = ("drift", "drift_smooth")
    result = {"window_samples": w, "block_samples": k, "split_penalty": da.DEFAULT_SPLIT_PENALTY,
              "max_step": da.DEFAULT_MAX_STEP, "step_cost": da.DEFAULT_STEP_COST, "knot_blocks": ds.DEFAULT_KNOT_BLOCKS,
              "radius": ds.DEFAULT_RADIUS, "bend_cost": ds.DEFAULT_BEND_COST, "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in args.pairs:
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        n_blocks = (db.lens[:, 1] + k - 1) // k
        # one pairs_in_flight for both plans (the smooth workspace is the larger), so the sub-batches are the same
        pif = ds._get_plan(n_pairs, int(n_blocks.max()), 2 * w, int(db.lens[:, 1].max()), None).pairs_in_flight

        def call(name):
            if name == "drift":
                return da.drift_align_batch(db, w, pairs_in_flight=pif)
            return ds.smooth_align_batch(db, w, pairs_in_flight=pif)

        times = {name: [] for name in variants}
        res = {}
        for rnd in range(args.repeats + 1):
            for name in variants:
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                res[name] = call(name)
                stop.record()
                torch.cuda.synchronize()
                if rnd:  # round 0 warms plans and code objects
                    times[name].append(start.elapsed_time(stop))
        same = all(np.array_equal(a.block_offsets, b.drift.block_offsets) and a.total == b.drift.total
                   for a, b in zip(res["drift"], res["drift_smooth"]))
        segs = [len(r.segments) for r in res["drift_smooth"]]
        knots = [sum(len(s.knots) for s in r.segments) for r in res["drift_smooth"]]
        base, fit = min(times["drift"]), min(times["drift_smooth"])
        entry = {"cells": int(n_blocks.sum()) * 2 * w, "pairs_in_flight": pif, "smooth_solve_equals_drift": bool(same),
                 "segments_per_pair": [min(segs), max(segs)], "knots_per_pair": [min(knots), max(knots)],
                 "blocks_moved": int(sum(np.count_nonzero(r.smooth_offsets != r.drift.block_offsets)
                                         for r in res["drift_smooth"])),
                 "drift_workspace_bytes": next(iter(da._plans.plans.values())).workspace_bytes,
                 "smooth_workspace_bytes": next(iter(ds._plans.plans.values())).workspace_bytes,
                 "drift_ms_per_call": base, "drift_times_ms": times["drift"], "smooth_ms_per_call": fit,
                 "smooth_times_ms": times["drift_smooth"], "added_ms_per_call": fit - base,
                 "added_ms_per_pair": (fit - base) / n_pairs, "added_fraction": (fit - base) / base}
        result["calls"][str(n_pairs)] = entry
        print(json.dumps({str(n_pairs): entry}), flush=True)
        da.clear_plan_cache()
        ds.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
