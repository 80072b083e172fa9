"""Timing of the split-aware aligner (ffsubsync_amd.split_align, csrc/ffs_split.h) at the defaults: 2 h problems of
workloads/splits.py, +-10 min window (W = 60 000), K = 1024, P = 8192.  One call of 1 pair and one of 256 pairs (32
distinct problems, tiled), each timed with HIP events around the native call (warm: one untimed call first), best of
three.  Run it once under ``rocprofv3 --kernel-trace --stats`` for the split between k_split_prefix / k_split_counts /
k_split_dp.

    python profiles/split_profile.py [--out profiles/split_profile.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import batch, split_align as sa
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import splits

    w, k = 60000, sa.DEFAULT_BLOCK_SAMPLES
    probs = [splits.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    result = {"window_samples": w, "block_samples": k, "split_penalty": sa.DEFAULT_SPLIT_PENALTY,
              "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 256):
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        sub_len = db.lens[:, 1]
        blocks = int(((sub_len + k - 1) // k).sum())
        sa.split_align_batch(db, w)  # warm: plan, code objects
        plan = next(iter(sa._plans.plans.values()))
        times = []
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            res = sa.split_align_batch(db, w)  # (the host read-back of the results is inside the window)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        ok = sum(not splits.check_recovery(probs[i % len(probs)], r.block_offsets, k) for i, r in enumerate(res))
        ms = min(times)
        result["calls"][str(n_pairs)] = {
            "ms_per_call": ms, "ms_per_pair": ms / n_pairs, "times_ms": times,
            "cells": blocks * 2 * w, "cells_per_s_end_to_end": blocks * 2 * w / (ms * 1e-3),
            "pairs_in_flight": plan.pairs_in_flight, "workspace_bytes": plan.workspace_bytes,
            "recovered": ok,
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
        sa.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
