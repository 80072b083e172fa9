"""Timing of sample-exact break refinement (ffsubsync_amd.split_refine, csrc/ffs_split_refine.h) at the defaults: 2 h
problems of workloads/splits.py, +-10 min window (W = 60 000), K = 1024, P = 8192, radius 27 000, margin 0.25.  The split
is solved once per size; then one refine call of 1 pair and one of 256 pairs (32 distinct problems, tiled), each timed
with HIP events (warm: one untimed call first), best of the repeats, for
  - the device call alone (SplitPlan.refine on buffers allocated up front: the two kernels plus the descriptor upload),
  - the Python call refine_breaks_batch (block offsets uploaded, records read back and unpacked).
Run it once under ``rocprofv3 --kernel-trace --stats`` for k_refine_breaks / k_refine_cut on their own.

    python profiles/split_refine_profile.py [--out profiles/split_refine_profile.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _best(fn, repeats):
    import torch

    fn()  # warm: plan, code objects
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return min(times), times, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_refine_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import _native, batch, split_align as sa, split_refine as sr
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import splits

    w, k = 60000, sa.DEFAULT_BLOCK_SAMPLES
    radius, beta = sr.DEFAULT_RADIUS_SAMPLES, sr.DEFAULT_UNMATCHED_MARGIN
    probs = [splits.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    result = {"window_samples": w, "block_samples": k, "split_penalty": sa.DEFAULT_SPLIT_PENALTY,
              "radius_samples": radius, "unmatched_margin": beta, "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 256):
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        res = sa.split_align_batch(db, w)
        sa.clear_plan_cache()
        ms_py, t_py, brks = _best(lambda: sr.refine_breaks_batch(db, res), args.repeats)
        # the device call alone
        sl = db.lens[:, 1].astype(np.int64)
        max_b = int((-(-sl // k)).max())
        offs = np.zeros((n_pairs, max_b), np.int32)
        for p, r in enumerate(res):
            offs[p, :r.block_offsets.size] = r.block_offsets
        dev = db.data.device
        offs_d = torch.from_numpy(offs.reshape(-1)).to(dev)
        rec = torch.empty(n_pairs * max_b * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev)
        cnt = torch.empty(n_pairs, dtype=torch.int32, device=dev)
        plan = sr._get_plan(n_pairs)
        call = lambda: plan.refine(*db.pair_arrays(), k, offs_d, radius, beta, rec, cnt)
        ms_dev, t_dev, _ = _best(call, args.repeats)
        n_brk = sum(len(b) for b in brks)
        result["calls"][str(n_pairs)] = {
            "device_call": {"ms_per_call": ms_dev, "us_per_break": 1000.0 * ms_dev / max(n_brk, 1), "times_ms": t_dev},
            "python_call": {"ms_per_call": ms_py, "times_ms": t_py},
            "breaks": n_brk, "unmatched_breaks": sum(b.t1 < b.t2 for bb in brks for b in bb),
            "pairs_in_flight": plan.pairs_in_flight, "max_blocks": max_b,
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
    sr.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
