"""Timing of ffs_drift_refine_batch (ffsubsync_amd.drift_refine, csrc/ffs_drift_refine.h) against the yardstick of the same
run, ffs_split_refine_batch, at the defaults (K = 1024, radius 27 000, margin 0.25); one process, per row a warm round,
then 5 rounds that run the variants in turn, every call between two HIP events, the median of the 5.

  flat      2 h problems of workloads/splits.py, split solve at +-10 min (W = 60 000, P = 8192): the split's offsets with a
            jump flag wherever they change.  Both calls do identical work and return identical bytes (checked here), so
            the ratio isolates the per-block lag lookup.
  drifting  2 h problems of workloads/drift.py with an inserted stretch, drift solve at +-10 min: the DP's own path and
            jump flags.  The split call has no meaning on such a path (every step is a break to it); the row gives the
            new call alone.
Each at 1 pair and at 256 pairs (32 distinct problems solved once, tiled).  Device calls on buffers allocated up front
(SplitPlan.refine / SplitPlan.drift_refine: the two kernels plus the descriptor upload).  There is no bar.

    python profiles/drift_refine_profile.py [--out profiles/drift_refine_profile.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 5


def _time(fn):
    import torch

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def _median_in_turn(variants):
    """{name: (median ms, the times)}: a warm round, then ROUNDS rounds running every variant in turn."""
    for fn in variants.values():
        _time(fn)
    times = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            times[name].append(_time(fn))
    return {name: (float(np.median(t)), t) for name, t in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drift_refine_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import _native, batch, drift_align as da, drift_refine as dref, split_align as sa
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import drift, splits

    w, k = 60000, sa.DEFAULT_BLOCK_SAMPLES
    radius, beta = dref.DEFAULT_RADIUS_SAMPLES, dref.DEFAULT_UNMATCHED_MARGIN
    result = {"window_samples": w, "block_samples": k, "radius_samples": radius, "unmatched_margin": beta,
              "rounds": ROUNDS, "device": torch.cuda.get_device_name(0), "rows": {}}

    def rasters(probs):
        return [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                 [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]

    def paths(name):
        if name == "flat":
            ras = rasters([splits.make_problem(seed) for seed in range(args.distinct)])
            res = sa.split_align_batch(batch.pack_pairs(ras), w)
            sa.clear_plan_cache()
            return ras, [(r.block_offsets, np.concatenate([[0], r.block_offsets[1:] != r.block_offsets[:-1]])) for r in res]
        ras = rasters([drift.make_problem(seed, insert_break=True) for seed in range(args.distinct)])
        res = da.drift_align_batch(batch.pack_pairs(ras), w)
        da.clear_plan_cache()
        return ras, [(r.block_offsets, r.block_jump) for r in res]

    for name in ("flat", "drifting"):
        ras, solved = paths(name)
        for n_pairs in (1, 256):
            db = batch.pack_pairs([ras[i % len(ras)] for i in range(n_pairs)])
            sl = db.lens[:, 1].astype(np.int64)
            max_b = int((-(-sl // k)).max())
            offs, jumps = np.zeros((n_pairs, max_b), np.int32), np.zeros((n_pairs, max_b), np.uint8)
            for p in range(n_pairs):
                o, j = solved[p % len(solved)]
                offs[p, :o.size], jumps[p, :o.size] = o, np.asarray(j) != 0
            dev = db.data.device
            offs_d, jumps_d = torch.from_numpy(offs.reshape(-1)).to(dev), torch.from_numpy(jumps.reshape(-1)).to(dev)
            new_out = lambda: (torch.empty(n_pairs * max_b * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev),
                               torch.empty(n_pairs, dtype=torch.int32, device=dev))
            (rec_d, cnt_d), (rec_s, cnt_s) = new_out(), new_out()
            plan = dref._get_plan(n_pairs)
            a = db.pair_arrays()
            variants = {"drift_refine": lambda: plan.drift_refine(*a, k, offs_d, jumps_d, radius, beta, rec_d, cnt_d)}
            if name == "flat":
                variants["split_refine"] = lambda: plan.refine(*a, k, offs_d, radius, beta, rec_s, cnt_s)
            got = _median_in_turn(variants)
            n_jumps = int(cnt_d.cpu().numpy().sum())
            row = {"pairs": n_pairs, "pairs_in_flight": plan.pairs_in_flight, "max_blocks": max_b, "jumps": n_jumps,
                   "offset_changes": sum(int((np.diff(solved[p % len(solved)][0].astype(np.int64)) != 0).sum())
                                         for p in range(n_pairs))}
            for v, (ms, t) in got.items():
                row[v] = {"ms_per_call": ms, "us_per_jump": 1000.0 * ms / max(n_jumps, 1), "times_ms": t}
            if name == "flat":
                row["identical_bytes"] = bool(torch.equal(rec_d, rec_s) and torch.equal(cnt_d, cnt_s))
                row["ratio"] = got["drift_refine"][0] / got["split_refine"][0]
            result["rows"]["%s_%d" % (name, n_pairs)] = row
            print(json.dumps({"%s_%d" % (name, n_pairs): row}))
    dref.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
