"""Timing of the per-piece report over the full lag range (ffsubsync_amd.cut_report, csrc/ffs_cut_report.h): 2 h
problems of workloads/cuts.py, every pair's full overlap range, K = 1024, the default penalty, top_k 3, E = 300.  One
call of 1 pair and one of 64 pairs (16 distinct problems, tiled), each timed with HIP events around the call (warm: one
untimed call first), best of three, for the plain range split (split_align_range_batch) at the report plan's
pairs_in_flight and for the report call (split_range_report_batch); the report's added time is the difference.  Run it
once under ``rocprofv3 --kernel-trace --stats`` for the split between the kernels.

    python profiles/cut_report_profile.py [--out profiles/cut_report_profile.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _best(fn, repeats):
    import torch

    fn()  # warm: plan, code objects
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()  # (the host read-back of the results is inside the window)
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return min(times), times, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_report_profile.json"))
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", default="1,64")
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import batch, cut_align as ca, cut_report as cr
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import cuts

    probs = [cuts.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    result = {"block_samples": 1024, "split_penalty": ca.DEFAULT_CUT_PENALTY, "top_k": cr.DEFAULT_TOP_K,
              "exclusion_samples": cr.DEFAULT_EXCLUSION_SAMPLES, "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in [int(x) for x in args.pairs.split(",")]:
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        ms_r, t_r, reps = _best(lambda: cr.split_range_report_batch(db), args.repeats)
        plan = cr._plans.plans[(torch.cuda.current_device(), "report")]
        pif, ws = plan.pairs_in_flight, plan.workspace_bytes
        cr.clear_plan_cache()
        ms_p, t_p, _ = _best(lambda: ca.split_align_range_batch(db, pairs_in_flight=pif), args.repeats)
        ca.clear_plan_cache()
        pieces = sum(len(r.pieces) for r in reps)
        result["calls"][str(n_pairs)] = {
            "report": {"ms_per_call": ms_r, "ms_per_pair": ms_r / n_pairs, "times_ms": t_r, "pairs_in_flight": pif,
                       "workspace_bytes": ws},
            "plain_same_pairs_in_flight": {"ms_per_call": ms_p, "ms_per_pair": ms_p / n_pairs, "times_ms": t_p},
            "report_added_ms_per_pair": (ms_r - ms_p) / n_pairs, "added_share": (ms_r - ms_p) / ms_p,
            "pieces": pieces, "max_pieces_per_pair": max(len(r.pieces) for r in reps),
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
