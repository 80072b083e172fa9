"""Timing of the split solve's per-piece quality report (ffsubsync_amd.split_report, csrc/ffs_split_report.h) at the
defaults: 2 h problems of workloads/splits.py, +-10 min window (W = 60 000), K = 1024, P = 8192, top_k 3, E = 300.  One
call of 1 pair and one of 256 pairs (32 distinct problems, tiled), each timed with HIP events around the call (warm: one
untimed call first), best of three, for
  - the plain split call (split_align_batch) at its own pairs_in_flight,
  - the plain split call at the report call's pairs_in_flight (the report's workspace is 3x the split's per pair, so
    fewer pairs are in flight), and
  - the report call (split_report_batch),
so that the report's added time per pair is report - plain at the same pairs_in_flight.  Run it once under
``rocprofv3 --kernel-trace --stats`` for the split between k_split_pieces / k_split_piece_sums / k_split_piece_report.

    python profiles/split_report_profile.py [--out profiles/split_report_profile.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_report_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import batch, split_align as sa, split_report as sr
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import splits

    w, k = 60000, sa.DEFAULT_BLOCK_SAMPLES
    probs = [splits.make_problem(seed) for seed in range(args.distinct)]
    rasters = [(DeviceRaster.from_host(p.ref.astype(float), lists=False),
                [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]) for p in probs]
    result = {"window_samples": w, "block_samples": k, "split_penalty": sa.DEFAULT_SPLIT_PENALTY,
              "top_k": sr.DEFAULT_TOP_K, "exclusion_samples": sr.DEFAULT_EXCLUSION_SAMPLES,
              "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 256):
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        ms_r, t_r, reps = _best(lambda: sr.split_report_batch(db, w), args.repeats)
        rplan = sa._plans.plans[(torch.cuda.current_device(), "report")]
        pif, ws_r = rplan.pairs_in_flight, rplan.workspace_bytes
        sa.clear_plan_cache()
        ms_p, t_p, _ = _best(lambda: sa.split_align_batch(db, w), args.repeats)
        pplan = sa._plans.plans[(torch.cuda.current_device(), None)]
        pif_p, ws_p = pplan.pairs_in_flight, pplan.workspace_bytes
        sa.clear_plan_cache()
        ms_q, t_q, _ = _best(lambda: sa.split_align_batch(db, w, pairs_in_flight=pif), args.repeats)
        sa.clear_plan_cache()
        breaks = [sum(sr.break_support(r.pieces)) for r in reps]
        true = [len(probs[i % len(probs)].breaks) for i in range(n_pairs)]
        result["calls"][str(n_pairs)] = {
            "report": {"ms_per_call": ms_r, "ms_per_pair": ms_r / n_pairs, "times_ms": t_r, "pairs_in_flight": pif,
                       "workspace_bytes": ws_r},
            "plain": {"ms_per_call": ms_p, "ms_per_pair": ms_p / n_pairs, "times_ms": t_p, "pairs_in_flight": pif_p,
                      "workspace_bytes": ws_p},
            "plain_same_pairs_in_flight": {"ms_per_call": ms_q, "ms_per_pair": ms_q / n_pairs, "times_ms": t_q},
            "report_added_ms_per_pair": (ms_r - ms_q) / n_pairs,
            "pieces": sum(len(r.pieces) for r in reps), "supported_breaks": sum(breaks), "true_breaks": sum(true),
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
