"""Timing of the joint cue retiming (ffsubsync_amd.cue_retime, csrc/ffs_cue_retime.h) at the calibrated defaults:
2 h problems of workloads/cue_stretches.py behind the true sync (about 870 cues each), one call of 1 problem and one of
256 problems (32 distinct, tiled).  HIP events around the device call on buffers allocated up front, a warm call first,
the best of the repeats.  On the same inputs in the same process: ffs_cue_report_batch at the retime's radius and
context (k_cue_report walks the same word-lag steps as k_retime_profile), and a device-to-device copy of the profile's
bytes (4 per (cue, shift)) for the copy rate the extra store traffic is judged by.

The split by kernel comes from a separate run under ``rocprofv3 --kernel-trace --stats`` and is folded in afterwards:

    python profiles/cue_retime_profile.py [--out profiles/cue_retime_profile.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cue_retime -- \\
        python profiles/cue_retime_profile.py --repeats 1 --distinct 8 --out /dev/null
    python profiles/cue_retime_profile.py --fold-stats DIR/.../cue_retime_kernel_stats.csv [--out ...]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_retime_profile", "k_retime_dp", "k_cue_report")


def fold_stats(stats_csv: str, out: str) -> None:
    """{kernel: calls, average us, total us} of the three kernels of a rocprofv3 stats CSV into the JSON.  The traced run
    makes, per problem count, a warm and one timed call of each entry point: the averages are over both counts."""
    table = {}
    for r in csv.DictReader(open(stats_csv)):
        short = r["Name"].split("ffsa::", 1)[-1].split("(", 1)[0]
        if short in KERNELS:
            table[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                            "total_us": float(r["TotalDurationNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                            "max_us": float(r["MaxNs"]) / 1e3}
    result = json.load(open(out))
    result["kernels_traced_run"] = {"source": "rocprofv3 --kernel-trace --stats of --repeats 1 --distinct 8 (per problem count a "
                                              "warm and a timed call of each entry point; both counts and every sub-batch "
                                              "pooled: min_us is the one-problem call, max_us the largest sub-batch)", "table": table}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def _best(fn, repeats):
    import torch

    fn()  # warm: plan, workspace, code objects
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return min(times), times


def _prepare(seed):
    """(problem, cue table) of one seed behind the true sync: seeded host work."""
    from ffsubsync_amd import cue_report as cr
    from workloads import cue_stretches as ws

    p = ws.make_stretch_problem(seed)
    return p, cr.cue_table(p.start_us, p.end_us, p.ratio, ws.true_sync(p).cue_start_us)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cue_retime_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--fold-stats", default=None)
    args = ap.parse_args()
    if args.fold_stats:
        fold_stats(args.fold_stats, args.out)
        return
    from multiprocessing import Pool

    with Pool(min(8, args.distinct)) as pool:  # before the GPU is opened
        prepared = pool.map(_prepare, range(args.distinct))
    import torch

    from ffsubsync_amd import _native, batch, cue_report as cr, cue_retime as ct
    from ffsubsync_amd.subtitle_raster import DeviceRaster, rasterize_candidates

    rasters, tables = [], []
    for p, table in prepared:
        sub = rasterize_candidates(p.start_us, p.end_us, p.meta, [p.ratio])[0]
        assert sub.n >= int(table[1].max())
        rasters.append((DeviceRaster.from_host(p.ref.astype(float), lists=False), [sub]))
        tables.append(table)
    radius, context, pq, jq = ct.DEFAULT_RADIUS, ct.DEFAULT_CONTEXT, ct.DEFAULT_PENALTY_Q, ct.DEFAULT_JUMP_Q
    n_delta = 2 * radius + 1
    result = {"radius": radius, "context": context, "penalty_q": pq, "jump_q": jq, "shifts": n_delta,
              "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 256):
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        cues = [tables[i % len(tables)] for i in range(n_pairs)]
        table, first, count = cr.flat_cue_table(cues, n_pairs)
        dev = db.data.device
        cue_dev = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        rec = torch.empty(table.size * _native.CUE_RETIME_BYTES, dtype=torch.uint8, device=dev)
        summ = torch.empty(n_pairs * _native.RETIME_SUMMARY_BYTES, dtype=torch.uint8, device=dev)
        rep = torch.empty(table.size * _native.CUE_REPORT_BYTES, dtype=torch.uint8, device=dev)
        plan = cr._get_plan(n_pairs)
        retime = lambda: plan.cue_retime(*db.pair_arrays(), cue_dev, first, count, radius, context, pq, jq,
                                         _native.RETIME_KEEP_ORDER, rec, summ)
        report = lambda: plan.cue_report(*db.pair_arrays(), cue_dev, first, count, radius, context, rep)
        ms_retime, t_retime = _best(retime, args.repeats)
        ms_report, t_report = _best(report, args.repeats)
        src = torch.empty(table.size * n_delta, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        ms_copy, _ = _best(lambda: dst.copy_(src), args.repeats)
        sums = summ.cpu().numpy().view(_native.RETIME_SUMMARY_DTYPE)
        words = sum(int(((min(e + context, s) + 31) // 32 - max(a - context, 0) // 32) * n_delta)
                    for c, s in zip(cues, db.lens[:, 1]) for a, e in zip(c[0], c[1]) if e > a)
        result["calls"][str(n_pairs)] = {
            "cues": int(table.size), "live_cues": int(sums["n_live"].sum()), "moved": int(sums["n_moved"].sum()),
            "jumps": int(sums["n_jumps"].sum()), "word_lag_steps": words, "pairs_in_flight": plan.pairs_in_flight,
            "workspace_bytes": ct.workspace_bytes(count, radius, plan.pairs_in_flight),
            "retime_call": {"ms_per_call": ms_retime, "us_per_cue": 1000.0 * ms_retime / max(table.size, 1), "times_ms": t_retime},
            "cue_report_call": {"ms_per_call": ms_report, "word_lag_steps_per_s": words / (ms_report * 1e-3),
                                "times_ms": t_report},
            "profile_store_bytes": int(table.size) * n_delta * 4,
            "copy_of_profile_bytes": {"ms": ms_copy, "bytes_per_s_read_plus_write": 2 * table.size * n_delta * 4 / (ms_copy * 1e-3)},
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
    cr.clear_plan_cache()
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
