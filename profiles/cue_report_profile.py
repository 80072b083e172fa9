"""Timing of the per-cue evidence report (ffsubsync_amd.cue_report, csrc/ffs_cue_report.h) at the defaults: 2 h problems
of workloads/cues.py behind the true sync (about 900 cues each), one call of 1 problem and one of 256 problems (32
distinct, tiled), each timed with HIP events (warm: one untimed call first), best of the repeats, for
  - the device call alone (SplitPlan.cue_report on buffers allocated up front: the kernel plus the descriptor upload),
  - the Python call cue_report_batch (table uploaded, records read back).
Run it once under ``rocprofv3 --kernel-trace --stats`` for k_cue_report on its own.

    python profiles/cue_report_profile.py [--out profiles/cue_report_profile.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cue_report_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import _native, batch, cue_report as cr
    from ffsubsync_amd.subtitle_raster import DeviceRaster, rasterize_candidates
    from workloads import cues as wc

    probs = [wc.make_cue_problem(seed) for seed in range(args.distinct)]
    rasters, tables = [], []
    for p in probs:
        res = wc.true_sync(p)
        sub = rasterize_candidates(p.start_us, p.end_us, p.meta, [p.ratio])[0]
        rasters.append((DeviceRaster.from_host(p.ref.astype(float), lists=False), [sub]))
        tables.append(cr.cue_table(p.start_us, p.end_us, p.ratio, res.cue_start_us, sub_len=sub.n))
    radius, context = cr.DEFAULT_RADIUS, cr.DEFAULT_CONTEXT
    result = {"radius_samples": radius, "context_samples": context, "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 256):
        db = batch.pack_pairs([rasters[i % len(rasters)] for i in range(n_pairs)])
        cues = [tables[i % len(tables)] for i in range(n_pairs)]
        ms_py, t_py, _ = _best(lambda: cr.cue_report_batch(db, cues, raw=True), args.repeats)
        table, first, count = cr.flat_cue_table(cues, n_pairs)
        dev = db.data.device
        cue_dev = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        rec = torch.empty(table.size * _native.CUE_REPORT_BYTES, dtype=torch.uint8, device=dev)
        plan = cr._get_plan(n_pairs)
        call = lambda: plan.cue_report(*db.pair_arrays(), cue_dev, first, count, radius, context, rec)
        ms_dev, t_dev, _ = _best(call, args.repeats)
        words = sum(int(((min(e + context, s) + 31) // 32 - max(a - context, 0) // 32) * (2 * radius + 1))
                    for c, s in zip(cues, db.lens[:, 1]) for a, e in zip(c[0], c[1]) if e > a)
        result["calls"][str(n_pairs)] = {
            "device_call": {"ms_per_call": ms_dev, "us_per_cue": 1000.0 * ms_dev / max(table.size, 1),
                            "word_lag_steps_per_s": words / (ms_dev * 1e-3), "times_ms": t_dev},
            "python_call": {"ms_per_call": ms_py, "times_ms": t_py},
            "cues": int(table.size), "word_lag_steps": words, "pairs_in_flight": plan.pairs_in_flight,
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
    cr.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
