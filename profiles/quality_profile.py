"""Timing of the alignment quality report (ffsubsync_amd.quality, csrc/ffs_quality.h) at the defaults: 2 h pairs of the
headline workload (workloads/synth.make_pair_spec, the true-ratio candidate), +-60 s window (W = 6000), top_k 3, E = 300.
One call of 1 pair and one of 1024 pairs (32 distinct pairs, tiled), each timed with HIP events around the native call
(warm: one untimed call first), best of three.  Run it once under ``rocprofv3 --kernel-trace --stats`` for the split
between k_split_prefix / k_quality_counts / k_quality_peaks.

    python profiles/quality_profile.py [--out profiles/quality_profile.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_profile.json"))
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch

    from ffsubsync_amd import _native, quality
    from ffsubsync_amd.batch import DeviceBatch
    from workloads import synth

    w, top_k, e = 6000, quality.DEFAULT_TOP_K, quality.DEFAULT_EXCLUSION_SAMPLES
    specs = [synth.make_pair_spec(seed) for seed in range(args.distinct)]
    full = synth.build_device_batch(specs)
    db = full.select_candidates([sp.true_ratio_index for sp in specs])
    result = {"window_samples": w, "top_k": top_k, "exclusion_samples": e,
              "device": torch.cuda.get_device_name(0), "calls": {}}
    for n_pairs in (1, 1024):
        rows = np.arange(n_pairs) % db.n_pairs
        tb = DeviceBatch(db.data, db.offs[rows], db.lens[rows], db.lo[rows], db.hi[rows], db.dtype)
        quality.quality_batch(tb, w, top_k, e)  # warm: plan, code objects
        plan = next(iter(quality._plans.plans.values()))
        out = torch.empty(n_pairs * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device=tb.data.device)
        times = []
        for _ in range(args.repeats):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            plan.report(*tb.pair_arrays(), w, top_k, e, out)
            stop.record()
            torch.cuda.synchronize()
            times.append(start.elapsed_time(stop))
        recs = out.cpu().numpy().view(_native.QUALITY_RESULT_DTYPE)
        qs = [quality.from_record(r) for r in recs]
        words = int(((tb.lens[:, 1] + 31) // 32).sum())
        ms = min(times)
        result["calls"][str(n_pairs)] = {
            "ms_per_call": ms, "us_per_pair": 1e3 * ms / n_pairs, "times_ms": times,
            "word_lag_steps": words * 2 * w, "word_lag_steps_per_s_end_to_end": words * 2 * w / (ms * 1e-3),
            "pairs_in_flight": plan.pairs_in_flight, "workspace_bytes": plan.workspace_bytes,
            "trusted": sum(not quality.assess(q) for q in qs), "psr_min": min(q.psr for q in qs),
        }
        print(json.dumps({str(n_pairs): result["calls"][str(n_pairs)]}))
        quality.clear_plan_cache()
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
