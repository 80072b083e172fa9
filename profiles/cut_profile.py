"""Profile of the lag-range split (csrc/ffs_split_range.h): wall time of ffs_align_split_range_batch calls
on synthetic pairs, against the old single-workgroup k_split_dp at the widest window it allows.

    python profiles/cut_profile.py [out.json]

Cases: one 2 h pair over its full overlap range, a 3 h subtitle against a 3 h 48 min video (full range), 64 2 h pairs
(full range), and ffs_align_split_batch at W = 131 072 (2W = 262 144 lags) for one and 64 2 h pairs.  Each case: one
warm-up call, then the median of `REPS` timed calls (torch.cuda.synchronize around each)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5


def _pairs(specs_and_extra):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import synth

    pairs = []
    for spec, extra_s in specs_and_extra:
        ref, cands = synth.pair_arrays(spec)
        if extra_s:  # a longer video: filler activity appended (the subtitle meets the start of it)
            rng = np.random.RandomState(spec.seed + 5)
            n = int(extra_s * 100)
            fill = np.repeat(rng.rand(n // 300 + 1) < 0.4, 300)[:n].astype(np.uint8)
            ref = np.concatenate([ref, fill])
        sub = cands[spec.true_ratio_index].astype(float) * spec.cand_amp[spec.true_ratio_index]
        pairs.append((DeviceRaster.from_host(ref.astype(float), lists=False), [DeviceRaster.from_host(sub, lists=False)]))
    return batch.pack_pairs(pairs)


def _time(fn):
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, [round(t * 1e3, 3) for t in ts]


def main(out_path=None):
    import torch

    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import split_align as sa
    from workloads import synth

    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "cases": {}}
    one = _pairs([(synth.make_pair_spec(0), 0)])
    big = _pairs([(synth.make_pair_spec(3, duration_s=10800.0), 48 * 60)])
    many = _pairs([(synth.make_pair_spec(s), 0) for s in range(64)])
    for name, db, fn in (
            ("range_full_2h_1pair", one, lambda db: ca.split_align_range_batch(db, None)),
            ("range_full_3h_vs_3h48_1pair", big, lambda db: ca.split_align_range_batch(db, None)),
            ("range_full_2h_64pairs", many, lambda db: ca.split_align_range_batch(db, None)),
            ("old_split_dp_W131072_2h_1pair", one, lambda db: sa.split_align_batch(db, 131072)),
            ("old_split_dp_W131072_2h_64pairs", many, lambda db: sa.split_align_batch(db, 131072)),
            ("range_W131072_2h_1pair", one, lambda db: ca.split_align_range_batch(db, (-131071, 131072), split_penalty=sa.DEFAULT_SPLIT_PENALTY)),
            ("range_W131072_2h_64pairs", many, lambda db: ca.split_align_range_batch(db, (-131071, 131072), split_penalty=sa.DEFAULT_SPLIT_PENALTY))):
        lens = db.lens
        k = 1024
        cells = int(sum(-(-int(l[1]) // k) * (int(l[0]) + int(l[1]) - 1) for l in lens)) if "range_full" in name else \
            int(sum(-(-int(l[1]) // k) * 262144 for l in lens))
        ms, all_ms = _time(lambda: fn(db))
        res["cases"][name] = {"pairs": int(db.n_pairs), "ms": round(ms, 3), "runs_ms": all_ms, "cells": cells,
                              "cells_per_s": cells / (ms * 1e-3)}
        print(name, res["cases"][name], flush=True)
        ca.clear_plan_cache()
        sa.clear_plan_cache()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
