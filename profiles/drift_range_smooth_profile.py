"""Profile of the smooth fit behind the lag-range drift solve (csrc/ffs_drift_range_smooth.h) against its
yardstick: the range drift call on the same inputs in the same run (ffs_align_drift_range_batch).

    python profiles/drift_range_smooth_profile.py [out.json]      # the timing table
    rocprofv3 --kernel-trace --stats -- python profiles/drift_range_smooth_profile.py --once   # the kernel table (no counters)

Rows: 2 h against 2 h over each pair's full overlap range, and [-131 071, 131 072]; each at 1 pair and at 64 pairs; the
defaults of both calls.  One process; per row one warm round over the two variants, then 5 rounds that run them in turn
(so that clock or thermal changes meet both alike); every call between two HIP events; the median of the 5.  Both
variants solve the same number of pairs in flight."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
IN_FLIGHT = 16
W = 131072


def _pairs(seeds):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import synth

    pairs = []
    for seed in seeds:
        spec = synth.make_pair_spec(seed)
        ref, cands = synth.pair_arrays(spec)
        sub = cands[spec.true_ratio_index].astype(float) * spec.cand_amp[spec.true_ratio_index]
        pairs.append((DeviceRaster.from_host(ref.astype(float), lists=False), [DeviceRaster.from_host(sub, lists=False)]))
    return batch.pack_pairs(pairs)


def _variants(row, db):
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs

    rng = None if row == "full" else (-W + 1, W)
    pif = min(int(db.n_pairs), IN_FLIGHT)
    return [("range_drift", lambda: dr.drift_align_range_batch(db, rng, pairs_in_flight=pif)),
            ("range_smooth", lambda: drs.smooth_align_range_batch(db, rng, pairs_in_flight=pif, raw=True))]


def main(argv):
    import torch

    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs

    torch.cuda.set_device(0)
    once = "--once" in argv
    out_path = next((a for a in argv if not a.startswith("--")), None)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "pairs_in_flight": IN_FLIGHT, "rows": {}}
    sets = {1: _pairs([0])} if once else {1: _pairs([0]), 64: _pairs(range(64))}
    for row in ("full", "W131072"):
        for n, db in sets.items():
            variants = _variants(row, db)
            outs = {name: fn() for name, fn in variants}  # the warm round: both plans are made here
            torch.cuda.synchronize()
            if once:
                continue
            same = all(np.array_equal(a.block_offsets, b.block_offsets)
                       for a, b in zip(outs["range_drift"], outs["range_smooth"][0]))
            times = {name: [] for name, _ in variants}
            for _ in range(REPS):
                for name, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            key = "%s_%dpairs" % (row, n)
            cell = {name: {"ms": round(float(np.median(t)), 3), "runs_ms": [round(x, 3) for x in t]} for name, t in times.items()}
            cell["drift_outputs_equal"] = bool(same)
            cell["fit_adds"] = round(cell["range_smooth"]["ms"] / cell["range_drift"]["ms"] - 1.0, 4)
            res["rows"][key] = cell
            print(key, json.dumps(cell), flush=True)
            dr.clear_plan_cache()
            drs.clear_plan_cache()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
