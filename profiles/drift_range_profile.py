"""Profile of the lag-range drift solve (csrc/ffs_drift_range.h) against its two yardsticks: the range
split on the same inputs (ffs_align_split_range_batch) and the windowed drift solve (ffs_align_drift_batch) at
W = 131 072.

    python profiles/drift_range_profile.py [out.json]          # the timing table
    rocprofv3 --kernel-trace --stats -- python profiles/drift_range_profile.py --once     # the kernel table (no counters)

Rows: 2 h against 2 h over each pair's full overlap range, and [-131 071, 131 072]; each at 1 pair and at 64 pairs.
Variants per row: the range split, the range drift solve at max_step 0, 2 and 7, and on the second row the windowed
drift solve at max_step 2.  One process; per row one warm round over the variants, then 5 rounds that run the variants
in turn (so that clock or thermal changes meet every variant alike); every call between two HIP events; the median of
the 5.  Every variant of a row solves the same number of pairs in flight."""
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
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import split_align as sa

    rng = None if row == "full" else (-W + 1, W)
    pif = min(int(db.n_pairs), IN_FLIGHT)
    p = ca.DEFAULT_CUT_PENALTY
    out = [("range_split", lambda: ca.split_align_range_batch(db, rng, split_penalty=p, pairs_in_flight=pif))]
    for s in (0, 2, 7):
        out.append(("range_drift_s%d" % s,
                    lambda s=s: dr.drift_align_range_batch(db, rng, split_penalty=p, max_step=s, pairs_in_flight=pif)))
    if row != "full":
        out.append(("windowed_drift_s2", lambda: da.drift_align_batch(db, W, split_penalty=p, max_step=2,
                                                                      step_cost=dr.DEFAULT_RANGE_STEP_COST,
                                                                      pairs_in_flight=pif)))
        out.append(("windowed_split", lambda: sa.split_align_batch(db, W, split_penalty=p, pairs_in_flight=pif)))
    return out


def _clear():
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import split_align as sa

    for m in (ca, da, dr, sa):
        m.clear_plan_cache()


def main(argv):
    import torch

    torch.cuda.set_device(0)
    once = "--once" in argv
    out_path = next((a for a in argv if not a.startswith("--")), None)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "pairs_in_flight": IN_FLIGHT, "rows": {}}
    sets = {1: _pairs([0]), 64: _pairs(range(64))}
    for row in ("full", "W131072"):
        for n, db in sets.items():
            if once and n != 1:
                continue
            variants = _variants(row, db)
            # the widest plan first, so that the rounds below never rebuild one
            outs = {name: fn() for name, fn in reversed(variants)}
            torch.cuda.synchronize()
            if once:
                continue
            same = all(np.array_equal(a.block_offsets, b.block_offsets)
                       for a, b in zip(outs["range_split"], outs["range_drift_s0"]))
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
            res["rows"][key] = {name: {"ms": round(float(np.median(t)), 3), "runs_ms": [round(x, 3) for x in t]}
                                for name, t in times.items()}
            res["rows"][key]["s0_equals_range_split"] = bool(same)
            base = res["rows"][key]["range_split"]["ms"]
            for name in times:
                res["rows"][key][name]["vs_range_split"] = round(res["rows"][key][name]["ms"] / base, 3)
            print(key, json.dumps(res["rows"][key]), flush=True)
            _clear()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
