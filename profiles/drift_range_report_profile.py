"""Profile of the segment path report over a lag range (csrc/ffs_drift_range_report.h) against its two
yardsticks: the range drift solve alone on the same inputs and pairs in flight (the added time is the figure), and the
added time of the piece report over a range (3.9: split_range_report_batch over split_align_range_batch) on the same
problems, which does the same S/32 x L counting without the scoring pass.

    timeout -k 10 900 python profiles/drift_range_report_profile.py [out.json]     # the timing table
    rocprofv3 --kernel-trace --stats -- python profiles/drift_range_report_profile.py --once    # the kernel table (no counters)

Rows: two-hour problems of workloads/cut_drift.py (SYNTHETIC: a drifting pair whose reference gained 22.5-30 min of
scenes, so the paths step and jump) over each pair's full overlap range, K = 1024, P = 8192, max_step 2, step_cost 64,
top_k 3, E = 300; at 1 pair and at 64 pairs, 16 in flight for every variant.  3.14's protocol: one process; per row one
warm round over the variants (the widest plan first), then 5 rounds that run the variants in turn, every call between
two HIP events; the median of the 5."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
IN_FLIGHT = 16
DURATION_S = 7200.0


def _pairs(seeds):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import cut_drift

    pairs = []
    for seed in seeds:
        p = cut_drift.make_problem(seed, duration_s=DURATION_S)
        pairs.append((DeviceRaster.from_host(p.ref.astype(float), lists=False),
                      [DeviceRaster.from_host(p.sub.astype(float) * p.sub_hi, lists=False)]))
    return batch.pack_pairs(pairs)


def _variants(db):
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import cut_report as cr
    from ffsubsync_amd import drift_range as dg
    from ffsubsync_amd import drift_range_report as drr

    pif = min(int(db.n_pairs), IN_FLIGHT)
    return [("range_split", lambda: ca.split_align_range_batch(db, None, pairs_in_flight=pif)),
            ("range_split_report", lambda: cr.split_range_report_batch(db, None, pairs_in_flight=pif, raw=True)),
            ("range_drift", lambda: dg.drift_align_range_batch(db, None, pairs_in_flight=pif)),
            ("range_drift_report", lambda: drr.drift_range_report_batch(db, None, pairs_in_flight=pif, raw=True))]


def _clear():
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import cut_report as cr
    from ffsubsync_amd import drift_range as dg
    from ffsubsync_amd import drift_range_report as drr

    for m in (ca, cr, dg, drr):
        m.clear_plan_cache()


def main(argv):
    import torch

    torch.cuda.set_device(0)
    once = "--once" in argv
    out_path = next((a for a in argv if not a.startswith("--")), None)
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "pairs_in_flight": IN_FLIGHT, "duration_s": DURATION_S,
           "note": "SYNTHETIC data (workloads/cut_drift.py)", "rows": {}}
    for n in (1, 64):
        if once and n != 1:
            continue
        db = _pairs(range(n))
        variants = _variants(db)
        outs = {name: fn() for name, fn in reversed(variants)}
        torch.cuda.synchronize()
        if once:
            continue
        times = {name: [] for name, _ in variants}
        for _ in range(REPS):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        row = {name: {"ms": round(float(np.median(t)), 3), "runs_ms": [round(x, 3) for x in t]} for name, t in times.items()}
        seg = outs["range_drift_report"][2]
        pieces = outs["range_split_report"][2]
        paths = outs["range_drift_report"][0]
        row["segments_per_pair"] = [int(seg.min()), int(seg.max())]
        row["pieces_per_pair"] = [int(pieces.min()), int(pieces.max())]
        row["steps_per_pair"] = [int(min(np.count_nonzero(np.diff(r.block_offsets)) for r in paths)),
                                 int(max(np.count_nonzero(np.diff(r.block_offsets)) for r in paths))]
        added = row["range_drift_report"]["ms"] - row["range_drift"]["ms"]
        added_split = row["range_split_report"]["ms"] - row["range_split"]["ms"]
        row["added_ms"] = round(added, 3)
        row["added_over_range_drift"] = round(added / row["range_drift"]["ms"], 3)
        row["split_report_added_ms"] = round(added_split, 3)
        row["added_over_split_report_added"] = round(added / added_split, 3)
        res["rows"]["full_%dpairs" % n] = row
        print("full_%dpairs" % n, json.dumps(row), flush=True)
        _clear()
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
