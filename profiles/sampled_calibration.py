"""Stop-rule defaults of the sampled alignment, by rule: the construction of
profiles/progressive_calibration.py on segments read in a spread order.  CPU model only (tests/sampled_model.py),
synthetic data only (workloads/synth.make_pair_spec): no device is involved.

Data: per duration, N matched seeds and as many wrong pairs (reference of seed a, candidates of seed a + 1).  Segments of
60 s (6000 samples) in sampled_model.segment_schedule order, W = 6000, E = 300.  Every file is run through its whole
schedule once; every (stable_updates k, min_ratio_margin m) cell is then decided on the stored states.  The same files
are run through the prefix schedule (the same segments, ascending) and its consumed fractions stand beside the spread
ones, as found.

  wrong stop   a matched file that settles on another candidate than its full solve, or more than offset_tolerance from
               its offset; a wrong pair that settles at all
  consumed     known samples at the stop / the reference length (1 when the file never settles), mean over matched files

Among the cells with zero wrong stops take the smallest mean consumed fraction; ship k + 1 and the next larger m of the
grid.  No such cell: ship stable_updates = None (the default rule never settles).

    python profiles/sampled_calibration.py [--seeds 40] [--durations 600 3600] [--jobs 8] > profiles/sampled_calibration.json
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import progressive_model as pm  # noqa: E402
import sampled_model as sm  # noqa: E402
from workloads import synth  # noqa: E402

SEGMENT, W, E, TOP_K = 6000, 6000, 300, 3
MIN_PSR, MIN_MARGIN, OFFSET_TOLERANCE = 5.0, 3.0, 2  # quality.DEFAULT_MIN_PSR / _MIN_MARGIN, check_recovery's offset_tol
K_GRID = (2, 3, 4, 6)
M_GRID = (0.0, 0.05, 0.1, 0.2, 0.4, 0.8)
NEVER = dict(min_psr=0, min_margin=0, min_ratio_margin=0, stable_updates=None, offset_tolerance=0, min_samples=0)


def histories_of(job):
    """(spread history, prefix history) of one file."""
    dur, seed, kind = job
    ref_spec = synth.make_pair_spec(seed, duration_s=dur)
    cand_spec = ref_spec if kind == "matched" else synth.make_pair_spec(seed + 1, duration_s=dur)
    ref = synth.rasterize(ref_spec.ref_len, ref_spec.ref_starts, ref_spec.ref_ends)
    cands = [(synth.rasterize(n, s, e), (0.0, a)) for n, s, e, a in
             zip(cand_spec.cand_len, cand_spec.cand_starts, cand_spec.cand_ends, cand_spec.cand_amp)]
    spread = sm.segment_schedule(ref.size, SEGMENT)
    out = []
    for schedule in (spread, sorted(spread)):
        out.append(sm.run(ref, cands, (0.0, 1.0), W, schedule, NEVER, TOP_K, E)["history"])
    print("%s %g s seed %d: %d updates" % (kind, dur, seed, len(out[0])), file=sys.stderr)
    return dict(duration=dur, seed=seed, kind=kind, ref_len=int(ref.size), history=out[0], prefix_history=out[1])


def stop_update(history, k, m):
    """Index of the update at which the rule settles, or None."""
    for u in range(1, len(history) + 1):
        if pm.settled(history[:u], MIN_PSR, MIN_MARGIN, m, k, OFFSET_TOLERANCE, 0):
            return u - 1
    return None


def ship(cells):
    """The shipped (stable_updates, min_ratio_margin) by the rules above, from the table's cells."""
    ok = [c for c in cells if c["wrong_stops"] == 0]
    if not ok:
        return None, 0.0
    best = min(ok, key=lambda c: (c["mean_consumed"], c["k"], c["m"]))
    larger = [m for m in M_GRID if m > best["m"]]
    return best["k"] + 1, (larger[0] if larger else best["m"])


def cell(files, key, k, m):
    wrong, consumed, stops = 0, [], []
    for f in files:
        h = f[key]
        u = stop_update(h, k, m)
        full = h[-1]
        if f["kind"] == "wrong":
            wrong += u is not None
            continue
        if u is None:
            consumed.append(1.0)
            continue
        st = h[u]
        consumed.append(st["ref_len"] / f["ref_len"])
        wrong += st["best_cand"] != full["best_cand"] or abs(st["offset"] - full["offset"]) > OFFSET_TOLERANCE
        stops.append(u + 1)
    return dict(wrong_stops=int(wrong), mean_consumed=float(np.mean(consumed)), matched_settled=len(stops),
                max_stop_update=max(stops) if stops else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--durations", type=float, nargs="+", default=[600.0, 3600.0])
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    jobs = []
    for dur in a.durations:
        specs = [synth.make_pair_spec(seed, duration_s=dur) for seed in range(a.seeds)]
        assert {sp.true_ratio_index for sp in specs} == set(range(7)), "the seeds must cover all seven ratios"
        jobs += [(dur, i, kind) for i in range(a.seeds) for kind in ("matched", "wrong")]
    with multiprocessing.Pool(a.jobs) as pool:
        files = pool.map(histories_of, jobs, chunksize=1)
    cells = []
    for k in K_GRID:
        for m in M_GRID:
            c = dict(k=k, m=m, **cell(files, "history", k, m))
            p = cell(files, "prefix_history", k, m)
            c["prefix_wrong_stops"], c["prefix_mean_consumed"] = p["wrong_stops"], p["mean_consumed"]
            cells.append(c)
    k_ship, m_ship = ship(cells)
    shipped = dict(stable_updates=k_ship, min_ratio_margin=m_ship)
    if k_ship is not None:  # the shipped rule itself on both schedules, as found
        shipped["spread"] = cell(files, "history", k_ship, m_ship)
        shipped["prefix"] = cell(files, "prefix_history", k_ship, m_ship)
    per_file = [dict(duration=f["duration"], seed=f["seed"], kind=f["kind"], updates=len(f["history"]),
                     final=[f["history"][-1]["best_cand"], f["history"][-1]["offset"]],
                     final_derived=[round(x, 4) for x in pm.derived(f["history"][-1])]) for f in files]
    json.dump(dict(model="tests/sampled_model.py (CPU, synthetic: workloads/synth.make_pair_spec)", seeds=a.seeds,
                   durations=a.durations, segment=SEGMENT, order="sampled_model.segment_schedule (bit-reversed)", W=W, E=E,
                   top_k=TOP_K, min_psr=MIN_PSR, min_margin=MIN_MARGIN, offset_tolerance=OFFSET_TOLERANCE,
                   k_grid=list(K_GRID), m_grid=list(M_GRID), cells=cells, shipped=shipped, files=per_file), sys.stdout,
              indent=1)
    print()


if __name__ == "__main__":
    main()
