"""Stop-rule defaults of the progressive alignment, by rule.  CPU model only (tests/progressive_model.py),
synthetic data only (workloads/synth.make_pair_spec): no device is involved.

Data: per duration, N matched seeds (reference and candidates of the same seed; N a multiple of 7 is not needed -- the
seeds' true ratios are asserted to cover all seven) and as many wrong pairs (reference of seed a, candidates of seed
a + 1).  Chunks of 10 000 samples, W = 6000, E = 300.  Every file is run to its end once; every (stable_updates k,
min_ratio_margin m) cell is then decided on the stored states.

  wrong stop   a matched file that settles on another candidate than its full solve, or more than offset_tolerance from
               its offset; a wrong pair that settles at all
  consumed     L at the stop / the reference length (1 when the file never settles), mean over the matched files

Among the cells with zero wrong stops take the smallest mean consumed fraction; ship k + 1 and the next larger m of the
grid.  No such cell: ship stable_updates = None (the default rule never settles).

    python profiles/progressive_calibration.py [--seeds 40] [--durations 600 3600] > profiles/progressive_calibration.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import progressive_model as pm  # noqa: E402
from workloads import synth  # noqa: E402

CHUNK, W, E, TOP_K = 10000, 6000, 300, 3
MIN_PSR, MIN_MARGIN, OFFSET_TOLERANCE = 5.0, 3.0, 2  # quality.DEFAULT_MIN_PSR / _MIN_MARGIN, check_recovery's offset_tol
K_GRID = (2, 3, 4, 6)
M_GRID = (0.0, 0.05, 0.1, 0.2, 0.4, 0.8)


def history_of(ref_spec, cand_spec):
    ref = synth.rasterize(ref_spec.ref_len, ref_spec.ref_starts, ref_spec.ref_ends)
    cands = [(synth.rasterize(n, s, e), (0.0, a)) for n, s, e, a in
             zip(cand_spec.cand_len, cand_spec.cand_starts, cand_spec.cand_ends, cand_spec.cand_amp)]
    never = dict(min_psr=0, min_margin=0, min_ratio_margin=0, stable_updates=None, offset_tolerance=0, min_samples=0)
    return pm.run(ref, cands, (0.0, 1.0), W, CHUNK, never, TOP_K, E)["history"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--durations", type=float, nargs="+", default=[600.0, 3600.0])
    a = ap.parse_args()
    files = []
    for dur in a.durations:
        specs = [synth.make_pair_spec(seed, duration_s=dur) for seed in range(a.seeds + 1)]
        assert {sp.true_ratio_index for sp in specs[:a.seeds]} == set(range(7)), "the seeds must cover all seven ratios"
        for i in range(a.seeds):
            for kind, cand in (("matched", specs[i]), ("wrong", specs[i + 1])):
                h = history_of(specs[i], cand)
                files.append(dict(duration=dur, seed=i, kind=kind, ref_len=specs[i].ref_len, history=h))
                print("%s %g s seed %d: %d updates" % (kind, dur, i, len(h)), file=sys.stderr)
    cells = []
    for k in K_GRID:
        for m in M_GRID:
            wrong, consumed, stops = 0, [], []
            for f in files:
                u = stop_update(f["history"], k, m)
                full = f["history"][-1]
                if f["kind"] == "wrong":
                    wrong += u is not None
                    continue
                if u is None:
                    consumed.append(1.0)
                    continue
                st = f["history"][u]
                consumed.append(st["ref_len"] / f["ref_len"])
                bad = st["best_cand"] != full["best_cand"] or abs(st["offset"] - full["offset"]) > OFFSET_TOLERANCE
                wrong += bad
                stops.append(u + 1)
            cells.append(dict(k=k, m=m, wrong_stops=int(wrong), mean_consumed=float(np.mean(consumed)),
                              matched_settled=len(stops), max_stop_update=max(stops) if stops else None))
    k_ship, m_ship = ship(cells)
    per_file = [dict(duration=f["duration"], seed=f["seed"], kind=f["kind"], updates=len(f["history"]),
                     final=[f["history"][-1]["best_cand"], f["history"][-1]["offset"]],
                     final_derived=[round(x, 4) for x in pm.derived(f["history"][-1])]) for f in files]
    json.dump(dict(model="tests/progressive_model.py (CPU, synthetic: workloads/synth.make_pair_spec)", seeds=a.seeds,
                   durations=a.durations, chunk=CHUNK, W=W, E=E, top_k=TOP_K, min_psr=MIN_PSR, min_margin=MIN_MARGIN,
                   offset_tolerance=OFFSET_TOLERANCE, k_grid=list(K_GRID), m_grid=list(M_GRID), cells=cells,
                   shipped=dict(stable_updates=k_ship, min_ratio_margin=m_ship), files=per_file), sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
