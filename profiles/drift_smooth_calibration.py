"""Calibration of drift_smooth.DEFAULT_KNOT_BLOCKS / DEFAULT_RADIUS / DEFAULT_BEND_COST on the CPU model
(tests/drift_smooth_model.py) over the SYNTHETIC problems of workloads/drift.py.  No GPU: the device equals the model bit
for bit (tests/test_gpu_drift_smooth.py), so these figures are the device's.

Two-hour problems, K = 1024, W = 6000 (+-60 s), P = 8192, the drift solve at its defaults (max_step 2, step_cost 128);
the three sets of profiles/drift_calibration.py:
  clean   seeds 0..39, clean=True         -- the fit must leave every block on the drift path
  drift   seeds 0..23 as drawn            -- |eps| in [3e-4, 6e-4], half of them with a 0.5-1.5 s wobble
  wobble  seeds 100..107, eps = 0, 1.5 s  -- the steepest wobble the workload makes
The block counts and the drift solve are built once per problem, the line tables once per (problem, knot_blocks, radius).
Per cell (knot_blocks, radius, bend_cost): clean pairs with a block off the path, and per drifting pair the mean
absolute block error (samples) of the path, of the fitted integer offsets, and of the polyline interpolated between knot
block centres as map_cues_smooth evaluates it (at the block centres).

Rule for the defaults: the bend cost is a price per sample of slope change per knot_blocks blocks, so its threshold is
taken per (knot_blocks, radius): the smallest power of two at which EVERY clean pair has smooth_offset == block_offset
on every block, and does so at every larger cost tried.  (DEFAULT_KNOT_BLOCKS, DEFAULT_RADIUS) = the pair with the
lowest mean fitted-offset error on the drifting set at its own threshold, the smaller radius when two radii are within
1 % of each other; DEFAULT_BEND_COST = that pair's threshold.

    python profiles/drift_smooth_calibration.py [jobs]   # writes profiles/drift_smooth_calibration.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import drift_model as dm  # noqa: E402
import drift_smooth_model as dsm  # noqa: E402
import split_model as sm  # noqa: E402
from workloads import drift  # noqa: E402

K, W, P = 1024, 6000, 8192.0
MAX_STEP, STEP_COST = 2, 128.0
DURATION_S = 7200.0
KNOT_BLOCKS = (8, 16, 32, 64)
RADII = (8, 16)
BEND_COSTS = (16.0, 32.0, 64.0, 128.0, 256.0, 512.0)
NEAR_TIE = 0.01
SETS = (("clean", [dict(seed=s, clean=True) for s in range(40)]),
        ("drift", [dict(seed=s) for s in range(24)]),
        ("wobble", [dict(seed=s, eps=0.0, wobble_s=1.5) for s in range(100, 108)]))


def polyline_error(pr, offsets, jump, smooth, knot):
    """Mean absolute error (samples) at the block centres of the polyline through the knots, evaluated as
    drift_smooth.polyline_shift does."""
    import drift_report_model as drm

    n = offsets.size
    centre = (np.arange(n) + 0.5) * K
    fitted = np.zeros(n)
    for f, e in drm.segments_of(jump):
        ks = [b for b in range(f, e) if knot[b]]
        if len(ks) == 1:
            fitted[f:e] = smooth[f]
            continue
        fitted[f:e] = np.interp(centre[f:e], centre[ks], smooth[ks].astype(np.float64))  # every block centre lies between knots
    truth = pr.true_offset(centre)  # (k + 1/2) K: the last block may be short, the polyline is defined on full blocks
    return float(np.mean(np.abs(fitted - truth)))


def one_problem(job):
    name, kw = job
    pr = drift.make_problem(duration_s=DURATION_S, **kw)
    cnt = dsm.Counts(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, W)
    m = sm.block_scores(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, W, n11=cnt.n11)
    off, _, jump, _ = dm.solve(None, None, None, None, K, W, P, MAX_STEP, STEP_COST, m=m)
    row = dict(set=name, seed=pr.seed, ratio=pr.ratio, eps=pr.eps, wobble_s=pr.wobble_s,
               path_error=drift.mean_block_error(pr, off, K), segments=int(jump.sum()) + 1, cells=[])
    for mk in KNOT_BLOCKS:
        for r in RADII:
            cache = {}
            for lam in BEND_COSTS:
                smooth, knot, recs = dsm.fit(cnt, off, jump, mk, r, lam, cache)
                row["cells"].append(dict(knot_blocks=mk, radius=r, bend_cost=lam,
                                         error=drift.mean_block_error(pr, smooth, K),
                                         polyline_error=polyline_error(pr, off, jump, smooth, knot),
                                         worst_error=float(np.max(np.abs(smooth - drift.block_truth(pr, off.size, K)))),
                                         blocks_differ=int((smooth != off).sum()),
                                         bend_total=float(recs["bend_total"].sum())))
    return row


def run(sets=SETS, jobs=1, log=None):
    work = [(name, kw) for name, specs in sets for kw in specs]
    if jobs > 1:
        import multiprocessing

        with multiprocessing.Pool(jobs) as pool:
            rows = pool.map(one_problem, work, chunksize=1)
    else:
        rows = []
        for w in work:
            rows.append(one_problem(w))
            if log:
                log("%s seed %d: path %.2f" % (rows[-1]["set"], rows[-1]["seed"], rows[-1]["path_error"]))
    return rows


def cell_of(row, mk, r, lam):
    return [c for c in row["cells"] if (c["knot_blocks"], c["radius"], c["bend_cost"]) == (mk, r, lam)][0]


def summarise(rows):
    out = []
    for mk in KNOT_BLOCKS:
        for r in RADII:
            for lam in BEND_COSTS:
                line = dict(knot_blocks=mk, radius=r, bend_cost=lam)
                clean = [row for row in rows if row["set"] == "clean"]
                line["clean_pairs_differing"] = sum(cell_of(row, mk, r, lam)["blocks_differ"] > 0 for row in clean)
                for name in ("drift", "wobble"):
                    rs = [row for row in rows if row["set"] == name]
                    cells = [cell_of(row, mk, r, lam) for row in rs]
                    gain = [row["path_error"] / max(c["error"], 1e-9) for row, c in zip(rs, cells)]
                    line[name] = dict(mean_error=float(np.mean([c["error"] for c in cells])),
                                      mean_polyline_error=float(np.mean([c["polyline_error"] for c in cells])),
                                      worst_block_error=float(np.max([c["worst_error"] for c in cells])),
                                      path_mean_error=float(np.mean([row["path_error"] for row in rs])),
                                      least_gain=float(np.min(gain)), pairs_not_better=int(sum(g <= 1.0 for g in gain)))
                out.append(line)
    return out


def choose(summary):
    def clean_ok(mk, r, lam):
        return all(l["clean_pairs_differing"] == 0 for l in summary
                   if (l["knot_blocks"], l["radius"]) == (mk, r) and l["bend_cost"] >= lam)

    at = {}  # (knot_blocks, radius) -> (its threshold cost, the drifting set's mean error there)
    for mk in KNOT_BLOCKS:
        for r in RADII:
            cost = next((lam for lam in BEND_COSTS if clean_ok(mk, r, lam)), None)
            if cost is not None:
                at[(mk, r)] = (cost, [l["drift"]["mean_error"] for l in summary
                                      if (l["knot_blocks"], l["radius"], l["bend_cost"]) == (mk, r, cost)][0])
    best = min(at, key=lambda key: (at[key][1], key[1]))
    for r in sorted(RADII):  # the smaller radius on a near tie
        if r < best[1] and (best[0], r) in at and at[(best[0], r)][1] <= at[best][1] * (1.0 + NEAR_TIE):
            best = (best[0], r)
            break
    return best[0], best[1], at[best][0]


def sync_gain(rows, mk, r, lam, seeds=range(12)):
    """Least path_error / polyline_error over the drifting seeds tests/test_gpu_drift.py syncs (block centres, not cues)."""
    rs = [row for row in rows if row["set"] == "drift" and row["seed"] in seeds]
    return float(min(row["path_error"] / max(cell_of(row, mk, r, lam)["polyline_error"], 1e-9) for row in rs))


def compact(rows, mk, r, lam):
    """One short row per pair: what it is, and its figures in the chosen cell (the summary holds every cell)."""
    out = []
    for row in rows:
        c = cell_of(row, mk, r, lam)
        out.append(dict(set=row["set"], seed=row["seed"], ratio=round(row["ratio"], 6), eps=round(row["eps"], 7),
                        wobble_s=round(row["wobble_s"], 3), segments=row["segments"], path_error=round(row["path_error"], 3),
                        error=round(c["error"], 3), polyline_error=round(c["polyline_error"], 3),
                        worst_error=round(c["worst_error"], 1), blocks_differ=c["blocks_differ"]))
    return out


def dump(doc, path):
    """JSON with one line per summary cell and per pair."""
    head = {k: v for k, v in doc.items() if k not in ("summary", "pairs")}
    lines = [json.dumps(head, indent=1)[:-2] + ","]
    for key in ("summary", "pairs"):
        rows = [" " + json.dumps(x) for x in doc[key]]
        lines.append(' "%s": [\n' % key + ",\n".join(rows) + "\n ]" + ("," if key == "summary" else ""))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n}\n")


def main():
    jobs = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    rows = run(jobs=jobs, log=lambda s: print(s, flush=True))
    summary = summarise(rows)
    mk, r, lam = choose(summary)
    for l in summary:
        for name in ("drift", "wobble"):
            l[name] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in l[name].items()}
    doc = dict(note="SYNTHETIC data (workloads/drift.py), CPU model (tests/drift_smooth_model.py); errors in samples of 10 ms; "
                    "pairs: each pair's figures in the chosen cell",
               block_samples=K, max_offset_samples=W, split_penalty=P, max_step=MAX_STEP, step_cost=STEP_COST,
               duration_s=DURATION_S, chosen=dict(knot_blocks=mk, radius=r, bend_cost=lam),
               least_polyline_gain_sync_seeds=round(sync_gain(rows, mk, r, lam), 3), summary=summary,
               pairs=compact(rows, mk, r, lam))
    dump(doc, os.path.join(ROOT, "profiles", "drift_smooth_calibration.json"))
    for l in summary:
        print("M %3d R %2d bend %4.0f: clean differing %2d | drift mean %.2f (polyline %.2f, path %.2f) least gain %.2f | "
              "wobble mean %.2f (polyline %.2f, path %.2f) least gain %.2f"
              % (l["knot_blocks"], l["radius"], l["bend_cost"], l["clean_pairs_differing"], l["drift"]["mean_error"],
                 l["drift"]["mean_polyline_error"], l["drift"]["path_mean_error"], l["drift"]["least_gain"],
                 l["wobble"]["mean_error"], l["wobble"]["mean_polyline_error"], l["wobble"]["path_mean_error"],
                 l["wobble"]["least_gain"]))
    print("chosen: knot_blocks = %d, radius = %d, bend_cost = %g" % (mk, r, lam))


if __name__ == "__main__":
    main()
