"""Calibration of drift_range_smooth.DEFAULT_RANGE_KNOT_BLOCKS / _RADIUS / _BEND_COST on the CPU model
(tests/drift_range_smooth_model.py) over the SYNTHETIC problems of workloads/cut_drift.py.  No GPU: the device equals
the model bit for bit (tests/test_gpu_drift_range_smooth.py), so these figures are the device's.

One-hour problems with 22.5-30 min of inserted scenes, K = 1024, each pair's full overlap range, the drift solve at
DESIGN 3.14's defaults (P = 8192, max_step 2, step_cost 64); the three sets of profiles/drift_range_calibration.py:
  clean   seeds 0..15, clean=True              -- the fit must leave every block on the drift path
  drift   seeds 0..15 as drawn                 -- |eps| in [3e-4, 6e-4], half of them with a 0.5-1.5 s wobble
  steep   cut_drift.steep_seeds(8), fixed=True -- eps = +-6e-4, no wobble
Every problem's drift path is solved ONCE (and kept in ``--cache DIR`` when given); only the fit is swept, the line
tables built once per (problem, knot_blocks, radius).  Errors are ``cut_drift.mean_block_error`` (samples, blocks more
than 2 from a true break) of the path and of the fitted integer offsets.

Rule for the defaults, DESIGN 3.12's unchanged: per (knot_blocks, radius) the smallest power-of-two bend cost at which
EVERY clean problem has smooth_offset == block_offset on every block, and does so at every larger cost tried; then the
(knot_blocks, radius) with the lowest mean fitted-offset error on the drifting set at its own threshold, the smaller
radius when two radii are within 1 % of each other.  Where no (knot_blocks, radius) has such a bend cost nothing is
chosen: the JSON says so, and its per-problem rows show drift_smooth's defaults, uncalibrated here.

``sync_check``: what tests/test_gpu_drift_range_smooth.py holds smooth_cut_sync to -- two steep seeds solved over ONE lag
range (the smallest holding every true block offset of both plus 4096 samples on each side, rounded out to multiples of
2048) at the chosen defaults: the path's and the fitted offsets' error per seed.  Steep seeds are taken in order; one on
which the fit does not gain is passed over, and listed.

    python profiles/drift_range_smooth_calibration.py [processes] [--cache DIR]
    # writes profiles/drift_range_smooth_calibration.json
"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cut_model as cm  # noqa: E402
import drift_range_model as drg  # noqa: E402
import drift_range_smooth_model as drsm  # noqa: E402
from workloads import cut_drift  # noqa: E402

K, P = 1024, 8192.0
MAX_STEP, STEP_COST = 2, 64.0
DURATION_S = cut_drift.DEFAULT_DURATION_S
KNOT_BLOCKS = (8, 16, 32, 64)
RADII = (8, 16)
BEND_COSTS = (16.0, 32.0, 64.0, 128.0, 256.0, 512.0)
NEAR_TIE = 0.01
SYNC_MARGIN, SYNC_ROUND, SYNC_SEEDS = 4096, 2048, 2
SHIPPED = (16, 16, 64.0)  # drift_smooth's defaults: what the per-problem rows show where the rule chooses nothing
SETS = (("clean", [dict(seed=s, clean=True) for s in range(16)]),
        ("drift", [dict(seed=s) for s in range(16)]),
        ("steep", [dict(seed=s, fixed=True) for s in cut_drift.steep_seeds(8)]))
CACHE = None


def drift_path(pr, name, lag_range=None):
    """(block offsets, jump flags) of the model's drift solve over ``lag_range`` (None = the full overlap range)."""
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size) if lag_range is None else lag_range
    path = CACHE and os.path.join(CACHE, "%s_%d_%d_%d.npz" % (name, pr.seed, lo, hi))
    if path and os.path.exists(path):
        z = np.load(path)
        return z["off"], z["jump"]
    off, _, jump, _ = drg.solve(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, lo, hi, P, MAX_STEP, STEP_COST)
    if path:
        os.makedirs(CACHE, exist_ok=True)
        np.savez(path, off=off, jump=jump)
    return off, jump


def sync_range(probs):
    """The smallest lag range holding every true block offset of ``probs`` plus SYNC_MARGIN on each side, rounded out
    to multiples of SYNC_ROUND."""
    truth = np.concatenate([cut_drift.block_truth(p, (p.sub.size + K - 1) // K, K) for p in probs])
    lo = int(np.floor((np.floor(truth.min()) - SYNC_MARGIN) / SYNC_ROUND)) * SYNC_ROUND
    hi = int(np.ceil((np.ceil(truth.max()) + SYNC_MARGIN) / SYNC_ROUND)) * SYNC_ROUND
    return lo, hi


def one_problem(job):
    name, kw = job
    pr = cut_drift.make_problem(duration_s=DURATION_S, **kw)
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size)
    off, jump = drift_path(pr, name)
    cnt = drsm.RangeCounts(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, lo, hi)
    row = dict(set=name, seed=pr.seed, ratio=pr.ratio, eps=pr.eps, wobble_s=pr.pair.wobble_s,
               path_error=cut_drift.mean_block_error(pr, off, K), segments=int(jump.sum()) + 1, cells=[])
    truth = cut_drift.block_truth(pr, off.size, K)
    for mk in KNOT_BLOCKS:
        for r in RADII:
            cache = {}
            for lam in BEND_COSTS:
                smooth, _, recs = drsm.fit(cnt, off, jump, mk, r, lam, cache)
                row["cells"].append(dict(knot_blocks=mk, radius=r, bend_cost=lam,
                                         error=cut_drift.mean_block_error(pr, smooth, K),
                                         blocks_differ=int((smooth != off).sum()),
                                         bend_total=float(recs["bend_total"].sum())))
    row["max_true_offset"] = float(np.abs(truth).max())
    return row


def sync_one(job):
    seed, lo, hi, mk, r, lam = job
    pr = cut_drift.make_problem(seed, duration_s=DURATION_S, fixed=True)
    off, jump = drift_path(pr, "sync", (lo, hi))
    cnt = drsm.RangeCounts(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, lo, hi)
    smooth, _, _ = drsm.fit(cnt, off, jump, mk, r, lam)
    return dict(seed=seed, path_error=cut_drift.mean_block_error(pr, off, K, exclude=2),
                smooth_error=cut_drift.mean_block_error(pr, smooth, K, exclude=2))


def sync_check(pool, mk, r, lam):
    """Two steep seeds, in order, on which the fit gains over one shared range; the seeds passed over are listed."""
    pool_seeds = cut_drift.steep_seeds(8)
    chosen, passed = pool_seeds[:SYNC_SEEDS], []
    rest = pool_seeds[SYNC_SEEDS:]
    while True:
        probs = [cut_drift.make_problem(s, duration_s=DURATION_S, fixed=True) for s in chosen]
        lo, hi = sync_range(probs)
        rows = pool.map(sync_one, [(s, lo, hi, mk, r, lam) for s in chosen])
        bad = [row["seed"] for row in rows if not row["smooth_error"] < row["path_error"]]
        if not bad or not rest:
            return dict(seeds=chosen, passed_over=passed, lag_range=[lo, hi], knot_blocks=mk, radius=r, bend_cost=lam,
                        every_seed_gains=not bad, by_seed={str(row["seed"]): row for row in rows})
        passed.append(bad[0])
        chosen = [s for s in chosen if s != bad[0]] + [rest.pop(0)]


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
                for name in ("drift", "steep"):
                    rs = [row for row in rows if row["set"] == name]
                    cells = [cell_of(row, mk, r, lam) for row in rs]
                    gain = [row["path_error"] / max(c["error"], 1e-9) for row, c in zip(rs, cells)]
                    line[name] = dict(mean_error=float(np.mean([c["error"] for c in cells])),
                                      path_mean_error=float(np.mean([row["path_error"] for row in rs])),
                                      least_gain=float(np.min(gain)), pairs_not_better=int(sum(g <= 1.0 for g in gain)))
                out.append(line)
    return out


def choose(summary):
    """(knot_blocks, radius, bend_cost) by the rule above, or None where no (knot_blocks, radius) has a bend cost that
    holds every clean problem."""
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
    if not at:
        return None
    best = min(at, key=lambda key: (at[key][1], key[1]))
    for r in sorted(RADII):  # the smaller radius on a near tie
        if r < best[1] and (best[0], r) in at and at[(best[0], r)][1] <= at[best][1] * (1.0 + NEAR_TIE):
            best = (best[0], r)
            break
    return best[0], best[1], at[best][0]


def compact(rows, mk, r, lam):
    """One short row per problem: what it is, and its figures in the chosen cell (the summary holds every cell)."""
    out = []
    for row in rows:
        c = cell_of(row, mk, r, lam)
        out.append(dict(set=row["set"], seed=row["seed"], ratio=round(row["ratio"], 6), eps=round(row["eps"], 7),
                        wobble_s=round(row["wobble_s"], 3), segments=row["segments"],
                        max_true_offset=round(row["max_true_offset"], 1), path_error=round(row["path_error"], 3),
                        error=round(c["error"], 3),
                        gain=round(row["path_error"] / c["error"], 3) if c["error"] > 0 else None,
                        blocks_differ=c["blocks_differ"]))
    return out


def dump(doc, path):
    """JSON with one line per summary cell and per problem."""
    head = {k: v for k, v in doc.items() if k not in ("summary", "pairs")}
    lines = [json.dumps(head, indent=1)[:-2] + ","]
    for key in ("summary", "pairs"):
        rows = [" " + json.dumps(x) for x in doc[key]]
        lines.append(' "%s": [\n' % key + ",\n".join(rows) + "\n ]" + ("," if key == "summary" else ""))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n}\n")


def main():
    global CACHE
    args = sys.argv[1:]
    if "--cache" in args:
        i = args.index("--cache")
        CACHE = args[i + 1]
        del args[i:i + 2]
    procs = int(args[0]) if args else 4
    work = [(name, kw) for name, specs in SETS for kw in specs]
    rows = []
    with multiprocessing.Pool(procs) as pool:
        for row in pool.imap(one_problem, work):
            rows.append(row)
            print("%s seed %d: path %.2f" % (row["set"], row["seed"], row["path_error"]), flush=True)
        summary = summarise(rows)
        chosen = choose(summary)
        check = sync_check(pool, *chosen) if chosen else None
    for l in summary:
        for name in ("drift", "steep"):
            l[name] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in l[name].items()}
        print("M %3d R %2d bend %4.0f: clean differing %2d | drift mean %.2f (path %.2f) least gain %.2f | steep mean %.2f "
              "(path %.2f) least gain %.2f"
              % (l["knot_blocks"], l["radius"], l["bend_cost"], l["clean_pairs_differing"], l["drift"]["mean_error"],
                 l["drift"]["path_mean_error"], l["drift"]["least_gain"], l["steep"]["mean_error"],
                 l["steep"]["path_mean_error"], l["steep"]["least_gain"]))
    note = ("SYNTHETIC data (workloads/cut_drift.py), CPU model (tests/drift_range_smooth_model.py); errors in samples of "
            "10 ms over the blocks more than 2 blocks from a true break; pairs: each problem's figures in the ")
    doc = dict(block_samples=K, split_penalty=P, max_step=MAX_STEP, step_cost=STEP_COST, duration_s=DURATION_S,
               lag_range="full overlap range")
    if chosen is None:
        mk, r, lam = SHIPPED
        differing = [dict(seed=row["seed"], blocks_differ=cell_of(row, mk, r, lam)["blocks_differ"])
                     for row in rows if row["set"] == "clean" and cell_of(row, mk, r, lam)["blocks_differ"]]
        doc.update(note=note + "SHIPPED cell, which is drift_smooth's and UNCALIBRATED here: no (knot_blocks, radius) has "
                   "a bend cost at which every clean problem stays on its path", chosen=None,
                   shipped_uncalibrated=dict(knot_blocks=mk, radius=r, bend_cost=lam), clean_problems_differing=differing,
                   sync_check=None)
        print("no (knot_blocks, radius) holds every clean problem at any bend cost tried: nothing chosen; per-problem "
              "figures at drift_smooth's defaults %r, clean problems off their path there: %r" % (SHIPPED, differing))
    else:
        mk, r, lam = chosen
        doc.update(note=note + "chosen cell; sync_check: the unrounded fp64 errors the GPU test compares with ==",
                   chosen=dict(knot_blocks=mk, radius=r, bend_cost=lam), sync_check=check)
        print("chosen: knot_blocks = %d, radius = %d, bend_cost = %g" % (mk, r, lam))
        print("sync check:", json.dumps(check))
    doc.update(summary=summary, pairs=compact(rows, mk, r, lam))
    dump(doc, os.path.join(ROOT, "profiles", "drift_range_smooth_calibration.json"))

if __name__ == "__main__":
    main()
