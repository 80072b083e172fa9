"""Calibration of drift_range.DEFAULT_RANGE_STEP_COST on the CPU model (tests/drift_range_model.py) over the SYNTHETIC
problems of workloads/cut_drift.py.  No GPU: the device equals the model bit for bit (tests/test_gpu_drift_range.py).

One-hour problems with 22.5-30 min of inserted scenes, K = 1024, each pair's full overlap range (about 880 k lags, 350
blocks), P = 8192 (cut_align's default), max_step = 2.  Three sets:
  clean   seeds 0..15, clean=True   -- the inserts without drift: the range drift DP must return the range split DP's
                                       block offsets exactly
  drift   seeds 0..15 as drawn      -- |eps| in [3e-4, 6e-4], half of them with a 0.5-1.5 s wobble
  steep   cut_drift.steep_seeds(8), fixed=True -- eps = +-6e-4, no wobble, the first 8 seeds whose nominal ratio stays
                                       the candidate nearest to ratio * (1 + eps): seeds 0 1 2 5 6 8 14 15 (the set
                                       tests/test_gpu_drift_range.py runs on the device; on the others the seven-ratio
                                       solve rightly returns the neighbouring candidate)
Every problem's score rows are streamed once and feed the range split DP (max_step = 0) and one drift DP per step cost.
Per step cost: the clean problems whose block offsets differ from the range split's; per drifting set the mean and worst
``cut_drift.mean_block_error`` (blocks more than 2 from a true break) and the least gain (split error / drift error).

Rule for the default (DESIGN 3.10's): the smallest power-of-two step cost at which EVERY clean problem returns the range
split's block offsets, and does so at every larger tested cost too.

    python profiles/drift_range_calibration.py [processes]    # writes profiles/drift_range_calibration.json
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
import drift_range_model as drm  # noqa: E402
from workloads import cut_drift  # noqa: E402

K, P, MAX_STEP = 1024, 8192.0, 2
DURATION_S = cut_drift.DEFAULT_DURATION_S
STEP_COSTS = (32.0, 64.0, 128.0, 256.0, 512.0)
SETS = (("clean", [dict(seed=s, clean=True) for s in range(16)]),
        ("drift", [dict(seed=s) for s in range(16)]),
        ("steep", [dict(seed=s, fixed=True) for s in cut_drift.steep_seeds(8)]))


def solve_costs(pr, step_costs=STEP_COSTS, max_step=MAX_STEP, block_samples=K, split_penalty=P, lag_range=None):
    """(range split block offsets, {step cost: (block offsets, jump flags)}) of one problem from one stream of rows."""
    lo, hi = cm.full_range(pr.ref.size, pr.sub.size) if lag_range is None else lag_range
    pair = cm._Pair(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), block_samples, lo, hi)
    split = drm.RowDP(split_penalty, 0, 0.0)
    dps = {q: drm.RowDP(split_penalty, max_step, q) for q in step_costs}
    for b in range(pair.n_blocks):
        row = pair.scores(b)
        split.push(row)
        for dp in dps.values():
            dp.push(row)
    out = {}
    for q, dp in dps.items():
        o, jump, _ = dp.finish()
        out[q] = (o + lo, jump)
    return split.finish()[0] + lo, out


def one(job):
    name, kw = job
    pr = cut_drift.make_problem(duration_s=DURATION_S, **kw)
    split_off, by_cost = solve_costs(pr)
    truth = cut_drift.block_truth(pr, split_off.size, K)
    row = dict(set=name, seed=pr.seed, ratio=pr.ratio, eps=pr.eps, wobble_s=pr.pair.wobble_s,
               inserted_s=float(pr.insert_len_s.sum()), n_inserts=int(pr.insert_len_s.size),
               max_true_offset=float(np.abs(truth).max()), split_error=cut_drift.mean_block_error(pr, split_off, K),
               split_pieces=int((np.diff(split_off) != 0).sum()) + 1, cells=[])
    for q, (off, jump) in by_cost.items():
        steps = int(((np.diff(off) != 0) & (jump[1:] == 0)).sum())
        row["cells"].append(dict(step_cost=q, error=cut_drift.mean_block_error(pr, off, K),
                                 blocks_differ=int((off != split_off).sum()), jumps=int(jump.sum()), steps=steps))
    return row


def summarise(rows, step_costs=STEP_COSTS):
    out = []
    for q in step_costs:
        cell = lambda r: [c for c in r["cells"] if c["step_cost"] == q][0]
        line = dict(max_step=MAX_STEP, step_cost=q)
        line["clean_problems_differing"] = sum(cell(r)["blocks_differ"] > 0 for r in rows if r["set"] == "clean")
        for name in ("drift", "steep"):
            rs = [r for r in rows if r["set"] == name]
            errs = [cell(r)["error"] for r in rs]
            gain = {r["seed"]: r["split_error"] / max(cell(r)["error"], 1e-9) for r in rs}
            line[name] = dict(mean_error=float(np.mean(errs)), worst_error=float(np.max(errs)),
                              split_mean_error=float(np.mean([r["split_error"] for r in rs])),
                              least_gain=float(min(gain.values())), gain_by_seed={str(s): g for s, g in gain.items()})
        out.append(line)
    return out


def choose(summary):
    ok = sorted(l["step_cost"] for l in summary if l["clean_problems_differing"] == 0)
    # "every clean problem identical" must also hold at every larger tested cost, or the threshold means nothing
    return next(q for q in ok if all(x in ok for x in STEP_COSTS if x >= q))


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    jobs = [(name, kw) for name, specs in SETS for kw in specs]
    rows = []
    with multiprocessing.Pool(procs) as pool:
        for row in pool.imap(one, jobs):
            rows.append(row)
            print("%s seed %d: split %.2f, drift(%g) %.2f" % (row["set"], row["seed"], row["split_error"], 128.0,
                                                             [c["error"] for c in row["cells"] if c["step_cost"] == 128.0][0]),
                  flush=True)
    summary = summarise(rows)
    cost = choose(summary)
    doc = dict(note="SYNTHETIC data (workloads/cut_drift.py), CPU model (tests/drift_range_model.py); errors in samples of "
                    "10 ms over the blocks more than 2 blocks from a true break",
               block_samples=K, split_penalty=P, duration_s=DURATION_S, lag_range="full overlap range",
               chosen=dict(max_step=MAX_STEP, step_cost=cost), summary=summary, problems=rows)
    with open(os.path.join(ROOT, "profiles", "drift_range_calibration.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for l in summary:
        print("step_cost %5.0f: clean differing %2d | drift mean %.2f worst %.2f least gain %.2f | steep mean %.2f worst "
              "%.2f least gain %.2f" % (l["step_cost"], l["clean_problems_differing"], l["drift"]["mean_error"],
                                        l["drift"]["worst_error"], l["drift"]["least_gain"], l["steep"]["mean_error"],
                                        l["steep"]["worst_error"], l["steep"]["least_gain"]))
    print("chosen: max_step = %d, step_cost = %g" % (MAX_STEP, cost))


if __name__ == "__main__":
    main()
