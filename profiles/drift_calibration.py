"""Calibration of drift_align.DEFAULT_MAX_STEP / DEFAULT_STEP_COST on the CPU model (tests/drift_model.py) over the
SYNTHETIC problems of workloads/drift.py.  No GPU: the device equals the model bit for bit (tests/test_gpu_drift.py).

Two-hour problems, K = 1024, W = 6000 (+-60 s), P = 8192.  Three sets:
  clean   seeds 0..39, clean=True         -- the drift DP must return the split DP's block offsets exactly
  drift   seeds 0..23 as drawn            -- |eps| in [3e-4, 6e-4], half of them with a 0.5-1.5 s wobble
  wobble  seeds 100..107, eps = 0, 1.5 s  -- the steepest wobble the workload makes
Per (max_step, step_cost): clean pairs whose block offsets differ from the split DP's, and per drifting pair the mean
absolute block-offset error (samples) of the split DP and of the drift DP against the truth at the block centre.

Rule for the defaults: the smallest step_cost (powers of two) at which EVERY clean pair is identical to the split DP,
with max_step = 2 unless a wobble pair misses "at most half the split DP's error" at 2 and meets it with more.

    python profiles/drift_calibration.py            # writes profiles/drift_calibration.json (some 20 minutes on one core)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import drift_model as dm  # noqa: E402
import split_model as sm  # noqa: E402
from workloads import drift  # noqa: E402

K, W, P = 1024, 6000, 8192.0
DURATION_S = 7200.0
MAX_STEPS = (2, 3, 4)
STEP_COSTS = (32.0, 64.0, 128.0, 256.0)
SETS = (("clean", [dict(seed=s, clean=True) for s in range(40)]),
        ("drift", [dict(seed=s) for s in range(24)]),
        ("wobble", [dict(seed=s, eps=0.0, wobble_s=1.5) for s in range(100, 108)]))


def run(duration_s=DURATION_S, sets=SETS, max_steps=MAX_STEPS, step_costs=STEP_COSTS, log=None):
    rows = []
    for name, specs in sets:
        for kw in specs:
            pr = drift.make_problem(duration_s=duration_s, **kw)
            m = sm.block_scores(pr.ref, pr.sub, (0.0, 1.0), (0.0, pr.sub_hi), K, W)
            o, _ = sm.dp(m, P)
            split_off = o - (W - 1)
            row = dict(set=name, seed=pr.seed, ratio=pr.ratio, eps=pr.eps, wobble_s=pr.wobble_s,
                       split_error=drift.mean_block_error(pr, split_off, K), split_pieces=int((np.diff(split_off) != 0).sum()) + 1,
                       cells=[])
            for s in max_steps:
                for q in step_costs:
                    off, _, jump, _ = dm.solve(None, None, None, None, K, W, P, s, q, m=m)
                    row["cells"].append(dict(max_step=s, step_cost=q, error=drift.mean_block_error(pr, off, K),
                                             blocks_differ=int((off != split_off).sum()), jumps=int(jump.sum())))
            rows.append(row)
            if log:
                log("%s seed %d: split %.2f, drift(2, 128) %.2f" % (
                    name, pr.seed, row["split_error"],
                    [c["error"] for c in row["cells"] if (c["max_step"], c["step_cost"]) == (2, 128.0)][0]))
    return rows


def summarise(rows, max_steps=MAX_STEPS, step_costs=STEP_COSTS):
    out = []
    for s in max_steps:
        for q in step_costs:
            cell = lambda r: [c for c in r["cells"] if (c["max_step"], c["step_cost"]) == (s, q)][0]
            line = dict(max_step=s, step_cost=q)
            clean = [r for r in rows if r["set"] == "clean"]
            line["clean_pairs_differing"] = sum(cell(r)["blocks_differ"] > 0 for r in clean)
            for name in ("drift", "wobble"):
                rs = [r for r in rows if r["set"] == name]
                errs = [cell(r)["error"] for r in rs]
                ratio = [r["split_error"] / max(cell(r)["error"], 1e-9) for r in rs]
                line[name] = dict(mean_error=float(np.mean(errs)), worst_error=float(np.max(errs)),
                                  split_mean_error=float(np.mean([r["split_error"] for r in rs])),
                                  least_gain=float(np.min(ratio)), pairs_below_factor_2=int(sum(x < 2.0 for x in ratio)))
            out.append(line)
    return out


def choose(summary):
    ok = sorted(l["step_cost"] for l in summary if l["max_step"] == 2 and l["clean_pairs_differing"] == 0)
    # "every clean pair identical" must also hold at every larger tested cost, or the threshold means nothing
    cost = next(q for q in ok if all(x in ok for x in STEP_COSTS if x >= q))
    step = 2
    at = {l["max_step"]: l for l in summary if l["step_cost"] == cost}
    if at[2]["wobble"]["pairs_below_factor_2"] or at[2]["drift"]["pairs_below_factor_2"]:
        for s in sorted(at):
            if not at[s]["wobble"]["pairs_below_factor_2"] and not at[s]["drift"]["pairs_below_factor_2"] \
                    and not at[s]["clean_pairs_differing"]:
                step = s
                break
    return step, cost


def main():
    rows = run(log=lambda s: print(s, flush=True))
    summary = summarise(rows)
    step, cost = choose(summary)
    doc = dict(note="SYNTHETIC data (workloads/drift.py), CPU model (tests/drift_model.py); errors in samples of 10 ms",
               block_samples=K, max_offset_samples=W, split_penalty=P, duration_s=DURATION_S,
               chosen=dict(max_step=step, step_cost=cost), summary=summary, pairs=rows)
    path = os.path.join(ROOT, "profiles", "drift_calibration.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for l in summary:
        print("max_step %d step_cost %5.0f: clean differing %2d | drift mean %.2f worst %.2f least gain %.2f | wobble mean "
              "%.2f worst %.2f least gain %.2f" % (l["max_step"], l["step_cost"], l["clean_pairs_differing"],
                                                   l["drift"]["mean_error"], l["drift"]["worst_error"], l["drift"]["least_gain"],
                                                   l["wobble"]["mean_error"], l["wobble"]["worst_error"], l["wobble"]["least_gain"]))
    print("chosen: max_step = %d, step_cost = %g" % (step, cost))


if __name__ == "__main__":
    main()
