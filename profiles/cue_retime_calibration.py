"""Calibration of the joint cue retiming's defaults (cue_retime.DEFAULT_RADIUS / DEFAULT_CONTEXT / DEFAULT_PENALTY_Q /
DEFAULT_JUMP_Q) on the CPU model tests/retime_model.py and the seeded workload workloads/cue_stretches.py.  No GPU.
Synthetic data only; nobody has measured real files.

Per seed: make_stretch_problem(seed, duration) behind the true sync (workloads.cues.true_sync), the table from
cue_report.cue_table, the model's profiles at every (rho, m) and its paths at every (penalty_q, jump_q), order kept.
Per setting, pooled over the seeds:
  stretch_recovered / isolated_recovered   the share of the class's cues with |delta + displacement| <= 10 samples
  untouched_moved                          the share of untouched cues with |delta| > 10 samples
  order_violations                         consecutive live cues, in order in the input, whose shifted starts are reversed
The baseline is the existing per-cue path on the same files: cue_report's model at its defaults, assess_cues, snap_cues
(delta = best_delta for a "shifted" cue, 0 otherwise), the same three figures.

The rule for the defaults, on the 2 h table: among the settings whose untouched_moved does not exceed the baseline's, the
one with the highest stretch_recovered; ties go to the higher isolated_recovered, then to the first setting of the grid.

    python profiles/cue_retime_calibration.py [--seeds 64] [--jobs 8] [--out profiles/cue_retime_calibration.json]
"""
import argparse
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import cue_model as cm  # noqa: E402
import retime_model as rm  # noqa: E402
from ffsubsync_amd import cue_report as cr  # noqa: E402
from workloads import cue_stretches as ws  # noqa: E402

RADII = (300, 600)
CONTEXTS = (0, 100, 200)
PENALTIES = (0, 4, 16, 64, 256)
JUMPS = (-1, 64 * 50, 64 * 150, 64 * 400)
SETTINGS = [(pq, jq) for pq in PENALTIES for jq in JUMPS]
DURATIONS = (7200.0, 600.0)
ERR_OK = 10
FIELDS = ("n_stretch", "n_isolated", "n_untouched", "stretch_recovered", "isolated_recovered", "untouched_moved",
          "order_violations")


def key(radius, context, penalty_q, jump_q):
    return "%d/%d/%d/%d" % (radius, context, penalty_q, jump_q)


def figures(pr, live, pos, delta):
    """The counts behind the three figures: ``delta`` per cue (0 for a skipped one), ``live`` the live cues' indices."""
    err = np.abs(delta + pr.displacement)
    st, iso, un = pr.kind == ws.STRETCH, pr.kind == ws.ISOLATED, pr.kind == ws.UNTOUCHED
    on = np.zeros(pr.kind.size, bool)
    on[live] = True
    a, b = live[:-1], live[1:]
    was_ordered = pos[b] >= pos[a]
    reversed_now = pos[b] + delta[b] < pos[a] + delta[a]
    return dict(n_stretch=int((st & on).sum()), n_isolated=int((iso & on).sum()), n_untouched=int((un & on).sum()),
                stretch_recovered=int((st & on & (err <= ERR_OK)).sum()),
                isolated_recovered=int((iso & on & (err <= ERR_OK)).sum()),
                untouched_moved=int((un & on & (np.abs(delta) > ERR_OK)).sum()),
                order_violations=int((was_ordered & reversed_now).sum()))


def problem(seed, duration):
    pr = ws.make_stretch_problem(seed, duration)
    res = ws.true_sync(pr)
    table = cr.cue_table(pr.start_us, pr.end_us, res.ratio, res.cue_start_us)
    return pr, table, ws.host_subtitle_vector(pr)


def retime_figures(pr, table, sub, radius, context, settings):
    """figures() of the model at one (rho, m) and every setting of ``settings``."""
    flags, pos, A = rm.profiles(cm.Pair(pr.ref, sub), table, radius, context)
    live = np.flatnonzero(flags == 0)
    paths, _ = rm.retime_paths(flags, pos, A, radius, settings, keep_order=True)
    out = []
    for path in paths:
        delta = np.zeros(flags.size, np.int64)
        delta[live] = path
        out.append(figures(pr, live, pos, delta))
    return out


def baseline_figures(pr, table, sub):
    """figures() of assess_cues + snap_cues at cue_report's defaults."""
    recs = cm.cue_report(pr.ref, sub, table, cr.DEFAULT_RADIUS, cr.DEFAULT_CONTEXT, (0.0, 1.0),
                         (0.0, min(1.0 / pr.ratio, 1.0)))
    verdicts = np.array(cr.assess_cues([cr.from_record(x) for x in recs]))
    delta = np.where(verdicts == "shifted", recs["best_delta"].astype(np.int64), 0)
    live = np.flatnonzero((recs["flags"] & (cm.EMPTY | cm.INVALID)) == 0)
    pos = np.clip(recs["start"], 0, sub.size) + recs["lag"]
    return figures(pr, live, pos, delta)


def _one(job):
    seed, duration = job
    pr, table, sub = problem(seed, duration)
    out = {"baseline": baseline_figures(pr, table, sub)}
    for radius in RADII:
        for context in CONTEXTS:
            for (pq, jq), f in zip(SETTINGS, retime_figures(pr, table, sub, radius, context, SETTINGS)):
                out[key(radius, context, pq, jq)] = f
    return seed, duration, out


def _pool(rows, duration, k):
    t = {f: sum(r[2][k][f] for r in rows if r[1] == duration) for f in FIELDS}
    t["stretch_recovered_share"] = round(t["stretch_recovered"] / max(t["n_stretch"], 1), 4)
    t["isolated_recovered_share"] = round(t["isolated_recovered"] / max(t["n_isolated"], 1), 4)
    t["untouched_moved_share"] = round(t["untouched_moved"] / max(t["n_untouched"], 1), 4)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cue_retime_calibration.json"))
    args = ap.parse_args()
    jobs = [(seed, d) for d in DURATIONS for seed in range(args.seeds)]
    with Pool(args.jobs) as pool:
        rows = pool.map(_one, jobs, chunksize=1)
    keys = [key(r, m, pq, jq) for r in RADII for m in CONTEXTS for pq, jq in SETTINGS]
    table = {"%d" % int(d): {k: _pool(rows, d, k) for k in ["baseline"] + keys} for d in DURATIONS}
    long = table["%d" % int(DURATIONS[0])]
    base = long["baseline"]
    allowed = [k for k in keys if long[k]["untouched_moved"] * base["n_untouched"] <= base["untouched_moved"] * long[k]["n_untouched"]]
    pick = max(allowed, key=lambda k: (long[k]["stretch_recovered"], long[k]["isolated_recovered"], -keys.index(k))) if allowed else None
    chosen = None
    per_seed = {}
    if pick:
        radius, context, pq, jq = (int(x) for x in pick.split("/"))
        chosen = dict(radius=radius, context=context, penalty_q=pq, jump_q=jq, key=pick,
                      beats_baseline_on_stretches=bool(long[pick]["stretch_recovered_share"] > base["stretch_recovered_share"]))
        for seed, d, out in rows:
            per_seed.setdefault("%d" % int(d), {})["%d" % seed] = dict(retime=out[pick], baseline=out["baseline"])
    doc = dict(note="synthetic data only; nobody has measured real files", seeds=args.seeds, radii=RADII, contexts=CONTEXTS,
               penalties_q=PENALTIES, jumps_q=JUMPS, err_ok_samples=ERR_OK, n_allowed=len(allowed), table=table,
               chosen=chosen, per_seed=per_seed)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(chosen=chosen, baseline={d: table[d]["baseline"] for d in table},
                          picked={d: table[d][pick] for d in table} if pick else None), indent=1))


if __name__ == "__main__":
    main()
