"""Calibration of the per-cue report's defaults (cue_report.DEFAULT_RADIUS / DEFAULT_CONTEXT / DEFAULT_MIN_GAIN /
DEFAULT_MIN_COVER) on the CPU model tests/cue_model.py and the seeded workload workloads/cues.py.  No GPU.

Per seed: make_cue_problem(seed, duration), 40 displaced + 40 extra cues, the true ratio and offset applied to every cue
(workloads.cues.true_sync), the table from cue_report.cue_table, the model at every radius rho and context m.  Per
(duration, rho, m) and class (untouched / displaced / extra), pooled over the seeds, the percentiles of
  err     |best_delta + displacement| in samples (the displacement is 0 for untouched and extra cues)
  gain    (best_score - own_score) / (U - L)
  cover   cue_own_n11 / cue_own_ov
and the shares of cues with FFS_CUE_BEST_AT_EDGE and FFS_CUE_SILENT.

The rule for the defaults, applied to the 2 h table (the 10 min files hold as many planted cues as real ones, so their
untouched cues sit in planted neighbourhoods; they are reported, not chosen on): among the (rho, m) whose radius covers
the largest displacement (rho >= 250), the pair with the widest gap between the displaced class's 5th percentile of gain
and the untouched class's 99th; min_gain = the middle of that gap, rounded to 0.01 (a negative gap is an overlap and is
reported as such); min_cover = the untouched class's 1st percentile of cover, rounded down to 0.05.  With the chosen
values: per seed and duration the recall of displaced cues ("shifted" with err <= 10), the share of untouched cues whose
verdict is not "ok", and the verdicts of the extra cues.

    python profiles/cue_report_calibration.py [--seeds 64] [--jobs 8] [--out profiles/cue_report_calibration.json]
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
from ffsubsync_amd import cue_report as cr  # noqa: E402
from workloads import cues as wc  # noqa: E402

RADII = (100, 300, 600)
CONTEXTS = (0, 100, 200, 400)
DURATIONS = (7200.0, 600.0)
PCT = (1, 5, 25, 50, 75, 95, 99)
ERR_OK = 10


def records(seed, duration, radius, context):
    """(problem, model records) of one seed behind the true sync."""
    pr = wc.make_cue_problem(seed, duration)
    res = wc.true_sync(pr)
    table = cr.cue_table(pr.start_us, pr.end_us, res.ratio, res.cue_start_us)
    sub = wc.host_subtitle_vector(pr)
    return pr, cm.cue_report(pr.ref, sub, table, radius, context, (0.0, 1.0), (0.0, min(1.0 / pr.ratio, 1.0)))


def verdict_figures(pr, recs, min_gain, min_cover):
    """What the assessment finds on one problem."""
    verdicts = np.array(cr.assess_cues([cr.from_record(x) for x in recs], min_gain, min_cover))
    err = np.abs(recs["best_delta"].astype(np.int64) + pr.displacement)
    moved, plain, extra = pr.kind == wc.DISPLACED, pr.kind == wc.UNTOUCHED, pr.kind == wc.EXTRA
    return dict(n_displaced=int(moved.sum()), n_untouched=int(plain.sum()), n_extra=int(extra.sum()),
                displaced_found=int(((verdicts == "shifted") & (err <= ERR_OK) & moved).sum()),
                displaced_flagged=int(((verdicts != "ok") & moved).sum()),
                untouched_flagged=int(((verdicts != "ok") & plain).sum()),
                extra_flagged=int(((verdicts != "ok") & extra).sum()),
                extra_silent=int(((verdicts == "silent") & extra).sum()))


def _one(job):
    seed, duration = job
    pr = wc.make_cue_problem(seed, duration)
    res = wc.true_sync(pr)
    table = cr.cue_table(pr.start_us, pr.end_us, res.ratio, res.cue_start_us)
    sub = wc.host_subtitle_vector(pr)
    pair = cm.Pair(pr.ref, sub, (0.0, 1.0), (0.0, min(1.0 / pr.ratio, 1.0)))
    out = {}
    for radius in RADII:
        for context in CONTEXTS:
            recs = np.array([pair.report(int(a), int(e), int(g), radius, context) for a, e, g in zip(*table)], cm.DTYPE)
            live = (recs["flags"] & (cm.EMPTY | cm.INVALID)) == 0
            out["%d/%d" % (radius, context)] = dict(
                kind=pr.kind[live], err=np.abs(recs["best_delta"].astype(np.int64) + pr.displacement)[live],
                gain=((recs["best_score"] - recs["own_score"]) / np.maximum(recs["hi"] - recs["lo"], 1))[live],
                cover=(recs["cue_own_n11"] / np.maximum(recs["cue_own_ov"], 1))[live],
                edge=((recs["flags"] & cm.BEST_AT_EDGE) != 0)[live], silent=((recs["flags"] & cm.SILENT) != 0)[live])
    return seed, duration, out


def _pct(x):
    return [round(float(v), 4) for v in np.percentile(x, PCT)] if len(x) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cue_report_calibration.json"))
    args = ap.parse_args()
    jobs = [(seed, d) for d in DURATIONS for seed in range(args.seeds)]
    with Pool(args.jobs) as pool:
        rows = pool.map(_one, jobs, chunksize=1)
    table = {}
    for d in DURATIONS:
        for radius in RADII:
            for context in CONTEXTS:
                key = "%d/%d" % (radius, context)
                cat = {f: np.concatenate([r[2][key][f] for r in rows if r[1] == d])
                       for f in ("kind", "err", "gain", "cover", "edge", "silent")}
                cell = {}
                for k, name in enumerate(wc.KIND_NAMES):
                    m = cat["kind"] == k
                    cell[name] = dict(n=int(m.sum()), err=_pct(cat["err"][m]), gain=_pct(cat["gain"][m]),
                                      cover=_pct(cat["cover"][m]), err_ok=round(float((cat["err"][m] <= ERR_OK).mean()), 4),
                                      at_edge=round(float(cat["edge"][m].mean()), 4),
                                      silent=round(float(cat["silent"][m].mean()), 4))
                u99, d5 = cell["untouched"]["gain"][PCT.index(99)], cell["displaced"]["gain"][PCT.index(5)]
                cell["gap"] = round(d5 - u99, 4)  # negative: the classes overlap by that much
                table.setdefault("%d" % int(d), {})[key] = cell
    long = table["%d" % int(DURATIONS[0])]
    ok = [k for k in long if int(k.split("/")[0]) >= 250]
    best = max(ok, key=lambda k: (long[k]["gap"], -int(k.split("/")[0]), -int(k.split("/")[1])))
    radius, context = (int(x) for x in best.split("/"))
    u99, d5 = long[best]["untouched"]["gain"][PCT.index(99)], long[best]["displaced"]["gain"][PCT.index(5)]
    min_gain = round((u99 + d5) / 2.0, 2)
    min_cover = float(np.floor(long[best]["untouched"]["cover"][PCT.index(1)] * 20.0) / 20.0)
    chosen = dict(radius=radius, context=context, min_gain=min_gain, min_cover=min_cover, untouched_gain_p99=u99,
                  displaced_gain_p5=d5, gap=long[best]["gap"],
                  gap_10min=table["%d" % int(DURATIONS[1])][best]["gap"])
    per_seed = {}
    for d in DURATIONS:
        for seed in range(args.seeds):
            pr, recs = records(seed, d, radius, context)
            per_seed.setdefault("%d" % int(d), {})["%d" % seed] = verdict_figures(pr, recs, min_gain, min_cover)
    totals = {}
    for d, seeds in per_seed.items():
        t = {f: sum(v[f] for v in seeds.values()) for f in next(iter(seeds.values()))}
        t["recall"] = round(t["displaced_found"] / max(t["n_displaced"], 1), 4)
        t["false_positive"] = round(t["untouched_flagged"] / max(t["n_untouched"], 1), 4)
        totals[d] = t
    doc = dict(note="synthetic data only; nobody has measured real files", seeds=args.seeds, radii=RADII, contexts=CONTEXTS,
               percentiles=PCT, err_ok_samples=ERR_OK, table=table, chosen=chosen, totals=totals, per_seed=per_seed)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(chosen=chosen, totals=totals), indent=1))


if __name__ == "__main__":
    main()
