"""Calibration of the ratio sweep's defaults on the CPU model -> profiles/ratio_sweep_calibration.json.

CPU MODEL ONLY, SYNTHETIC DATA: every score here is ``tests/sweep_model.py``'s (the oracle's FFTAligner on the oracle's
rasters) on the seeded problems of ``workloads/unknown_ratio.py``; no device code runs.  Durations are 10 min and 1 h: a
two-hour sweep on the CPU is ~1 400 solves of 0.4 s per file and tolerance, too slow to repeat over seeds and tolerances.

Phase 1, `free` problems, per tolerance in TOLERANCES: the fraction of the exact-ratio score that the grid maximum keeps,
and whether the maximum is the grid point nearest the truth.  RULE: DEFAULT_TOLERANCE is the largest tolerance whose worst
kept fraction, over both durations, is >= 0.9.
Phase 2, every class at that tolerance: the whole sweep (coarse grid, peaks, fine stage), psr and margin of the ratio
profile, and for `free` the reference's own golden-section search on the same file (hit = within 2e-4 of the truth) and
its best score among the seven framerate ratios.  RULE: min_psr / min_margin are the midpoints between the smallest
value over `free` and `seven` and the largest over `wrong` if these separate; otherwise quality's defaults stay.

    python profiles/ratio_sweep_calibration.py [--procs N] [--quick]
"""
import argparse
import json
import math
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import sweep_model as sm  # noqa: E402
from oracle import aligners_oracle as orc  # noqa: E402
from oracle import raster_oracle as ro  # noqa: E402
from workloads import unknown_ratio as ur  # noqa: E402

TOLERANCES = (10, 15, 25, 40, 60)
W = 6000
KEEP_AT_LEAST = 0.9
SEEDS = {600.0: {"free": range(8), "seven": range(100, 106), "wrong": range(200, 208)},
         3600.0: {"free": range(4), "seven": range(100, 103), "wrong": range(200, 204)}}
QUICK = {600.0: {"free": range(2), "seven": range(100, 101), "wrong": range(200, 202)}}


def phase1(task):
    duration, seed, tol = task
    p = ur.make_problem("free", seed, duration)
    exact = float(sm.evaluate(p.reference, p.track, [p.true_ratio], W)[0][0])
    ratios, step = sm.grid(sm.duration_samples(p.track), tolerance_samples=tol)
    sc, off, fl = sm.evaluate(p.reference, p.track, ratios, W)
    rep = sm.report(sc, off, fl, 3, sm.default_exclusion_steps(tol))
    i = rep["peaks"][0][2]
    return dict(duration=duration, seed=seed, tolerance=tol, grid_points=int(ratios.size), true_ratio=p.true_ratio,
                kept=rep["peaks"][0][0] / exact, nearest=bool(i == int(np.argmin(np.abs(ratios - p.true_ratio)))))


def phase2(task):
    duration, kind, seed, tol = task
    p = ur.make_problem(kind, seed, duration)
    res = sm.sweep(p.reference, p.track, W, tolerance_samples=tol)
    psr, margin = sm.psr_margin(res["report"])
    out = dict(duration=duration, kind=kind, seed=seed, psr=psr, margin=margin, ratio=res["ratio"], offset=res["offset"],
               score=res["score"], step=res["step"])
    if kind != "wrong":
        out["ratio_error_in_fine_steps"] = abs(res["ratio"] - p.true_ratio) / (res["step"] / 16)
        out["offset_error"] = res["offset"] - p.true_offset_samples
    if kind == "free":
        seven = sm.evaluate(p.reference, p.track, sm.SEVEN, W)[0]
        out["best_of_seven_over_sweep"] = float(seven.max()) / res["score"]
        rec = {}

        def objective(r, last):
            s, _ = orc.fft_align(p.reference, ro.rasterize(p.track[0], p.track[1], p.track[2], r, 100, 0), W)
            if last:
                rec["v"] = (r, float(s))
            return -s

        orc.gss_trace(objective, 0.9, 1.1)
        out["gss_ratio"], out["gss_score_over_sweep"] = rec["v"][0], rec["v"][1] / res["score"]
        out["gss_hit"] = bool(abs(rec["v"][0] - p.true_ratio) <= 2e-4)
        out["true_ratio"] = p.true_ratio
    return out


def span(xs):
    xs = [float(x) for x in xs]
    return [min(xs), max(xs)] if xs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=max(1, min(8, (os.cpu_count() or 2) - 1)))
    ap.add_argument("--quick", action="store_true", help="two 10-min seeds per class, nothing written")
    args = ap.parse_args()
    seeds = QUICK if args.quick else SEEDS
    with multiprocessing.Pool(args.procs) as pool:
        t1 = [(d, s, t) for d in seeds for s in seeds[d]["free"] for t in TOLERANCES]
        t1.sort(key=lambda x: -x[0] / x[2])  # longest first
        r1 = pool.map(phase1, t1, chunksize=1)
        kept = {t: {d: [r["kept"] for r in r1 if r["tolerance"] == t and r["duration"] == d] for d in seeds} for t in TOLERANCES}
        worst = {t: min(min(v) for v in kept[t].values()) for t in TOLERANCES}
        passing = [t for t in TOLERANCES if worst[t] >= KEEP_AT_LEAST]
        if not passing:
            raise SystemExit("no tolerance keeps %.2f of the exact-ratio score: %r" % (KEEP_AT_LEAST, worst))
        tol = max(passing)
        t2 = [(d, k, s, tol) for d in sorted(seeds, reverse=True) for k in ur.CLASSES for s in seeds[d][k]]
        r2 = pool.map(phase2, t2, chunksize=1)
    good = [r for r in r2 if r["kind"] != "wrong"]
    bad = [r for r in r2 if r["kind"] == "wrong"]
    rules = {"default_tolerance": tol}
    for key, fallback in (("psr", 5.0), ("margin", 3.0)):
        lo_good, hi_bad = min(r[key] for r in good), max(r[key] for r in bad)
        rules[key + "_separates"] = bool(lo_good > hi_bad)
        rules["min_" + key] = round((lo_good + hi_bad) / 2, 2) if lo_good > hi_bad else fallback
    free = [r for r in r2 if r["kind"] == "free"]
    out = {
        "what": "CPU model only (tests/sweep_model.py on workloads/unknown_ratio.py), synthetic data, no device code; "
                "durations 600 s and 3600 s (two-hour sweeps are too slow on the CPU)",
        "window_samples": W, "tolerances": list(TOLERANCES), "keep_at_least": KEEP_AT_LEAST,
        "seeds": {str(int(d)): {k: [int(s) for s in v] for k, v in seeds[d].items()} for d in seeds},
        "per_tolerance": {str(t): {"worst_kept": worst[t],
                                   "kept": {str(int(d)): span(kept[t][d]) for d in seeds},
                                   "grid_points": {str(int(d)): max(r["grid_points"] for r in r1 if r["tolerance"] == t and r["duration"] == d) for d in seeds},
                                   "maximum_is_nearest_point": "%d of %d" % (sum(r["nearest"] for r in r1 if r["tolerance"] == t),
                                                                             sum(1 for r in r1 if r["tolerance"] == t))}
                          for t in TOLERANCES},
        "at_default_tolerance": {
            kind: {str(int(d)): {"psr": span(r["psr"] for r in r2 if r["kind"] == kind and r["duration"] == d),
                                 "margin": span(r["margin"] for r in r2 if r["kind"] == kind and r["duration"] == d)}
                   for d in seeds} for kind in ur.CLASSES},
        "found": {"ratio_error_in_fine_steps": span(r["ratio_error_in_fine_steps"] for r in good),
                  "offset_error_samples": span(r["offset_error"] for r in good)},
        "free_against_the_baselines": {
            "gss_hits": "%d of %d" % (sum(r["gss_hit"] for r in free), len(free)),
            "gss_score_over_sweep": span(r["gss_score_over_sweep"] for r in free),
            "best_of_seven_over_sweep": span(r["best_of_seven_over_sweep"] for r in free)},
        "rules": rules,
        "files": r2,
    }
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.quick:
        print(text)
        return
    with open(os.path.join(ROOT, "profiles", "ratio_sweep_calibration.json"), "w") as f:
        f.write(text + "\n")
    print(json.dumps({k: out[k] for k in ("per_tolerance", "at_default_tolerance", "rules", "free_against_the_baselines", "found")}, indent=1))


if __name__ == "__main__":
    main()
