"""Cost of a ratio sweep evaluation against a golden-section evaluation -> profiles/ratio_sweep_profile.json.

GPU script: HIP events around whole calls, one warm call first, best of several.  On 1 and on 64 two-hour `free`
problems (workloads/unknown_ratio.py) it times ``ratio_profile_batch`` + ``sweep_peaks`` and, on the same files in the
same process, ``fit_gss_batch``; both are divided by their number of (file, ratio) evaluations.  The only bar: a sweep
evaluation must not cost more than a ``fit_gss_batch`` evaluation -- it issues more vectors per call, never fewer.

    python profiles/ratio_sweep_profile.py [--files 1 64] [--repeats 5] [--duration 7200]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ffsubsync_amd import ratio_sweep  # noqa: E402
from ffsubsync_amd.batch_gss import fit_gss_batch  # noqa: E402
from workloads import unknown_ratio as ur  # noqa: E402

W = 6000


def best_ms(fn, repeats):
    fn()  # warm: plans, allocator, code objects
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--duration", type=float, default=7200.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ratio_sweep_profile.json"))
    args = ap.parse_args()
    rows = []
    for n in args.files:
        probs = [ur.make_problem("free", seed, args.duration) for seed in range(n)]
        problems = [p.problem for p in probs]
        refs, tracks = [p.reference for p in probs], [p.track for p in probs]
        box = {}

        def sweep():
            prof = ratio_sweep.ratio_profile_batch(problems)
            box["peaks"] = ratio_sweep.sweep_peaks(prof.table, prof.first_dev)
            box["prof"] = prof

        def gss():
            box["stats"] = {}
            box["gss"] = fit_gss_batch(refs, tracks, max_offset_samples=W, stats=box["stats"])

        sweep_ms, gss_ms = best_ms(sweep, args.repeats), best_ms(gss, args.repeats)
        sweep_evals = int(box["prof"].first[-1])
        gss_evals = int(box["stats"]["steps"]) * n
        hits = sum(int(pk["peak_index"][0]) == int(abs(g - p.true_ratio).argmin())
                   for pk, g, p in zip(box["peaks"], box["prof"].grids, probs))
        gss_hits = sum(abs(r[1] - p.true_ratio) <= 2e-4 for r, p in zip(box["gss"], probs))
        rows.append({"files": n, "duration_s": args.duration, "sweep_ms": sweep_ms, "sweep_evaluations": sweep_evals,
                     "sweep_us_per_evaluation": 1e3 * sweep_ms / sweep_evals, "sweep_chunks": box["prof"].stats["chunks"],
                     "sweep_maximum_is_nearest_point": "%d of %d" % (hits, n), "gss_ms": gss_ms, "gss_evaluations": gss_evals,
                     "gss_us_per_evaluation": 1e3 * gss_ms / gss_evals, "gss_hits": "%d of %d" % (gss_hits, n),
                     "sweep_evaluation_not_dearer": bool(sweep_ms / sweep_evals <= gss_ms / gss_evals)})
        print(json.dumps(rows[-1]))
    out = {"what": "whole calls between HIP events on one MI355X, warm, best of %d; tolerance %.0f, window %d samples"
                   % (args.repeats, ratio_sweep.DEFAULT_TOLERANCE, W),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
