"""The tolerance and the share threshold of the half-sample stability test, by rule.  CPU model only
(tests/stability_model.py with tests/exact_reference.py), synthetic data only (workloads/synth.make_pair_spec): no device
is involved and no real file has been measured.

Data: the files and classes of profiles/null_calibration.py.  Per duration N seeds; matched = the true-ratio candidate of
seed i against the reference of seed i, wrong = the same candidate against the reference of seed i + 1.  W = 6000, K = 64
half-samples, block_runs B in {1, 8}, the seed of file i = fmix32(0 + i) as ``stability_test_lists`` derives it from seed 0.

Per file the sorted |offset - real offset| of its usable half-samples is kept, so the share within any tol can be
recomputed from the JSON (tests/test_stability_host.py does).

RULES.  DEFAULT_TOL = twice the largest matched max_dev over every cell (both durations, both B); the factor 2 is margin
for real audio, which is noisier than the synthetic pairs.  DEFAULT_MIN_SHARE = the midpoint between the smallest matched
and the largest wrong share_within at that tol, rounded to 0.01, if the classes separate (smallest matched > largest
wrong); otherwise no ``stable`` verdict is shipped and the interval is reported alone.

    python profiles/stability_calibration.py [--seeds 32] [--durations 600 3600] [--jobs 8] > profiles/stability_calibration.json
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import stability_model as stm  # noqa: E402
from workloads import synth  # noqa: E402

W, K, BLOCK_RUNS, SEED = 6000, 64, (1, 8), 0


def one_file(job):
    dur, i, kind, b = job
    sp = synth.make_pair_spec(i, duration_s=dur)
    ref_sp = sp if kind == "matched" else synth.make_pair_spec(i + 1, duration_s=dur)
    ref = synth.rasterize(ref_sp.ref_len, ref_sp.ref_starts, ref_sp.ref_ends)
    j = sp.true_ratio_index
    sub = synth.rasterize(sp.cand_len[j], sp.cand_starts[j], sp.cand_ends[j])
    sc, off, fl = stm.half_records(ref, sub, (0.0, 1.0), (0.0, sp.cand_amp[j]), W, stm.file_seed(SEED, i), K, b)
    rec = stm.offset_stats(sc, off, fl, 0)
    ok = stm.usable(sc, fl)
    devs = sorted(abs(int(o) - int(off[0])) for o, u in zip(off[1:], ok[1:]) if u)
    print("%s %g s seed %d B=%d: max_dev %d, interval [%d, %d] around %d" % (kind, dur, i, b, rec["max_dev"], rec["off_lo"],
                                                                               rec["off_hi"], rec["real_offset"]), file=sys.stderr)
    return dict(duration=dur, seed=i, kind=kind, block_runs=b, blocks=stm.n_blocks(stm.boundaries(sub).size, b),
                real_offset=rec["real_offset"], off_lo=rec["off_lo"], off_hi=rec["off_hi"], off_median=rec["off_median"],
                max_dev=rec["max_dev"], max_pair_gap=rec["max_pair_gap"], n_sub=rec["n_sub"], n_pairs=rec["n_pairs"],
                flags=rec["flags"], pair_score_min=rec["pair_score_min"], real_score=rec["real_score"], devs=devs)


def share(f, tol):
    return sum(1 for d in f["devs"] if d <= tol) / f["n_sub"] if f["n_sub"] else 0.0


def ship(files):
    """The two defaults by the rules above, from the per-file rows alone."""
    tol = 2 * max(f["max_dev"] for f in files if f["kind"] == "matched")
    lo = min(share(f, tol) for f in files if f["kind"] == "matched")
    hi = max(share(f, tol) for f in files if f["kind"] == "wrong")
    return dict(largest_matched_max_dev=tol // 2, tol=tol, smallest_matched_share=round(lo, 4), largest_wrong_share=round(hi, 4),
                separate=bool(lo > hi), min_share=round((lo + hi) / 2.0, 2) if lo > hi else None)


def summarise(files, tol):
    cells = []
    for dur in sorted({f["duration"] for f in files}):
        for b in BLOCK_RUNS:
            for kind in ("matched", "wrong"):
                fs = [f for f in files if f["duration"] == dur and f["block_runs"] == b and f["kind"] == kind]
                shares = [share(f, tol) for f in fs]
                widths = [f["off_hi"] - f["off_lo"] for f in fs]
                cells.append(dict(duration=dur, block_runs=b, kind=kind, files=len(fs),
                                  max_dev=[min(f["max_dev"] for f in fs), max(f["max_dev"] for f in fs)],
                                  interval_width=[min(widths), max(widths)],
                                  max_pair_gap=[min(f["max_pair_gap"] for f in fs), max(f["max_pair_gap"] for f in fs)],
                                  share_within=[round(min(shares), 4), round(max(shares), 4)],
                                  pair_score_min_below_real=sum(1 for f in fs if f["pair_score_min"] < f["real_score"])))
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--durations", type=float, nargs="+", default=[600.0, 3600.0])
    ap.add_argument("--jobs", type=int, default=1)
    a = ap.parse_args()
    jobs = [(dur, i, kind, b) for dur in a.durations for b in BLOCK_RUNS for i in range(a.seeds) for kind in ("matched", "wrong")]
    if a.jobs > 1:
        with multiprocessing.Pool(a.jobs) as pool:
            files = pool.map(one_file, jobs, chunksize=1)
    else:
        files = [one_file(j) for j in jobs]
    shipped = ship(files)
    head = json.dumps(dict(model="tests/stability_model.py + tests/exact_reference.py (CPU, synthetic: workloads/synth.make_pair_spec)",
                           seeds=a.seeds, durations=a.durations, W=W, n_subsamples=K, block_runs=list(BLOCK_RUNS), seed=SEED,
                           cells=summarise(files, shipped["tol"]), shipped=shipped), indent=1)
    rows = [json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in f.items()}) for f in files]  # a file a line
    print(head[:-2] + ',\n "files": [\n  ' + ",\n  ".join(rows) + "\n ]\n}")


if __name__ == "__main__":
    main()
