"""The z threshold of the shuffled-cue significance test, by rule.  CPU model only
(tests/surrogate_model.py with tests/exact_reference.py), synthetic data only (workloads/synth.make_pair_spec): no device
is involved.

Data: per duration N seeds; matched = the true-ratio candidate of seed i against the reference of seed i, wrong = the same
candidate against the reference of seed i + 1 (the classes of DESIGN 3.5).  W = 6000, K = 64 surrogates, block_units B in
{1, 8}, the seed of file i = fmix32(0 + i) as ``null_test_lists`` derives it from seed 0.

Per class and B: the ranges of the real score, of the null mean and std and of z; the matched files' largest n_ge; the
wrong files' n_ge, one per file, and their histogram over four equal bins of [0, K] (an exchangeable null spreads them
evenly: the chi-square statistic against the uniform expectation is reported, 3 degrees of freedom, 7.81 = the 5 % point).

RULE: DEFAULT_MIN_Z = the midpoint between the smallest matched z and the largest wrong z over every cell (both durations,
both B: one default has to serve either block size), rounded to 0.1, if the classes separate (smallest matched > largest
wrong); otherwise none is shipped and the verdict is ``n_ge == 0`` alone.  The same two figures are reported per B.

    python profiles/null_calibration.py [--seeds 32] [--durations 600 3600] [--jobs 8] > profiles/null_calibration.json
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import surrogate_model as sm  # noqa: E402
from workloads import synth  # noqa: E402

W, K, BLOCK_UNITS, SEED = 6000, 64, (1, 8), 0


def one_file(job):
    dur, i, kind, b = job
    sp = synth.make_pair_spec(i, duration_s=dur)
    ref_sp = sp if kind == "matched" else synth.make_pair_spec(i + 1, duration_s=dur)
    ref = synth.rasterize(ref_sp.ref_len, ref_sp.ref_starts, ref_sp.ref_ends)
    j = sp.true_ratio_index
    sub = synth.rasterize(sp.cand_len[j], sp.cand_starts[j], sp.cand_ends[j])
    sc, fl = sm.null_scores(ref, sub, (0.0, 1.0), (0.0, sp.cand_amp[j]), W, sm.file_seed(SEED, i), K, b)
    rec = sm.stats(sc, fl)
    z, p = sm.z_p(rec)
    print("%s %g s seed %d B=%d: z %.2f n_ge %d" % (kind, dur, i, b, z, rec["n_ge"]), file=sys.stderr)
    return dict(duration=dur, seed=i, kind=kind, block_units=b, blocks=sm.n_blocks(sm.boundaries(sub).size, b),
                real=rec["real_score"], null_mean=rec["null_mean"], null_std=rec["null_std"], n_null=rec["n_null"],
                n_ge=rec["n_ge"], z=z, p=p, flags=rec["flags"])


def span(values):
    return [round(float(min(values)), 3), round(float(max(values)), 3)]


def summarise(files):
    cells = []
    for dur in sorted({f["duration"] for f in files}):
        for b in BLOCK_UNITS:
            for kind in ("matched", "wrong"):
                fs = [f for f in files if f["duration"] == dur and f["block_units"] == b and f["kind"] == kind]
                cell = dict(duration=dur, block_units=b, kind=kind, files=len(fs), real=span([f["real"] for f in fs]),
                            null_mean=span([f["null_mean"] for f in fs]), null_std=span([f["null_std"] for f in fs]),
                            z=span([f["z"] for f in fs]), max_n_ge=max(f["n_ge"] for f in fs))
                if kind == "wrong":
                    n_ge = [f["n_ge"] for f in fs]
                    hist = np.histogram(n_ge, bins=4, range=(0, K + 1))[0]
                    expect = len(fs) / 4.0
                    cell.update(n_ge=n_ge, n_ge_quarters=[int(h) for h in hist],
                                chi_square_3dof=round(float(((hist - expect) ** 2 / expect).sum()), 2),
                                n_ge_zero=int(sum(1 for x in n_ge if x == 0)))
                cells.append(cell)
    return cells


def ship(files):
    def edge(fs):
        lo = min(f["z"] for f in fs if f["kind"] == "matched")
        hi = max(f["z"] for f in fs if f["kind"] == "wrong")
        return dict(smallest_matched_z=round(lo, 3), largest_wrong_z=round(hi, 3), separate=bool(lo > hi),
                    min_z=round((lo + hi) / 2.0, 1) if lo > hi else None)

    out = edge(files)
    out["per_block_units"] = {str(b): edge([f for f in files if f["block_units"] == b]) for b in BLOCK_UNITS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--durations", type=float, nargs="+", default=[600.0, 3600.0])
    ap.add_argument("--jobs", type=int, default=1)
    a = ap.parse_args()
    jobs = [(dur, i, kind, b) for dur in a.durations for b in BLOCK_UNITS for i in range(a.seeds) for kind in ("matched", "wrong")]
    if a.jobs > 1:
        with multiprocessing.Pool(a.jobs) as pool:
            files = pool.map(one_file, jobs, chunksize=1)
    else:
        files = [one_file(j) for j in jobs]
    json.dump(dict(model="tests/surrogate_model.py + tests/exact_reference.py (CPU, synthetic: workloads/synth.make_pair_spec)",
                   seeds=a.seeds, durations=a.durations, W=W, n_surrogates=K, block_units=list(BLOCK_UNITS), seed=SEED,
                   cells=summarise(files), shipped=ship(files),
                   files=[{k: (round(v, 4) if isinstance(v, float) else v) for k, v in f.items()} for f in files]),
              sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
