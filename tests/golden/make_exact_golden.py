"""Generate tests/golden/exact_golden.npz: the exact reference (tests/exact_reference.py) on the benchmark's inputs.

  - "headline": seeds 0..1023 of workloads.synth.make_pair_spec (2 h @ 100 Hz, seven framerate ratios), lag window
    +-6000 and the same offset filter -- MaxScoreAligner(FFTAligner, None, 100, 60)
  - "windowless": seeds 0..127, every lag of the reference's convolve, no filter -- MaxScoreAligner(FFTAligner())

Per candidate the score (fp64), the offset, n_at_max (lags at the exact maximum) and the flags; per pair the winner
(best_cand, offset, score); exact_reference.save_golden / load_golden hold the layout.  Imports nothing but numpy,
the project's workloads and the exact reference; about 0.8 s per headline pair on one core.

    python tests/golden/make_exact_golden.py [n_headline=1024] [n_windowless=128] [procs=8]
"""
import multiprocessing as mp
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

import numpy as np  # noqa: E402

import exact_reference as er  # noqa: E402

CONFIGS = {"headline": (6000, 6000), "windowless": (None, None)}  # (lag window, offset filter)


def solve_seed(kind, seed):
    """The golden record of one seed (also used by the fixture-honesty test)."""
    from workloads import synth

    window, filt = CONFIGS[kind]
    recs, win = er.solve_spec(synth.make_pair_spec(seed), window, filt)
    return {
        "seed": seed,
        "cand": [[float(r["score"]), r["offset"], r["n_at_max"], r["flags"]] for r in recs],
        "winner": [win["best_cand"], win["offset"], float(win["score"])],
    }


def _job(args):
    return solve_seed(*args)


def main():
    n_head = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    n_wl = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    jobs = [("windowless", s) for s in range(n_wl)] + [("headline", s) for s in range(n_head)]
    with mp.get_context("fork").Pool(procs) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    out = {"windowless": res[:n_wl], "headline": res[n_wl:]}
    er.save_golden(os.path.join(HERE, "exact_golden.npz"), out)
    ties = sum(c[2] >= 2 for k in ("headline", "windowless") for p in out[k] for c in p["cand"])
    print("wrote %d + %d pairs, %d candidate records with n_at_max >= 2" % (n_head, n_wl, ties))


if __name__ == "__main__":
    main()
