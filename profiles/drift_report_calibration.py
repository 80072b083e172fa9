"""Calibration of drift_report.DEFAULT_MIN_SEGMENT_PSR / DEFAULT_MIN_GAIN / DEFAULT_MIN_DRIFT_GAIN on the CPU model
(tests/drift_report_model.py) over the SYNTHETIC problems of workloads/drift.py.  No GPU: the device equals the model
bit for bit (tests/test_gpu_drift_report.py).

Two-hour problems, K = 1024, P = 8192, max_step = 2, E = 300.  Classes:
  a  drifting as drawn, seeds 0..23, +-60 s            (and seeds 0..7 at +-10 min)
  b  drifting with insert_break=True, seeds 0..7, +-5 min: one true break per problem
  c  clean, step_cost = 128 (the default), seeds 0..23, +-60 s   (and seeds 0..7 at +-10 min)
  d  clean, step_cost = 32, seeds 0..39, +-60 s: the cost at which DESIGN 3.10 found invented drift
  e  wrong pairs: the subtitle of seed i against the reference of seed i+1, seeds 0..23, +-60 s (and 0..7 at +-10 min),
     the candidate at the ratio with the best whole-file score in the window (what the seven-ratio solve picks)
Per class: the ranges of segment psr, of jump gain min(gain_next_i, gain_prev_{i+1}) (a jump with a NaN side has no gain: it is unsupported whatever the floor, and is counted apart)
and of drift_gain of the segments that took a step.

    python profiles/drift_report_calibration.py [workers]     # writes profiles/drift_report_calibration.json
"""
import json
import math
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, P, MAX_STEP, TOP_K, EXCL = 1024, 8192.0, 2, 3, 300
DURATION_S = 7200.0
BREAK_TOLERANCE = 200  # samples: a jump whose offset change is within 2 s of the inserted stretch is the true break


def tasks():
    out = []
    for w, n_a, n_d in ((6000, 24, 40), (60000, 8, 0)):
        out += [("a", s, w) for s in range(n_a)]
        out += [("c", s, w) for s in range(n_a)]  # class d rides on c's block scores at +-60 s
        out += [("d", s, w) for s in range(n_a, n_d)]
        out += [("e", s, w) for s in range(n_a)]
    out += [("b", s, 30000) for s in range(8)]
    return sorted(out, key=lambda t: -t[2])  # the long ones first


def _raster_at(start_us, end_us, ratio):
    """The candidate at ``ratio`` as workloads.drift.make_problem rasterises it."""
    from ffsubsync_amd.constants import SAMPLE_RATE as sr
    from workloads import synth

    a0, a1 = start_us / 1e6 * ratio, end_us / 1e6 * ratio
    n = int(a1.max() * sr) + 2
    st = np.rint(a0 * sr).astype(np.int64)
    en = np.minimum(st + np.rint((a1 - a0) * sr).astype(np.int64), n)
    return synth.rasterize(n, st, en)


def _rows(cls, seed, w, step_cost, ref, sub, sub_hi, n11, break_samples=None):
    import drift_report_model as drm
    from ffsubsync_amd import drift_report as dr

    (offs, _, jump, total), recs, _ = drm.report(ref, sub, (0.0, 1.0), (0.0, sub_hi), K, w, P, MAX_STEP, step_cost, TOP_K,
                                                 EXCL, n11_blocks=n11)
    q = [dr.from_record(r) for r in recs]
    segs = [dict(first_block=s.first_block, end_block=s.end_block, psr=s.psr, stepped=s.stepped,
                 steps=int(np.count_nonzero(np.diff(offs[s.first_block:s.end_block]))), spread=s.max_offset - s.min_offset,
                 drift_gain=s.drift_gain, flat=s.flat, own_is_peak=s.own_is_peak, n_lags=s.n_lags) for s in q]
    jumps = []
    for a, b in zip(q[:-1], q[1:]):
        g = None if math.isnan(a.gain_next) or math.isnan(b.gain_prev) else min(a.gain_next, b.gain_prev)
        true = break_samples is not None and abs((b.first_offset - a.last_offset) - break_samples) <= BREAK_TOLERANCE
        jumps.append(dict(block=b.first_block, gain=g, true_break=bool(true)))
    return dict(cls=cls, seed=seed, w=w, step_cost=step_cost, total=total, segments=segs, jumps=jumps)


def run_task(task):
    import split_model as sm
    import quality_model as qm
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import drift

    cls, seed, w = task
    out = []
    if cls in ("a", "b"):
        pr = drift.make_problem(seed, duration_s=DURATION_S, insert_break=cls == "b")
        n11 = sm.block_counts(pr.ref, pr.sub, K, w)
        brk = int(round(pr.break_len_s * 100)) if cls == "b" else None
        out.append(_rows(cls, seed, w, 128.0, pr.ref, pr.sub, pr.sub_hi, n11, brk))
    elif cls in ("c", "d"):
        pr = drift.make_problem(seed, duration_s=DURATION_S, clean=True)
        n11 = sm.block_counts(pr.ref, pr.sub, K, w)
        if cls == "c":
            out.append(_rows("c", seed, w, 128.0, pr.ref, pr.sub, pr.sub_hi, n11))
        if w == 6000:
            out.append(_rows("d", seed, w, 32.0, pr.ref, pr.sub, pr.sub_hi, n11))
    else:
        a = drift.make_problem(seed, duration_s=DURATION_S)
        ref = drift.make_problem(seed + 1, duration_s=DURATION_S).ref
        best = None
        for ri, ratio in enumerate(candidate_ratios()):
            sub = _raster_at(a.start_us, a.end_us, ratio)
            hi = min(1.0 / ratio, 1.0)
            top = float(qm.scores(ref, sub, (0.0, 1.0), (0.0, hi), w)[1].max())
            if best is None or top > best[0]:
                best = (top, ri, sub, hi)
        _, ri, sub, hi = best
        n11 = sm.block_counts(ref, sub, K, w)
        row = _rows("e", seed, w, 128.0, ref, sub, hi, n11)
        row["ratio_index"] = ri
        out.append(row)
    return out


def _rng(xs):
    xs = [float(x) for x in xs]
    return dict(n=len(xs), min=min(xs), max=max(xs)) if xs else dict(n=0, min=None, max=None)


def summarise(rows):
    out = []
    keys = sorted(set((r["cls"], r["w"]) for r in rows))
    for cls, w in keys:
        rs = [r for r in rows if (r["cls"], r["w"]) == (cls, w)]
        segs = [s for r in rs for s in r["segments"]]
        jumps = [j for r in rs for j in r["jumps"]]
        out.append(dict(cls=cls, w=w, pairs=len(rs), segment_psr=_rng(s["psr"] for s in segs),
                        segments_per_pair=_rng(len(r["segments"]) for r in rs),
                        pairs_with_steps=sum(any(s["stepped"] for s in r["segments"]) for r in rs),
                        drift_gain_of_stepping_segments=_rng(s["drift_gain"] for s in segs if s["stepped"]),
                        true_break_gain=_rng(j["gain"] for j in jumps if j["true_break"] and j["gain"] is not None),
                        other_jump_gain=_rng(j["gain"] for j in jumps if not j["true_break"] and j["gain"] is not None),
                        jumps_with_nan_side=sum(j["gain"] is None for j in jumps),
                        own_not_peak=sum(not s["own_is_peak"] for s in segs)))
    return out


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    todo = tasks()
    rows = []
    if workers > 1:
        with multiprocessing.Pool(workers) as pool:
            for i, got in enumerate(pool.imap_unordered(run_task, todo)):
                rows += got
                print("%d / %d tasks" % (i + 1, len(todo)), flush=True)
    else:
        for i, t in enumerate(todo):
            rows += run_task(t)
            print("%d / %d tasks" % (i + 1, len(todo)), flush=True)
    rows.sort(key=lambda r: (r["w"], r["cls"], r["seed"]))
    summary = summarise(rows)
    doc = dict(note="SYNTHETIC data (workloads/drift.py), CPU model (tests/drift_report_model.py); nobody has measured real "
                    "files", block_samples=K, split_penalty=P, max_step=MAX_STEP, top_k=TOP_K, exclusion_samples=EXCL,
               duration_s=DURATION_S, summary=summary, pairs=rows)
    with open(os.path.join(ROOT, "profiles", "drift_report_calibration.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for l in summary:
        print(json.dumps(l))


if __name__ == "__main__":
    main()
