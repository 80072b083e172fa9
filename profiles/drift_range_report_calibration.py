"""Calibration of drift_range_report.DEFAULT_MIN_SEGMENT_PSR / DEFAULT_MIN_GAIN / DEFAULT_MIN_DRIFT_GAIN on the CPU model
(tests/drift_range_report_model.py on the path of tests/drift_range_model.py) over the SYNTHETIC problems of
workloads/cut_drift.py.  No GPU: the device equals the model bit for bit (tests/test_gpu_drift_range_report.py).

DESIGN 3.14's setup: one-hour problems with 22.5-30 min of inserted scenes, each pair's full overlap range (about 880 k
lags, 350 blocks), K = 1024, P = 8192, max_step = 2, step_cost = 64; top_k 3, E = 300.  Classes:
  clean    seeds 0..15, clean=True: the inserts without drift
  drift    seeds 0..15 as drawn: |eps| in [3e-4, 6e-4], half of them with a wobble
  steep    cut_drift.steep_seeds(8), fixed=True: eps = +-6e-4
  wrong    the subtitle track of drift seed i against the reference of drift seed i + 1, seeds 0..15
  clean32  the clean problems at step_cost = 32, the cost at which DESIGN 3.14 found invented steps
Every problem runs on the candidate the windowless seven-ratio solve picks: the track rasterised at each candidate ratio
as workloads/drift.py rasterises it, the ratio whose correlation over every lag with an overlap has the largest maximum.

Per class: the ranges of segment psr, of jump gain min(gain_next_i, gain_prev_{i+1}) -- true inserts (the offset change
is within 2 s of an inserted stretch) against the other jumps, a jump with a NaN side counted apart -- and of drift_gain
of the segments that took a step; per problem, the decision under the module's defaults ("drift" = assess_drift has no
reason; anything else goes to checked_cut_sync).

    python profiles/drift_range_report_calibration.py [workers]    # writes profiles/drift_range_report_calibration.json
    python profiles/drift_range_report_calibration.py --rescore    # the recorded reports, the module's current defaults
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

K, P, MAX_STEP, STEP_COST, TOP_K, EXCL = 1024, 8192.0, 2, 64.0, 3, 300
CHEAP_STEP_COST = 32.0
INSERT_TOLERANCE = 200  # samples: a jump whose offset change is within 2 s of an inserted stretch is a true insert
OUT = os.path.join(ROOT, "profiles", "drift_range_report_calibration.json")


def tasks():
    from workloads import cut_drift

    out = [("clean", s) for s in range(16)] + [("drift", s) for s in range(16)]
    out += [("steep", s) for s in cut_drift.steep_seeds(8)] + [("wrong", s) for s in range(16)]
    return out


def _raster_at(start_us, end_us, ratio):
    """The candidate at ``ratio`` as workloads.drift.make_problem rasterises it."""
    from ffsubsync_amd.constants import SAMPLE_RATE as sr
    from workloads import synth

    a0, a1 = start_us / 1e6 * ratio, end_us / 1e6 * ratio
    n = int(a1.max() * sr) + 2
    st = np.rint(a0 * sr).astype(np.int64)
    en = np.minimum(st + np.rint((a1 - a0) * sr).astype(np.int64), n)
    return synth.rasterize(n, st, en)


def pick_candidate(ref, start_us, end_us):
    """(ratio index, candidate bits, its upper level) of the windowless seven-ratio solve: the largest correlation of the
    mapped levels over every lag with an overlap."""
    from ffsubsync_amd.constants import candidate_ratios

    r = 2.0 * (np.asarray(ref) != 0) - 1.0
    best = None
    for ri, ratio in enumerate(candidate_ratios()):
        sub = _raster_at(start_us, end_us, ratio)
        hi = min(1.0 / ratio, 1.0)
        s = np.where(sub != 0, 2.0 * hi - 1.0, -1.0)
        n = 1 << int(math.ceil(math.log2(r.size + s.size)))
        top = float(np.fft.irfft(np.fft.rfft(r, n) * np.conj(np.fft.rfft(s, n)), n).max())
        if best is None or top > best[0]:
            best = (top, ri, sub, hi)
    return best[1], best[2], best[3]


def _row(cls, seed, step_cost, ref, sub, hi, lo, top, offs, jump, total, ratio_index, insert_samples):
    import drift_range_report_model as m
    from ffsubsync_amd import drift_report as dr

    recs, _ = m.report(ref, sub, (0.0, 1.0), (0.0, hi), K, lo, top, offs, jump, TOP_K, EXCL)
    q = [dr.from_record(r) for r in recs]
    nan = lambda x: None if isinstance(x, float) and math.isnan(x) else x
    segs = [dict(first_block=s.first_block, end_block=s.end_block, psr=s.psr, flat=s.flat, stepped=s.stepped,
                 steps=int(np.count_nonzero(np.diff(offs[s.first_block:s.end_block]))), spread=s.max_offset - s.min_offset,
                 first_offset=s.first_offset, last_offset=s.last_offset, drift_gain=s.drift_gain,
                 gain_prev=nan(s.gain_prev), gain_next=nan(s.gain_next), own_is_peak=s.own_is_peak, n_lags=s.n_lags)
            for s in q]
    jumps = []
    for a, b in zip(q[:-1], q[1:]):
        g = None if math.isnan(a.gain_next) or math.isnan(b.gain_prev) else min(a.gain_next, b.gain_prev)
        change = b.first_offset - a.last_offset
        true = any(abs(change - n) <= INSERT_TOLERANCE for n in insert_samples)
        jumps.append(dict(block=b.first_block, gain=g, true_insert=bool(true)))
    return dict(cls=cls, seed=seed, step_cost=step_cost, ratio_index=ratio_index, total=total, segments=segs, jumps=jumps)


def run_task(task):
    import cut_model as cm
    import drift_range_model as drgm
    from workloads import cut_drift

    cls, seed = task
    if cls == "wrong":
        a = cut_drift.make_problem(seed)
        ref = cut_drift.make_problem(seed + 1).ref
        start_us, end_us, inserts = a.pair.start_us, a.pair.end_us, []
    else:
        a = cut_drift.make_problem(seed, clean=cls == "clean", fixed=cls == "steep")
        ref, start_us, end_us = a.ref, a.pair.start_us, a.pair.end_us
        inserts = [int(round(x * 100)) for x in a.insert_len_s]
    ri, sub, hi = pick_candidate(ref, start_us, end_us)
    lo, top = cm.full_range(ref.size, sub.size)
    pair = cm._Pair(ref, sub, (0.0, 1.0), (0.0, hi), K, lo, top)
    costs = (STEP_COST, CHEAP_STEP_COST) if cls == "clean" else (STEP_COST,)
    dps = {q: drgm.RowDP(P, MAX_STEP, q) for q in costs}
    for b in range(pair.n_blocks):
        row = pair.scores(b)
        for dp in dps.values():
            dp.push(row)
    out = []
    for q, dp in dps.items():
        o, jump, total = dp.finish()
        name = cls if q == STEP_COST else "clean32"
        out.append(_row(name, seed, q, ref, sub, hi, lo, top, o + lo, jump, float(total), ri, inserts))
    return out


class _Q:  # the fields drift_report.assess_drift reads
    pass


def decide(row, dr):
    """(whether checked_cut_drift_sync applies the drift solve, the reasons) under the module's defaults."""
    qs = []
    for s in row["segments"]:
        q = _Q()
        q.flat, q.psr, q.stepped, q.drift_gain, q.first_block = s["flat"], s["psr"], s["stepped"], s["drift_gain"], s["first_block"]
        q.gain_prev = math.nan if s["gain_prev"] is None else s["gain_prev"]
        q.gain_next = math.nan if s["gain_next"] is None else s["gain_next"]
        qs.append(q)
    ok, reasons = dr.decide_drift(qs)
    return ok, reasons


def _rng(xs):
    xs = [float(x) for x in xs]
    return dict(n=len(xs), min=min(xs), max=max(xs)) if xs else dict(n=0, min=None, max=None)


def summarise(rows):
    out = []
    for cls in ("clean", "drift", "steep", "wrong", "clean32"):
        rs = [r for r in rows if r["cls"] == cls]
        segs = [s for r in rs for s in r["segments"]]
        jumps = [j for r in rs for j in r["jumps"]]
        out.append(dict(cls=cls, problems=len(rs), segment_psr=_rng(s["psr"] for s in segs),
                        best_segment_psr_per_problem=_rng(max(s["psr"] for s in r["segments"]) for r in rs),
                        least_segment_psr_per_problem=_rng(min(s["psr"] for s in r["segments"]) for r in rs),
                        segments_per_problem=_rng(len(r["segments"]) for r in rs),
                        problems_with_steps=sum(any(s["stepped"] for s in r["segments"]) for r in rs),
                        drift_gain_of_stepping_segments=_rng(s["drift_gain"] for s in segs if s["stepped"]),
                        true_insert_gain=_rng(j["gain"] for j in jumps if j["true_insert"] and j["gain"] is not None),
                        other_jump_gain=_rng(j["gain"] for j in jumps if not j["true_insert"] and j["gain"] is not None),
                        jumps_with_nan_side=sum(j["gain"] is None for j in jumps),
                        own_not_peak=sum(not s["own_is_peak"] for s in segs),
                        decided_drift=sum(bool(r["drift"]) for r in rs)))
    return out


def write(rows):
    from ffsubsync_amd import drift_range_report as drr

    for r in rows:
        r["drift"], r["reasons"] = decide(r, drr)
    rows.sort(key=lambda r: (r["cls"], r["seed"]))
    summary = summarise(rows)
    doc = dict(note="SYNTHETIC data only (workloads/cut_drift.py), CPU model (tests/drift_range_report_model.py); nobody has "
                    "measured real files", block_samples=K, split_penalty=P, max_step=MAX_STEP, step_cost=STEP_COST,
               cheap_step_cost=CHEAP_STEP_COST, top_k=TOP_K, exclusion_samples=EXCL, lag_range="full overlap range",
               defaults=dict(min_segment_psr=drr.DEFAULT_MIN_SEGMENT_PSR, min_gain=drr.DEFAULT_MIN_GAIN,
                             min_drift_gain=drr.DEFAULT_MIN_DRIFT_GAIN), summary=summary, problems=rows)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for l in summary:
        print(json.dumps(l))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--rescore":
        write(json.load(open(OUT))["problems"])
        return
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
    write(rows)


if __name__ == "__main__":
    main()
