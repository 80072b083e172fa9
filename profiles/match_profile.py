"""Timing of the all-pairs quality report from boundary lists (ffsubsync_amd.match, csrc/ffs_match.h) against
quality_batch's device call on the same pairs, in ONE process, alternating: 32 x 32 two-hour synthetic vectors
(workloads/synth.make_pair_spec seeds 0..31: each spec's reference, and its candidate at the true ratio), all 1 024 pairs,
+-60 s, top_k 3.  Per round each variant's device call runs once between two HIP events (the descriptors are built
before, the records stay on the device); best of the rounds after one untimed warm round.  The yardstick is
``ffs_align_quality_batch`` on bit-packed rows that share the same 64 vectors -- what quality_batch does for such a batch
-- and, as quality_batch would have to for boundary-list input, the same call behind one ``ffs_runs_to_bits`` per vector
of every pair.  Also: one pair alone, and the sweep behind FFS_MATCH_AUTO_COST -- 64 pairs (8 x 8) at 1x .. 16x the boundary
density (make_pair_spec's run_scale), list path against bit path of the same entry point.

Kernel times come from a separate run under ``rocprofv3 --kernel-trace --stats`` and are folded into the JSON afterwards:

    python profiles/match_profile.py [--out profiles/match_profile.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o match -- \\
        python profiles/match_profile.py --repeats 1 --no-sweep --out /dev/null
    python profiles/match_profile.py --fold-stats DIR/.../match_kernel_stats.csv [--out profiles/match_profile.json]
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

W, TOP_K, E = 6000, 3, 300


def fold_stats(stats_csv: str, out: str) -> None:
    """{kernel: calls, average us, total us} of the library's kernels of a rocprofv3 stats CSV into the JSON."""
    table = {}
    for r in csv.DictReader(open(stats_csv)):
        name = r["Name"]
        short = name.split("ffsa::", 1)[1] if "ffsa::" in name else name
        short = short.split("(", 1)[0]
        if not short.startswith("k_"):
            continue
        table[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                        "total_us": float(r["TotalDurationNs"]) / 1e3}
    result = json.load(open(out))
    result["kernels_one_round"] = {"source": "rocprofv3 --kernel-trace --stats of --repeats 1 --no-sweep (warm round + one round: "
                                             "two calls of every variant at 1 024 pairs and at one pair)", "table": table}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def vectors(torch, seeds, duration_s, run_scale):
    """(bits DeviceBatch rows [ref, true-ratio candidate] per seed, list blocks of the same vectors, list lengths)."""
    from ffsubsync_amd import _native
    from workloads import synth

    specs = [synth.make_pair_spec(s, duration_s=duration_s, run_scale=run_scale) for s in seeds]
    db = synth.build_device_batch(specs).select_candidates([sp.true_ratio_index for sp in specs])
    n = db.offs.size
    block = (_native.runs_list_bytes(65536) + 63) // 64 * 64
    lists = torch.empty(n * block, dtype=torch.uint8, device="cuda")
    loff = (np.arange(n, dtype=np.int64) * block).reshape(db.offs.shape)
    _native.runs_from_bits_batch(db.data.data_ptr() + db.offs.ravel().astype(np.uint64), db.lens.ravel(),
                                 lists.data_ptr() + loff.ravel().astype(np.uint64), np.full(n, 65536, dtype=np.int64))
    counts = lists.view(torch.int32)[torch.from_numpy(loff.ravel() // 4).cuda()].cpu().numpy().reshape(db.offs.shape)
    assert counts.max() < 65536, "a list was truncated"
    return db, lists, loff, counts


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def measure(torch, db, lists, loff, pr, ps, repeats, algorithms=("auto",), yardsticks=True):
    """Best-of-``repeats`` ms of every variant on the pairs (pr[p], ps[p]) of the table, and whether all records agree."""
    from ffsubsync_amd import _native, match, quality

    n = pr.size
    ref_len, sub_len = db.lens[:, 0].astype(np.int64), db.lens[:, 1].astype(np.int64)
    base = np.uint64(db.data.data_ptr())
    lbase = np.uint64(lists.data_ptr())
    bits_args = (base + db.offs[pr, 0].astype(np.uint64), ref_len[pr], db.lo[pr, 0], db.hi[pr, 0],
                 base + db.offs[ps, 1].astype(np.uint64), sub_len[ps], db.lo[ps, 1], db.hi[ps, 1])
    max_samples = int(max(ref_len.max(), sub_len.max()))
    qplan = quality._get_plan(n, 2 * W, max_samples, None)
    mplan = match._get_plan(n, 2 * W, max_samples, 2 * ref_len.size, None)
    outs = {}

    def out_for(name):
        outs[name] = torch.zeros(n * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device="cuda")
        return outs[name]

    variants = {}
    for alg in algorithms:
        variants["match_" + alg] = (lambda alg=alg: mplan.report(
            lbase + loff[:, 0].astype(np.uint64), ref_len, db.lo[:, 0], db.hi[:, 0], lbase + loff[:, 1].astype(np.uint64), sub_len,
            db.lo[:, 1], db.hi[:, 1], pr, ps, W, TOP_K, E, out_for("match_" + alg), alg))
    if yardsticks:
        variants["quality_batch_bits"] = lambda: qplan.report(*bits_args, W, TOP_K, E, out_for("quality_batch_bits"))
        words = (np.stack([ref_len[pr], sub_len[ps]], axis=1) + 31) // 32
        slots = (words + 15) // 16 * 16
        starts = np.concatenate([[0], np.cumsum(slots.ravel())[:-1]]).reshape(n, 2)
        lib = _native.load()

        def from_lists():  # quality_batch's path for FFS_DTYPE_RUNS input: every vector of every pair expanded first
            scratch = qplan.scratch_words(int(slots.sum()))
            st = _native.current_stream_ptr(torch)
            ptr = np.zeros((n, 2), dtype=np.uint64)
            for p in range(n):
                for v, (idx, length) in enumerate(((pr[p], ref_len[pr[p]]), (ps[p], sub_len[ps[p]]))):
                    dst = scratch.data_ptr() + 4 * int(starts[p, v])
                    _native.check(lib.ffs_runs_to_bits(int(lbase) + int(loff[idx, v]), int(length), dst, st))
                    ptr[p, v] = dst
            a = list(bits_args)
            a[0], a[4] = ptr[:, 0], ptr[:, 1]
            qplan.report(*a, W, TOP_K, E, out_for("quality_batch_lists"))

        variants["quality_batch_lists"] = from_lists
    times = {name: [] for name in variants}
    for rnd in range(repeats + 1):
        for name, fn in variants.items():
            ms = timed(torch, fn)
            if rnd:  # round 0 warms plans and code objects
                times[name].append(ms)
    recs = {name: o.cpu().numpy().tobytes() for name, o in outs.items()}
    same = len(set(recs.values())) == 1
    entry = {"pairs": int(n), "records_identical": bool(same)}
    for name, t in times.items():
        entry[name + "_ms"] = min(t)
        entry[name + "_times_ms"] = t
        entry[name + "_us_per_pair"] = 1e3 * min(t) / n
    return entry


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_profile.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--fold-stats", default=None)
    args = ap.parse_args()
    if args.fold_stats:
        fold_stats(args.fold_stats, args.out)
        return
    import torch

    from ffsubsync_amd import match, quality

    result = {"window_samples": W, "top_k": TOP_K, "exclusion_samples": E, "device": torch.cuda.get_device_name(0),
              "data": "synthetic (workloads/synth.make_pair_spec, 7200 s); nobody has measured real files"}
    db, lists, loff, counts = vectors(torch, range(32), 7200.0, 1.0)
    result["boundaries_per_vector"] = {"reference_mean": float(counts[:, 0].mean()), "subtitle_mean": float(counts[:, 1].mean())}
    pr, ps = np.divmod(np.arange(32 * 32), 32)
    entry = measure(torch, db, lists, loff, pr, ps, args.repeats, algorithms=("auto", "runs", "bits"))
    entry["match_workspace_bytes"] = next(iter(match._plans.plans.values())).workspace_bytes
    entry["quality_workspace_bytes"] = next(iter(quality._plans.plans.values())).workspace_bytes
    entry["speedup_over_quality_batch_bits"] = entry["quality_batch_bits_ms"] / entry["match_auto_ms"]
    entry["speedup_over_quality_batch_lists"] = entry["quality_batch_lists_ms"] / entry["match_auto_ms"]
    result["pairs_1024"] = entry
    print(json.dumps({"pairs_1024": entry}), flush=True)
    one = measure(torch, db, lists, loff, np.array([0]), np.array([0]), args.repeats, algorithms=("auto",))
    result["pairs_1"] = one
    print(json.dumps({"pairs_1": one}), flush=True)
    if not args.no_sweep:
        sweep = []
        for mult in (1, 2, 4, 8, 16):
            match.clear_plan_cache()
            quality.clear_plan_cache()
            d, l, lo, c = vectors(torch, range(100, 108), 7200.0, 1.0 / mult)
            p8, s8 = np.divmod(np.arange(64), 8)
            e = measure(torch, d, l, lo, p8, s8, args.repeats, algorithms=("runs", "bits"), yardsticks=False)
            nq, npp = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
            r_len, s_len = d.lens[:, 0].astype(np.float64), d.lens[:, 1].astype(np.float64)
            # the pair's side of the FFS_MATCH_AUTO rule: word steps per coincidence, R * S / 32 / (|P| * |Q|)
            steps = (r_len[p8] * s_len[s8] / 32.0) / (nq[p8] * npp[s8])
            e.update({"density": mult, "boundaries_mean": float(c.mean()), "word_steps_per_coincidence_mean": float(steps.mean()),
                      "word_steps_per_coincidence_min": float(steps.min()), "runs_over_bits": e["match_runs_ms"] / e["match_bits_ms"]})
            sweep.append(e)
            print(json.dumps({"density_%dx" % mult: e}), flush=True)
        result["density_sweep"] = sweep
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
