"""Cost of one sampled append round, with little and with much already known, against the prefix append
 -> profiles/sampled_profile.json.

GPU script: HIP events around the device work of whole calls (no read-back), one warm call first, best of five with all
five values kept.  256 two-hour files (workloads/synth.make_pair_spec) x 7 candidates, W = 6000; every timed call feeds
6000 reference samples to all 256 files:
  1. ``ffs_prog_append_at`` at [304 000, 310 000) with 1 known interval ([0, 3000));
  2. the same call with 60 known intervals ([12 000 k, 12 000 k + 3000), k = 0 .. 59);
  3. ``ffs_prog_append`` on prefix slots of the same plan at L = 304 000, in the same process.
(The slots are opened and brought to their state before every timed call; only the last call is timed.)
The only bar: best-of-five of 2 <= the slowest of the five of 1 -- the cost of an append must not depend on what is
already known; the run's own spread is the margin.  The ratio of 1 to 3 is recorded, not barred.
  4. End to end (wall clock): ``sampled_sync`` against ``progressive_sync`` and full ingest + ``quality_sync`` on
     32 files x 90 min of PCM in pinned host memory (bench.py's end-to-end shape; profiles/progressive_profile.py makes
     the files), with the consumed fractions.  That input is synthetic noise: no bar.

    python profiles/sampled_profile.py [--files 256] [--repeats 5] [--e2e-files 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "profiles")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffsubsync_amd import _native, quality  # noqa: E402
from workloads import synth  # noqa: E402

W, SEG, TOP_K, E = 6000, 6000, 3, 300
AT, KNOWN_LEN, STRIDE, MANY = 304000, 3000, 12000, 60


def timed(prepare, fn, repeats):
    """The HIP-event times (ms) of fn() over ``repeats``, each after an untimed prepare(); one warm round first."""
    out = []
    for i in range(repeats + 1):
        prepare()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return out


def end_to_end(n_files, minutes):
    from ffsubsync_amd import progressive, sampled
    from ffsubsync_amd.speech_transformers import detect_pinned_stream
    from progressive_profile import make_files

    files, truth = make_files(n_files, minutes)
    n_frames, frame = int(minutes * 60 * 100), 480

    def reader(host):
        return lambda start, seconds: host[int(round(start * 100)) * frame:int(round((start + seconds) * 100)) * frame]

    def full():
        refs = [detect_pinned_stream(host, 100, 48000, 0.0, packed=True) for host, _ in files]
        return quality.quality_sync([(r, t) for r, (_, t) in zip(refs, files)])

    def prog():
        return progressive.progressive_sync([(progressive.pcm_label_chunks(host), t) for host, t in files])

    def samp(rule):
        return lambda: sampled.sampled_sync([(reader(host), t, minutes * 60) for host, t in files], rule)

    out = {}
    for name, fn in (("full_ingest_quality_sync", full), ("progressive_sync", prog),
                     ("sampled_sync_default_rule", samp(None)),
                     ("sampled_sync_progressive_default_rule", samp(progressive.StopRule()))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = sum(r.ratio_index == t[0] and abs(r.offset - t[1]) <= 2 for r, t in zip(res, truth))
        out[name] = {"files_per_s": n_files / dt, "recovered_ratio_and_offset": "%d/%d" % (ok, n_files)}
        if name != "full_ingest_quality_sync":
            out[name]["settled"] = "%d/%d" % (sum(r.settled for r in res), n_files)
            out[name]["mean_consumed_fraction"] = float(np.mean([r.consumed_samples / n_frames for r in res]))
    out["workload"] = "%d files x %.0f min of 48 kHz PCM in pinned host memory, seven ratios, wall clock" % (n_files, minutes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--e2e-files", type=int, default=32, help="0: skip the end-to-end reading")
    ap.add_argument("--e2e-minutes", type=float, default=90.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampled_profile.json"))
    args = ap.parse_args()
    n = args.files
    specs = [synth.make_pair_spec(seed) for seed in range(n)]
    db = synth.build_device_batch(specs)
    assert db.dtype == _native.FFS_DTYPE_U1
    nc = db.lens.shape[1] - 1
    ptr = np.uint64(db.data.data_ptr()) + db.offs.astype(np.uint64)
    lens = db.lens.astype(np.int64)
    assert int(lens[:, 0].min()) >= STRIDE * MANY and AT + SEG <= int(lens[:, 0].min())
    plan = _native.ProgPlan(n, nc, 2 * W, int(lens[:, 0].max()), int(lens[:, 1:].max()))
    cand_out = torch.empty(n * nc * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    state_out = torch.empty(n * _native.PROG_STATE_BYTES, dtype=torch.uint8, device="cuda")
    slots = np.arange(n)
    tables = (slots, np.full(n, nc), ptr[:, 1:], lens[:, 1:], db.lo[:, 1:], db.hi[:, 1:], db.lo[:, 0], db.hi[:, 0], np.full(n, W))

    def chunk_args(at, count):
        """The reference samples [at, at + count) of every file, handed over in place: word pointer and first bit."""
        return ptr[:, 0] + np.uint64(4 * (at // 32)), np.full(n, at % 32)

    def at_call(at, count):
        p, fb = chunk_args(at, count)
        plan.append_at(slots, p, fb, np.full(n, at), np.full(n, count), TOP_K, E, cand_out, state_out)

    def bring_sampled(n_known):
        plan.open_sampled(*tables, lens[:, 0])
        for k in range(n_known):
            at_call(STRIDE * k, KNOWN_LEN)

    def bring_prefix():
        plan.open(*tables)
        p, fb = chunk_args(0, AT)
        plan.append(slots, p, fb, np.full(n, AT), TOP_K, E, cand_out, state_out)

    def prefix_call():
        p, fb = chunk_args(AT, SEG)
        plan.append(slots, p, fb, np.full(n, SEG), TOP_K, E, cand_out, state_out)

    one = timed(lambda: bring_sampled(1), lambda: at_call(AT, SEG), args.repeats)
    many = timed(lambda: bring_sampled(MANY), lambda: at_call(AT, SEG), args.repeats)
    assert all(len(plan.known(s)) == MANY + 1 for s in (0, n - 1))
    prefix = timed(bring_prefix, prefix_call, args.repeats)
    out = {"what": "device work of whole calls between HIP events on one MI355X, warm, all %d timed values (ms); %d files x "
                   "%d candidates x %d new samples, W = %d, top_k = %d, E = %d" % (args.repeats, n, nc, SEG, W, TOP_K, E),
           "device": torch.cuda.get_device_name(0), "workspace_bytes": plan.workspace_bytes,
           "sampled_bytes": plan.sampled_bytes(),
           "append_at_1_known_ms": one, "append_at_60_known_ms": many, "prefix_append_ms": prefix,
           "best_60_known_ms": min(many), "slowest_1_known_ms": max(one),
           "bar_best_60_known_not_above_slowest_1_known": bool(min(many) <= max(one)),
           "ratio_append_at_to_prefix_append": min(one) / min(prefix)}
    print(json.dumps(out))
    plan.close()
    del db, cand_out, state_out
    quality.clear_plan_cache()
    torch.cuda.empty_cache()

    def write():
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")

    write()
    if args.e2e_files > 0:
        out["end_to_end"] = end_to_end(args.e2e_files, args.e2e_minutes)
        print(json.dumps(out["end_to_end"]))
        write()


if __name__ == "__main__":
    main()
