"""Cost of one progressive append round against the same records by a re-solve
-> profiles/progressive_profile.json.

GPU script: HIP events around the device work of whole calls (no read-back on either side), one warm call first, best
of several.  256 two-hour files (workloads/synth.make_pair_spec) x 7 candidates, W = 6000:
  1. ``ffs_prog_append`` of 10 000 reference samples for all 256 files at L = 10 000 and at L = 710 000 (the slots are
     opened and brought to L before every timed call; only the append of the next 10 000 samples is timed);
  2. ``ffs_align_quality_batch`` on the 1792 (prefix, candidate) pairs of the same prefixes r[0, L + 10 000): the only
     means to the same records before the progressive plan.
The only bar: reading 1 at L = 710 000 is not slower than reading 2 there.  The two readings of 1 side by side show that
the cost of an append does not grow with L.
  3. End to end (wall clock): ``progressive_sync`` with the default StopRule against full ingest + ``quality_sync`` on
     32 files x 90 min of PCM in pinned host memory (bench.py's end-to-end shape): files/s and mean consumed fraction.

    python profiles/progressive_profile.py [--files 256] [--repeats 5] [--e2e-files 32]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ffsubsync_amd import _native, quality  # noqa: E402
from ffsubsync_amd.batch import DeviceBatch  # noqa: E402
from workloads import synth  # noqa: E402

W, CHUNK, TOP_K, E = 6000, 10000, 3, 300


def timed(prepare, fn, repeats):
    """Best HIP-event time (ms) of fn() over ``repeats``, each after an untimed prepare(); one warm round first."""
    best = float("inf")
    for i in range(repeats + 1):
        prepare()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            best = min(best, a.elapsed_time(b))
    return best


def make_files(n_files, minutes):
    """([(pinned int16 PCM tensor, track)], [(true ratio index, true offset)]) of the end-to-end shape."""
    from ffsubsync_amd.constants import candidate_ratios

    ratios = candidate_ratios()
    frame, n_frames = 480, int(minutes * 60 * 100)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    files, truth = [], []
    for f in range(n_files):
        rng = np.random.RandomState(7000 + f)
        track = synth.make_subtitle_records(7000 + f, duration_s=minutes * 60 * 0.9)
        idx, shift = int(rng.randint(7)), int(rng.randint(-4000, 4000))
        act = _native.rasterize_subtitles(*track, ratios[idx], 100, 0)
        speech = torch.zeros(n_frames, dtype=torch.bool, device="cuda")
        lo, hi = max(shift, 0), min(n_frames, shift + act.numel())
        speech[lo:hi] = act[lo - shift: hi - shift] != 0
        sigma = torch.where(speech, 3000.0, 30.0).repeat_interleave(frame)
        pcm = (torch.randn(n_frames * frame, generator=g, device="cuda") * sigma).round().clamp(-32768, 32767).to(torch.int16)
        host = torch.empty(pcm.numel(), dtype=torch.int16).pin_memory()
        host.copy_(pcm)
        del pcm, sigma
        files.append((host, track))
        truth.append((idx, shift))
    return files, truth


def end_to_end(n_files, minutes):
    """Reading 3: bench.py's end-to-end shape (per file 48 kHz s16le PCM in pinned host memory whose loud frames follow
    the subtitles stretched by one of the seven ratios and shifted by a known offset).  Wall clock around whole calls,
    one warm run first: full ingest (``detect_pinned_stream``) + ``quality_sync`` against ``progressive_sync`` on
    ``pcm_label_chunks`` of the same tensors with the default StopRule."""
    import time

    from ffsubsync_amd import progressive
    from ffsubsync_amd.speech_transformers import detect_pinned_stream

    files, truth = make_files(n_files, minutes)
    n_frames = int(minutes * 60 * 100)

    def full():
        refs = [detect_pinned_stream(host, 100, 48000, 0.0, packed=True) for host, _ in files]
        return quality.quality_sync([(r, t) for r, (_, t) in zip(refs, files)])

    def prog():
        return progressive.progressive_sync([(progressive.pcm_label_chunks(host), t) for host, t in files])

    out = {}
    for name, fn in (("full_ingest_quality_sync", full), ("progressive_sync", prog)):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = sum(r.ratio_index == t[0] and abs(r.offset - t[1]) <= 2 for r, t in zip(res, truth))
        out[name] = {"files_per_s": n_files / dt, "recovered_ratio_and_offset": "%d/%d" % (ok, n_files)}
        if name == "progressive_sync":
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive_profile.json"))
    args = ap.parse_args()
    n = args.files
    specs = [synth.make_pair_spec(seed) for seed in range(n)]
    db = synth.build_device_batch(specs)
    assert db.dtype == _native.FFS_DTYPE_U1
    nc = db.lens.shape[1] - 1
    base = db.data.data_ptr()
    ptr = np.uint64(base) + db.offs.astype(np.uint64)
    lens = db.lens.astype(np.int64)
    plan = _native.ProgPlan(n, nc, 2 * W, int(lens[:, 0].max()), int(lens[:, 1:].max()))
    cand_out = torch.empty(n * nc * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    state_out = torch.empty(n * _native.PROG_STATE_BYTES, dtype=torch.uint8, device="cuda")
    slots = np.arange(n)

    def chunk_args(at, count):
        """The reference samples [at, at + count) of every file, handed over in place: word pointer and first bit."""
        return ptr[:, 0] + np.uint64(4 * (at // 32)), np.full(n, at % 32), np.full(n, count)

    def bring_to(L):
        plan.open(slots, np.full(n, nc), ptr[:, 1:], lens[:, 1:], db.lo[:, 1:], db.hi[:, 1:], db.lo[:, 0], db.hi[:, 0],
                  np.full(n, W))
        plan.append(slots, *chunk_args(0, L), TOP_K, E, cand_out, state_out)

    rows = []
    for L in (10000, 710000):
        append_ms = timed(lambda: bring_to(L),
                          lambda: plan.append(slots, *chunk_args(L, CHUNK), TOP_K, E, cand_out, state_out), args.repeats)
        prog = cand_out.cpu().numpy().copy()
        # the same records by a re-solve: one (prefix, candidate) pair per record
        pairs = n * nc
        offs = np.stack([np.repeat(db.offs[:, 0], nc), db.offs[:, 1:].reshape(-1)], axis=1)
        plens = np.stack([np.full(pairs, L + CHUNK), db.lens[:, 1:].reshape(-1)], axis=1).astype(db.lens.dtype)
        lo = np.stack([np.repeat(db.lo[:, 0], nc), db.lo[:, 1:].reshape(-1)], axis=1)
        hi = np.stack([np.repeat(db.hi[:, 0], nc), db.hi[:, 1:].reshape(-1)], axis=1)
        one = DeviceBatch(db.data, offs, plens, lo, hi, db.dtype, db.ref_dtype)
        qplan = quality._get_plan(pairs, 2 * W, int(plens.max()), None)
        out = torch.empty(pairs * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device="cuda")
        resolve_ms = timed(lambda: None, lambda: qplan.report(*one.pair_arrays(), W, TOP_K, E, out), args.repeats)
        same = bool((out.cpu().numpy() == prog).all())
        rows.append({"L": L, "files": n, "candidates": nc, "new_samples": CHUNK, "append_ms": append_ms,
                     "resolve_ms": resolve_ms, "records_identical": same, "append_not_slower": bool(append_ms <= resolve_ms)})
        print(json.dumps(rows[-1]))
    out = {"what": "device work of whole calls between HIP events on one MI355X, warm, best of %d; W = %d, top_k = %d, "
                   "E = %d" % (args.repeats, W, TOP_K, E),
           "device": torch.cuda.get_device_name(0), "workspace_bytes": plan.workspace_bytes, "rows": rows}
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
