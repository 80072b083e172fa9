#!/usr/bin/env python
"""The stereo level sweep beside the mono sweep it is modelled on, and the centre gate beside the plain labels (DESIGN
3.28): a 2 h stereo file at 48 kHz (345.6 M pairs, 1.38 GB) resident in HBM, 10 ms frames of 480 pairs.

The parent starts ONE fresh child under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, no other
tracing) under a time limit.  The child queues, after a warm-up, CALLS calls of ffs_vad_stereo_levels on the buffer and
CALLS of ffs_vad_levels on THE SAME BYTES taken as mono PCM in frames of 480 samples -- both read every byte once and
make one wave reduction per 960 bytes -- then GATE_CALLS calls of ffs_vad_centre_gate (its memset, k_centre_gate and
k_centre_finish) and of ffs_vad_level_labels (fp32 labels) on the file's 720 000 levels, and times all four with HIP
events as well.  The parent reads the kernel statistics and reports bytes per second of both sweeps and their ratio,
and the gate's two launches against k_vad_level_labels.  No rate is fixed in advance.

    python profiles/stereo_vad_bench.py > profiles/stereo_vad_bench.json
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE, SECONDS, FRAME = 48000, 7200, 480
N_PAIRS = RATE * SECONDS
N_FRAMES = N_PAIRS // FRAME
CALLS, WARMUP = 20, 5
GATE_CALLS, GATE_WARMUP = 200, 20
KERNELS = ("k_vad_stereo_levels", "k_vad_levels", "k_centre_gate", "k_centre_finish", "k_vad_level_labels")
LIMIT_S = 420


def child():
    import torch

    from ffsubsync_amd import _native, adaptive_vad

    lib = _native.load()
    # centred "speech" in bursts over an independent floor, in pieces (the whole file at once would need twice the memory)
    pcm = torch.empty(2 * N_PAIRS, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    piece = 60 * RATE
    for o in range(0, N_PAIRS, piece):
        common = torch.randint(-6000, 6001, (piece,), dtype=torch.int16, device="cuda", generator=gen)
        if (o // piece) % 3 == 2:   # every third minute is wide: the channels are independent
            common = common >> 8
        own = torch.randint(-3000 if (o // piece) % 3 == 2 else -40, 3001 if (o // piece) % 3 == 2 else 41, (piece, 2), dtype=torch.int16,
                            device="cuda", generator=gen)
        pcm[2 * o:2 * (o + piece)] = (own + common[:, None]).reshape(-1)
    edges = adaptive_vad._edges_dev(None, pcm.device)
    mid = torch.empty(N_FRAMES, dtype=torch.uint8, device="cuda")
    side = torch.empty(N_FRAMES, dtype=torch.uint8, device="cuda")
    mono = torch.empty(2 * N_FRAMES, dtype=torch.uint8, device="cuda")
    out = torch.empty(N_FRAMES, dtype=torch.uint8, device="cuda")
    labels = torch.empty(N_FRAMES, dtype=torch.float32, device="cuda")
    record = torch.empty(48, dtype=torch.uint8, device="cuda")
    stream = _native.current_stream_ptr(torch)
    stereo = lambda: _native.check(lib.ffs_vad_stereo_levels(pcm.data_ptr(), N_PAIRS, FRAME, edges.data_ptr(), 191, mid.data_ptr(),
                                                            side.data_ptr(), stream))
    plain = lambda: _native.check(lib.ffs_vad_levels(pcm.data_ptr(), 2 * N_PAIRS, FRAME, edges.data_ptr(), 191, mono.data_ptr(), stream))
    gate = lambda: _native.check(lib.ffs_vad_centre_gate(mid.data_ptr(), side.data_ptr(), N_FRAMES, None, 100, 12, out.data_ptr(),
                                                         record.data_ptr(), stream))
    label = lambda: _native.check(lib.ffs_vad_level_labels(mid.data_ptr(), N_FRAMES, None, 100, 0.0, labels.data_ptr(), None, stream))
    res = {}
    for name, fn, calls, warm in (("stereo_levels", stereo, CALLS, WARMUP), ("mono_levels", plain, CALLS, WARMUP),
                                  ("centre_gate", gate, GATE_CALLS, GATE_WARMUP), ("level_labels", label, GATE_CALLS, GATE_WARMUP)):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        res[name + "_event_us_per_call"] = a.elapsed_time(b) * 1000.0 / calls
    rec = adaptive_vad.centre_record_of(record.cpu().numpy().view(_native.VAD_CENTRE_DTYPE)[0])
    res["record"] = rec.__dict__
    res["mid_levels"] = [int(mid.min()), int(mid.max())]
    res["side_levels"] = [int(side.min()), int(side.max())]
    print("CHILD " + json.dumps(res))


def kernel_stats(directory):
    """{kernel: (calls, average ns)} from rocprofv3's kernel statistics CSV."""
    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            low = {k.lower(): v for k, v in row.items()}
            name = low.get("name", "")
            for k in KERNELS:
                if k in name:   # no name holds another
                    found[k] = (int(low["calls"]), float(low["averagens"]))
    return found


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        return child()
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                               "run"], capture_output=True, text=True, timeout=LIMIT_S)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")]
        if done.returncode != 0 or not lines:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-2000:])
            raise SystemExit("the profiled child failed (exit %d)" % done.returncode)
        stats = kernel_stats(tmp)
    out = {"measured": "MI355X, rocprofv3 --kernel-trace --stats, a run of its own", "rate": RATE, "seconds": SECONDS, "frame_len_pairs": FRAME,
           "n_pairs": N_PAIRS, "bytes": 4 * N_PAIRS, "n_frames": N_FRAMES, "calls": CALLS, "gate_calls": GATE_CALLS}
    out.update(json.loads(lines[0][6:]))
    for k in KERNELS:
        if k in stats:
            out[k] = {"calls": stats[k][0], "average_us": stats[k][1] / 1000.0}
    if "k_vad_stereo_levels" in stats and "k_vad_levels" in stats:
        s, m = stats["k_vad_stereo_levels"][1], stats["k_vad_levels"][1]
        out["stereo_bytes_per_s"] = 4 * N_PAIRS / (s * 1e-9)
        out["mono_bytes_per_s"] = 4 * N_PAIRS / (m * 1e-9)
        out["ratio_stereo_to_mono_bytes_per_s"] = m / s
    if all(k in stats for k in KERNELS[2:]):
        g = (stats["k_centre_gate"][1] + stats["k_centre_finish"][1]) / 1000.0
        out["gate_two_launches_us"] = g
        out["ratio_gate_to_level_labels"] = g / (stats["k_vad_level_labels"][1] / 1000.0)
    if not all(k in stats for k in KERNELS):
        out["note"] = "some kernel statistics not found in the profiler's output: event timings stand in"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
