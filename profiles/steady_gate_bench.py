#!/usr/bin/env python
"""The steady-run gate beside the plain labels it replaces: the 720 000 level bytes of a 2 h file at 100
frames per second, resident in HBM, the packed form the aligner reads.

The parent starts ONE fresh child under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, no other
tracing).  The child queues CALLS calls of ffs_vad_steady_gate (k_gate_tiles, k_gate_carry, k_gate_labels) and CALLS of
ffs_vad_level_labels (k_vad_level_labels, the path without the gate) on the same levels after a warm-up, and times both
with HIP events as well.  The parent reads the kernel statistics and reports per kernel the average duration, the sum
of the gate's three, and its ratio to k_vad_level_labels.  No target is fixed; the figure to put it against is the PCM
sweep's 75 us per 90-minute file, which the gate should not rival.

    python profiles/steady_gate_bench.py > profiles/steady_gate_bench.json
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

N_FRAMES = 720000
MAX_RUN = 1000
CALLS, WARMUP = 200, 20
KERNELS = ("k_gate_tiles", "k_gate_carry", "k_gate_labels", "k_vad_level_labels")


def levels_of_a_film(n):
    """Level bytes shaped like a film's: a floor near bin 40, speech bursts of 0.3 .. 6 s with pauses, one music stretch
    of five minutes, all above a threshold of 100."""
    import numpy as np

    rng = np.random.RandomState(7)
    lv = rng.randint(30, 50, size=n).astype(np.uint8)
    f = 100
    while f < n - 1000:
        ln = int(rng.randint(30, 600))
        lv[f:f + ln] = rng.randint(110, 150, size=ln)
        f += ln + int(rng.randint(20, 400))
    lv[300000:330000] = 135
    return lv


def child():
    import torch

    from ffsubsync_amd import _native, adaptive_vad

    lib = _native.load()
    levels = torch.from_numpy(levels_of_a_film(N_FRAMES)).cuda()
    bits_a = torch.zeros((N_FRAMES + 31) // 32, dtype=torch.int32, device="cuda")
    bits_b = torch.zeros_like(bits_a)
    record = torch.empty(48, dtype=torch.uint8, device="cuda")
    ws_bytes = int(lib.ffs_vad_steady_gate_workspace_bytes(N_FRAMES))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    stream = _native.current_stream_ptr(torch)
    gate = lambda: _native.check(lib.ffs_vad_steady_gate(levels.data_ptr(), N_FRAMES, None, 100, 0, MAX_RUN, 0.0, None, bits_a.data_ptr(),
                                                         record.data_ptr(), ws.data_ptr(), ws_bytes, stream))
    plain = lambda: _native.check(lib.ffs_vad_level_labels(levels.data_ptr(), N_FRAMES, None, 100, 0.0, None, bits_b.data_ptr(), stream))
    out = {}
    for name, fn in (("steady_gate", gate), ("level_labels", plain)):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out[name + "_event_us_per_call"] = a.elapsed_time(b) * 1000.0 / CALLS
    rec = adaptive_vad.gate_record_of(record.cpu().numpy().view(_native.VAD_GATE_DTYPE)[0])
    out["record"] = rec.__dict__
    import numpy as np

    dropped = int(np.unpackbits((bits_a ^ bits_b).cpu().numpy().view(np.uint8)).sum())   # plain labels the gate took away
    out["frames_dropped"] = dropped
    out["dropped_equals_record"] = dropped == rec.n_active - rec.n_kept
    print("CHILD " + json.dumps(out))


def kernel_stats(directory):
    """{kernel: (calls, average ns)} from rocprofv3's kernel statistics CSV."""
    found = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            low = {k.lower(): v for k, v in row.items()}
            name = low.get("name", "")
            for k in KERNELS:
                if k in name:
                    found[k] = (int(low["calls"]), float(low["averagens"]))
    return found


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        return child()
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                               "run"], capture_output=True, text=True, timeout=300)
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("CHILD ")]
        if done.returncode != 0 or not lines:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-2000:])
            raise SystemExit("the profiled child failed (exit %d)" % done.returncode)
        stats = kernel_stats(tmp)
    out = {"n_frames": N_FRAMES, "max_run": MAX_RUN, "dip_bins": 0, "calls": CALLS, "warmup": WARMUP, "form": "packed bits",
           "tool": "rocprofv3 --kernel-trace --stats"}
    out.update(json.loads(lines[0][6:]))
    for k in KERNELS:
        if k in stats:
            out[k] = {"calls": stats[k][0], "average_us": stats[k][1] / 1000.0}
    if all(k in stats for k in KERNELS):
        gate = sum(stats[k][1] for k in KERNELS[:3]) / 1000.0
        out["gate_three_kernels_us"] = gate
        out["ratio_gate_to_level_labels"] = gate / (stats[KERNELS[3]][1] / 1000.0)
    else:
        out["note"] = "kernel statistics not found in the profiler's output: event timings only"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
