#!/usr/bin/env python
"""The adaptive energy VAD beside the sweep it was modelled on: the 90-minute 48 kHz s16le buffer of the VAD
headline (259.2 M samples, 518 MB) resident in HBM, HIP-event timing.

ffs_vad_energy_bits (the existing sweep) and ffs_vad_levels (pass 1) alternate in ONE process: each round times REPS
launches of one, then REPS of the other, after a warm-up; the medians over the rounds and their spread are reported, and
the ratio levels / energy_bits.  Then the three small kernels on the file's 540 000 level bytes and the whole
detect_device_adaptive (four launches and the 48-byte read-back).

    python profiles/adaptive_vad_bench.py > profiles/adaptive_vad_bench.json
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from ffsubsync_amd import _native, adaptive_vad  # noqa: E402

N, FRAME = 259200000, 480
REPS, ROUNDS = 300, 7   # 300 launches of ~0.1 ms a side per round, seven rounds: about a third of a second in all


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "rounds": len(ms)}


def main():
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    pcm = (torch.randn(N, device="cuda", generator=g) * 3000).to(torch.int16)
    n_frames = N // FRAME
    words = torch.zeros((n_frames + 31) // 32, dtype=torch.int32, device="cuda")
    levels = torch.empty(n_frames, dtype=torch.uint8, device="cuda")
    sweeps = {"energy_bits": lambda: _native.vad_energy_bits(pcm, FRAME, 50.0, out=words),
              "levels": lambda: adaptive_vad.frame_levels(pcm, FRAME, out=levels)}
    for fn in sweeps.values():   # warm-up: the default edge table is uploaded here
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in sweeps}
    for _ in range(ROUNDS):
        for name, fn in sweeps.items():
            ms[name].append(timed(fn, REPS))
    out = {"samples": N, "frame_len": FRAME, "n_frames": n_frames, "reps": REPS}
    for name in sweeps:
        out[name] = summary(ms[name])
    moved = 2 * N + n_frames   # the PCM once and a level byte per frame
    out["levels"]["bytes"] = moved
    out["levels"]["GBps"] = moved / out["levels"]["ms_median"] / 1e6
    out["energy_bits"]["GBps"] = (2 * N + n_frames // 8) / out["energy_bits"]["ms_median"] / 1e6
    out["ratio_levels_to_energy_bits"] = out["levels"]["ms_median"] / out["energy_bits"]["ms_median"]
    out["ratio_per_round"] = [a / b for a, b in zip(ms["levels"], ms["energy_bits"])]
    # the three small kernels on this file's levels
    hist = torch.empty(192, dtype=torch.int32, device="cuda")
    raw = adaptive_vad.pick_threshold_device(adaptive_vad.level_hist(levels, out=hist))
    small = {"level_hist": lambda: adaptive_vad.level_hist(levels, out=hist),
             "pick_threshold": lambda: adaptive_vad.pick_threshold_device(hist, out=raw),
             "level_labels_bits": lambda: adaptive_vad.level_labels(levels, raw, packed=True),
             "level_labels_f32": lambda: adaptive_vad.level_labels(levels, raw)}
    for name, fn in small.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = summary([timed(fn, 200) for _ in range(5)])
    whole = lambda: adaptive_vad.detect_device_adaptive(pcm, 100, 48000, 0.0, packed=True)
    whole()
    out["detect_device_adaptive"] = summary([timed(whole, 10) for _ in range(5)])
    _, rec = whole()
    out["record"] = rec.__dict__
    # the tie to the existing kernel on this very buffer
    bits = adaptive_vad.level_labels(levels, 100, packed=True).bits
    _native.vad_energy_bits(pcm, FRAME, 50.0, out=words)
    out["labels_at_bin_100_equal_energy_bits"] = bool(torch.equal(bits, words))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
