"""The defaults of the adaptive energy VAD, by rule.  CPU model only (tests/adaptive_vad_model.py), synthetic
PCM only: no device is involved and no real file has been measured.

Data.  16 kHz mono s16 PCM in 10 ms frames, built per file from a class per frame: digital silence (exact zeros), a
noise floor (35 dB mean square at gain 0), speech bursts (each burst at its own level of 62 .. 76 dB, every frame
modulated by -8 .. +3 dB) and one music stretch (three sines, 68 dB, steady).  The float signal is scaled by the gain
(0, -10, -20, -30, -40 dB) BEFORE it is rounded to int16, as a quieter recording would be.  Kinds: "mixed" (all four
classes; 10 min and 1 h) and "no_speech" (silence and noise floor only: a file on which any threshold is meaningless).
The share of digital silence cycles with the seed through 0, 12 and 40 % of the runs (SILENCE_SHARES).
Per (file, gain) the JSON keeps the level histogram of every class, sparse, so every figure below can be recomputed
from it for any parameters (tests/test_adaptive_vad_host.py does, with the model's pick).

Error of a pick on a file: (share of speech frames missed + share of silence and noise-floor frames labelled speech) / 2.
Music frames are left out of it and reported on their own: an energy rule labels loud music as speech.

RULES, fixed before the numbers were seen.  (The data were widened once after a first run: every file then had 12 %
silence, which never exercised what lo_bin is for; the shares of 0 and 40 % were added, the rules were left alone.)
  lo_bin       of {0, 1, 10, 20}: the value with the smallest worst error over all mixed files and gains under the Otsu
               rule; among equals the one nearest 20 (the starting point).
  floor_ppm, margin_bins   of {50000, 100000, 200000} x {10, 20, 30}: the pair with the smallest worst error under the
               floor rule at that lo_bin; among equals the smaller margin, then the smaller floor_ppm.
  rule         the one with the smaller worst error at those parameters; Otsu when equal.
  min_eta      Otsu at those parameters: the midpoint, rounded to 0.01, between the smallest eta of a mixed file whose
               error is at most 0.05 and the largest eta of a no_speech file, if the former exceeds the latter; else no
               bound is shipped and assess() reports eta only when the caller passes one.

    python profiles/adaptive_vad_calibrate.py [--seeds 6] > profiles/adaptive_vad_calibration.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adaptive_vad_model as am  # noqa: E402

RATE, FRAME = 16000, 160
GAINS_DB = (0, -10, -20, -30, -40)
DURATIONS = (600, 3600)
CLASSES = ("silence", "noise", "speech", "music")
LO_BINS = (0, 1, 10, 20)
FLOOR_PPM = (50000, 100000, 200000)
MARGINS = (10, 20, 30)
GOOD_ERROR = 0.05
CHUNK_FRAMES = 10000
SILENCE_SHARES = (0.0, 0.12, 0.4)


def frame_classes(rng, n_frames, kind, silence):
    """A class per frame in runs: silence 0, noise 1, speech 2, music 3 (one stretch of a tenth of the file)."""
    runs = np.maximum(1, rng.geometric(1.0 / 150.0, size=n_frames // 50 + 8))
    p = [silence, 0.6 - silence, 0.4] if kind == "mixed" else [silence, 1.0 - silence, 0.0]
    cls = np.repeat(rng.choice(3, size=runs.size, p=p), runs)[:n_frames]
    burst = np.repeat(rng.uniform(62.0, 76.0, size=runs.size), runs)[:n_frames]
    if kind == "mixed":
        m0 = int(rng.randint(0, n_frames - n_frames // 10))
        cls[m0:m0 + n_frames // 10] = 3
    return cls, burst


def class_histograms(seed, duration, kind, silence):
    """{gain: int64 [4, 192]} of one file: the level counts of every class at every gain."""
    cls, levels = class_levels(seed, duration, kind, silence)
    return {g: np.stack([np.bincount(levels[g][cls == k], minlength=192) for k in range(4)]).astype(np.int64) for g in GAINS_DB}


def class_levels(seed, duration, kind, silence, gains=GAINS_DB):
    """(class per frame, {gain: uint8 level per frame}) of one file, frame by frame (profiles/steady_gate_calibrate.py
    needs the order of the frames, not only their counts)."""
    rng = np.random.RandomState(seed)
    n_frames = duration * RATE // FRAME
    cls, burst = frame_classes(rng, n_frames, kind, silence)
    edges = am.default_edges()
    out = {g: np.zeros(n_frames, np.uint8) for g in gains}
    t = np.arange(CHUNK_FRAMES * FRAME, dtype=np.float64) / RATE
    music = sum(np.sin(2 * np.pi * f * t + ph) for f, ph in ((220.0, 0.1), (277.2, 1.3), (329.6, 2.2)))
    music *= 10.0 ** (68.0 / 20.0) / np.sqrt(1.5)
    for f0 in range(0, n_frames, CHUNK_FRAMES):
        c = cls[f0:f0 + CHUNK_FRAMES]
        level_db = np.where(c == 2, burst[f0:f0 + CHUNK_FRAMES] + rng.uniform(-8.0, 3.0, size=c.size), 35.0)
        sigma = np.where(c == 0, 0.0, 10.0 ** (level_db / 20.0))
        sigma[c == 3] = 10.0 ** (35.0 / 20.0)  # the noise floor under the music
        x = rng.standard_normal((c.size, FRAME)) * sigma[:, None]
        x[c == 3] += music[:c.size * FRAME].reshape(c.size, FRAME)[c == 3]
        for g in gains:
            pcm = np.clip(np.rint(x * 10.0 ** (g / 20.0)), -32768, 32767).astype(np.int16).ravel()
            out[g][f0:f0 + c.size] = am.frame_levels(pcm, FRAME, edges)
    return cls, out


def evaluate(class_hist, **pick_args):
    """(error, share of music frames labelled speech, record) of one pick on one file's class histograms."""
    h = np.asarray(class_hist, np.int64)
    rec = am.pick(h.sum(axis=0), **pick_args)
    above = h[:, rec["threshold_bin"]:].sum(axis=1)
    n = h.sum(axis=1)
    miss = 1.0 - above[2] / n[2] if n[2] else 0.0
    quiet = n[0] + n[1]
    false = (above[0] + above[1]) / quiet if quiet else 0.0
    return (miss + false) / 2.0, (above[3] / n[3] if n[3] else None), rec


def derive(files):
    """The shipped values from the files' class histograms, by the rules of the module docstring."""
    mixed = [f for f in files if f["kind"] == "mixed"]
    dense = lambda f: sparse_to_dense(f["class_hist"])
    worst = lambda **a: max(evaluate(dense(f), **a)[0] for f in mixed)
    otsu = {lo: worst(rule=am.OTSU, lo_bin=lo, t_min=lo + 1) for lo in LO_BINS}
    lo_bin = min(LO_BINS, key=lambda lo: (otsu[lo], abs(lo - 20)))
    floor = {(m, p): worst(rule=am.FLOOR, lo_bin=lo_bin, t_min=lo_bin + 1, floor_ppm=p, margin_bins=m) for m in MARGINS for p in FLOOR_PPM}
    margin, ppm = min(floor, key=lambda k: (floor[k], k))
    rule = "otsu" if otsu[lo_bin] <= floor[(margin, ppm)] else "floor"
    args = dict(rule=am.OTSU, lo_bin=lo_bin, t_min=lo_bin + 1)
    good = [r["eta"] for e, _, r in (evaluate(dense(f), **args) for f in mixed) if e <= GOOD_ERROR and not r["flags"] & am.FALLBACK]
    bad = [evaluate(dense(f), **args)[2]["eta"] for f in files if f["kind"] == "no_speech"]
    separate = bool(good) and bool(bad) and min(good) > max(bad)
    return dict(rule=rule, lo_bin=lo_bin, floor_ppm=ppm, margin_bins=margin, otsu_worst_error={str(k): v for k, v in otsu.items()},
                floor_worst_error={"%d,%d" % k: v for k, v in floor.items()}, eta_good_min=min(good) if good else None,
                eta_no_speech_max=max(bad) if bad else None, separate=separate,
                min_eta=round((min(good) + max(bad)) / 2.0, 2) if separate else None)


def dense_to_sparse(h):
    return [[[int(b), int(x)] for b, x in enumerate(row) if x] for row in h]


def sparse_to_dense(s, n_bins=192):
    h = np.zeros((len(s), n_bins), np.int64)
    for k, row in enumerate(s):
        for b, x in row:
            h[k, b] = x
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=6)
    a = ap.parse_args()
    files = []
    for duration in DURATIONS:
        for kind in ("mixed", "no_speech"):
            for seed in range(a.seeds if duration == 600 else max(a.seeds // 2, 1)):
                silence = SILENCE_SHARES[seed % len(SILENCE_SHARES)]
                hists = class_histograms(1000 * duration + seed + (500 if kind == "no_speech" else 0), duration, kind, silence)
                for g in GAINS_DB:
                    files.append(dict(duration=duration, kind=kind, seed=seed, silence=silence, gain_db=g,
                                      class_hist=dense_to_sparse(hists[g])))
                print("%s %d s seed %d" % (kind, duration, seed), file=sys.stderr)
    shipped = derive(files)
    table = []   # what DESIGN 3.26 quotes: per gain, the fixed rule beside the shipped parameters of either rule
    for g in GAINS_DB:
        rows = [f for f in files if f["kind"] == "mixed" and f["gain_db"] == g]
        line = dict(gain_db=g)
        for name, args in (("fixed", None), ("otsu", dict(rule=am.OTSU)), ("floor", dict(rule=am.FLOOR, floor_ppm=shipped["floor_ppm"],
                                                                                         margin_bins=shipped["margin_bins"]))):
            recall, false, music, thr = [], [], [], []
            for f in rows:
                h = sparse_to_dense(f["class_hist"])
                t = 100 if args is None else evaluate(h, lo_bin=shipped["lo_bin"], t_min=shipped["lo_bin"] + 1, **args)[2]["threshold_bin"]
                above, n = h[:, t:].sum(axis=1), h.sum(axis=1)
                recall.append(above[2] / n[2])
                false.append((above[0] + above[1]) / max(n[0] + n[1], 1))
                music.append(above[3] / n[3])
                thr.append(t)
            line[name] = dict(recall_min=min(recall), false_max=max(false), music_min=min(music), threshold_bin=[min(thr), max(thr)])
        table.append(line)
    json.dump(dict(rate=RATE, frame_len=FRAME, gains_db=list(GAINS_DB), durations=list(DURATIONS), classes=list(CLASSES),
                   lo_bins=list(LO_BINS), floor_ppm=list(FLOOR_PPM), margins=list(MARGINS), good_error=GOOD_ERROR, seeds=a.seeds, silence_shares=list(SILENCE_SHARES),
                   shipped=shipped, by_gain=table, files=files), sys.stdout, separators=(",", ":"))


if __name__ == "__main__":
    main()
