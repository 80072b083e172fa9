"""What the steady-run gate does to the adaptive VAD's labels, and its default dip_bins, by rule.  CPU model
only (tests/steady_gate_model.py behind tests/adaptive_vad_model.py's pick), synthetic PCM only: no device is involved
and no real file has been measured.

Data.  The 10 min "mixed" files of profiles/adaptive_vad_calibrate.py (same seeds, so the same PCM: digital silence, a
noise floor, speech bursts, one steady music stretch of a tenth of the file) at every gain of that script, the threshold
picked per file with the shipped parameters of the adaptive VAD.  The synthetic speech has NO pauses inside a burst and
bursts abut the music and each other, so it forms stretches longer than real speech would: the speech kept here is a
lower bound of a kind, not an estimate.  max_run is the reference's longest cue, 10 s of frames.

Per (file, gain), for every dip_bins of DIPS:
  music_before / music_after   share of the music frames labelled speech by the plain labels / behind the gate
  speech_kept                  share of the speech frames the plain labels find that the gate keeps (None: none found)
  quiet_labelled               share of the silence and noise-floor frames labelled speech behind the gate
The JSON keeps each file as run-length coded (band, class) symbols -- band 2: level >= t, band 1: t - max(DIPS) <= level
< t, band 0: below -- from which tests/test_steady_gate_host.py recomputes every figure with the model.

RULE, fixed before the numbers were produced.  dip_bins = 0 rejects the least (for fixed t and max_run the kept set only
shrinks as dip_bins grows), so it ships UNLESS a larger value of DIPS, on every file where the pick finds the speech
(plain recall of speech >= 0.5), keeps at least 0.99 of the speech that dip_bins = 0 keeps AND lowers the music share
behind the gate on at least one such file; then the smallest such value is recommended.

    python profiles/steady_gate_calibrate.py [--seeds 3] > profiles/steady_gate_calibration.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

import adaptive_vad_model as am  # noqa: E402
import steady_gate_model as gm  # noqa: E402

DIPS = (0, 10)
MAX_RUN = 1000   # DEFAULT_MAX_SUBTITLE_SECONDS * 100 frames per second
DURATION = 600
FOUND = 0.5
KEEPS = 0.99
# the model's levels of the three bands around a threshold of 100 with DIPS[-1] = 10
BAND_LEVEL, BAND_T = (10, 95, 120), 100


def encode(cls, levels, t):
    """[[symbol, length], ...]: symbol = 4 * band + class."""
    lv = levels.astype(np.int64)
    sym = 4 * ((lv >= t).astype(np.int64) + (lv >= t - DIPS[-1])) + cls
    cut = np.flatnonzero(np.diff(sym)) + 1
    starts = np.concatenate([[0], cut])
    return [[int(sym[s]), int(n)] for s, n in zip(starts, np.diff(np.concatenate([starts, [sym.size]])))]


def decode(runs):
    sym = np.repeat(np.array([s for s, _ in runs], np.int64), np.array([n for _, n in runs], np.int64))
    return sym % 4, np.array(BAND_LEVEL, np.uint8)[sym // 4]


def figures(runs, max_run):
    """{dip: the four shares} of one file from its run-length code, by the model."""
    cls, lv = decode(runs)
    plain = gm.classes(lv, BAND_T, 0)[0]
    share = lambda flags, members: float(flags[members].sum()) / int(members.sum()) if members.any() else None
    out = {}
    for dip in DIPS:
        speech = gm.gate_vectorised(lv, BAND_T, dip, max_run)[0]
        found = plain & (cls == 2)
        out[str(dip)] = dict(music_before=share(plain, cls == 3), music_after=share(speech, cls == 3),
                             speech_kept=share(speech, found), quiet_labelled=share(speech, cls <= 1))
    return out


def recommend(files):
    found = [f for f in files if f["finds_speech"]]
    for dip in DIPS[1:]:
        a = [(f["figures"]["0"], f["figures"][str(dip)]) for f in found]
        if a and all(d["speech_kept"] >= KEEPS * z["speech_kept"] for z, d in a) and any(d["music_after"] < z["music_after"] for z, d in a):
            return dip
    return 0


def by_gain(files):
    """What DESIGN 3.27 quotes: per gain and dip over the files where the pick finds the speech."""
    table = []
    for g in sorted({f["gain_db"] for f in files}, reverse=True):
        rows = [f for f in files if f["gain_db"] == g and f["finds_speech"]]
        line = dict(gain_db=g, files=len(rows))
        for dip in DIPS:
            fs = [f["figures"][str(dip)] for f in rows]
            line[str(dip)] = None if not fs else dict(
                music_before_min=min(x["music_before"] for x in fs), music_after_max=max(x["music_after"] for x in fs),
                speech_kept=[min(x["speech_kept"] for x in fs), max(x["speech_kept"] for x in fs)],
                quiet_labelled_max=max(x["quiet_labelled"] for x in fs))
        table.append(line)
    return table


def main():
    import adaptive_vad_calibrate as base
    from ffsubsync_amd import adaptive_vad as av

    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    a = ap.parse_args()
    pick = dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, fallback_bin=100,
                floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)
    files = []
    for seed in range(a.seeds):
        silence = base.SILENCE_SHARES[seed % len(base.SILENCE_SHARES)]
        cls, levels = base.class_levels(1000 * DURATION + seed, DURATION, "mixed", silence)
        for g in base.GAINS_DB:
            t = am.pick(am.level_hist(levels[g], 192), **pick)["threshold_bin"]
            runs = encode(cls, levels[g], t)
            plain = levels[g].astype(np.int64) >= t
            recall = float(plain[cls == 2].mean())
            files.append(dict(seed=seed, silence=silence, gain_db=g, threshold_bin=int(t), plain_recall=recall,
                              finds_speech=bool(recall >= FOUND), runs=runs, figures=figures(runs, MAX_RUN)))
        print("seed %d" % seed, file=sys.stderr)
    json.dump(dict(rate=base.RATE, frame_len=base.FRAME, duration=DURATION, seeds=a.seeds, dips=list(DIPS), max_run=MAX_RUN,
                   found=FOUND, keeps=KEEPS, shipped=dict(dip_bins=recommend(files), max_run=MAX_RUN), by_gain=by_gain(files),
                   files=files), sys.stdout, separators=(",", ":"))


if __name__ == "__main__":
    main()
