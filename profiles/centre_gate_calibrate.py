"""What the centre gate does to the adaptive VAD's labels on stereo files, and its default min_contrast_bins, by rule
(DESIGN 3.28).  CPU model only (tests/stereo_vad_model.py behind tests/adaptive_vad_model.py's pick), synthetic PCM
only: no device is involved and no real file has been measured.

Data.  The 10 min "mixed" files of profiles/adaptive_vad_calibrate.py made stereo (same seeds, classes, burst levels and
music; the noise is drawn anew per channel): digital silence is zero in both channels, the noise floor is independent
in the two channels, speech is IDENTICAL in both channels plus that small independent floor, and the music stretch is
the script's three sines in both channels with inter-channel correlation rho: L = m1, R = rho m1 + sqrt(1 - rho^2) m2,
m2 the same sines a quarter period on (the same level; uncorrelated with m1 over the stretch -- within ONE 10 ms frame
the three sines beat against each other, so a frame's own correlation swings around rho, as it does in real music).
Cells:
  rho in RHOS = (0, 0.5, 0.9, 1)     the plain files; rho = 1 is centred (mono) music
  bed at -20 and -10 dB              the rho = 0 music ALSO lies under every speech frame, that far below the speech's
                                     mean level (69 dB): speech over a wide bed
Every gain of that script (0 .. -40 dB) scales the float signal before it is rounded to int16.  The threshold is picked
per file on the histogram of the mid levels with the shipped parameters of the adaptive VAD.

Per (cell, file, gain) the JSON keeps the counts of (class, active or not at the picked threshold, how many of the
candidates the frame's contrast mid - side reaches) -- everything a figure depends on, at most 48 numbers a file -- from
which tests/test_stereo_vad_host.py recomputes every figure of the table with the model's centre gate.  Per candidate c:
  music_before / music_after   share of the music frames labelled speech by the plain labels of mid / behind the gate
  speech_kept                  share of the speech frames the plain labels find that the gate keeps (None: none found)
  quiet_labelled               share of the silence and noise-floor frames labelled speech behind the gate

RULE, fixed before the numbers were produced.  Candidates c in CANDIDATES = (0, 6, 12, 18, 24) bins (half-dB steps).
DEFAULT_MIN_CONTRAST_BINS is the LARGEST candidate that, on every (cell, file, gain) where the pick finds the speech
(plain recall of speech >= 0.5), keeps at least 0.99 of the speech frames that c = 0 keeps.  If no candidate above 0
does so, 0 ships.

Limits.  Centred music (rho = 1) passes whatever c is: that is what vad="centre_steady" is for.  The data are synthetic.
5.1 input is out of scope: callers downmix to two channels.

    python profiles/centre_gate_calibrate.py [--seeds 3] > profiles/centre_gate_calibration.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]

import adaptive_vad_model as am  # noqa: E402
import stereo_vad_model as sm  # noqa: E402

CANDIDATES = (0, 6, 12, 18, 24)
RHOS = (0.0, 0.5, 0.9, 1.0)
BEDS_DB = (-20, -10)       # the bed's level against the speech's mean level
SPEECH_MEAN_DB = 69.0      # bursts of 62 .. 76 dB
DURATION = 600
FOUND = 0.5
KEEPS = 0.99
CELLS = tuple(("rho", r, None) for r in RHOS) + tuple(("bed", 0.0, b) for b in BEDS_DB)


def cell_name(cell):
    return "rho %.1f" % cell[1] if cell[0] == "rho" else "bed %d dB" % cell[2]


def stereo_class_levels(seed, silence, cell, gains):
    """(class per frame, {gain: (mid, side) uint8 levels per frame}) of one stereo file."""
    import adaptive_vad_calibrate as base

    rng = np.random.RandomState(seed)
    n_frames = DURATION * base.RATE // base.FRAME
    cls, burst = base.frame_classes(rng, n_frames, "mixed", silence)
    _, rho, bed_db = cell
    edges = am.default_edges()
    out = {g: (np.zeros(n_frames, np.uint8), np.zeros(n_frames, np.uint8)) for g in gains}
    t = np.arange(base.CHUNK_FRAMES * base.FRAME, dtype=np.float64) / base.RATE
    tones = ((220.0, 0.1), (277.2, 1.3), (329.6, 2.2))
    scale = 10.0 ** (68.0 / 20.0) / np.sqrt(1.5)
    m1 = sum(np.sin(2 * np.pi * f * t + ph) for f, ph in tones) * scale
    m2 = sum(np.cos(2 * np.pi * f * t + ph) for f, ph in tones) * scale
    shape = lambda m, k: m[:k * base.FRAME].reshape(k, base.FRAME)
    for f0 in range(0, n_frames, base.CHUNK_FRAMES):
        c = cls[f0:f0 + base.CHUNK_FRAMES]
        k = c.size
        level_db = np.where(c == 2, burst[f0:f0 + k] + rng.uniform(-8.0, 3.0, size=k), 35.0)
        centre = rng.standard_normal((k, base.FRAME)) * np.where(c == 2, 10.0 ** (level_db / 20.0), 0.0)[:, None]
        floor = rng.standard_normal((2, k, base.FRAME)) * np.where(c == 0, 0.0, 10.0 ** (35.0 / 20.0))[None, :, None]
        left, right = centre + floor[0], centre + floor[1]
        music = c == 3
        left[music] += shape(m1, k)[music]
        right[music] += (rho * shape(m1, k) + np.sqrt(1.0 - rho * rho) * shape(m2, k))[music]
        if bed_db is not None:   # the wide music under the speech, scaled from its 68 dB to bed_db below the speech's mean
            g_bed = 10.0 ** ((SPEECH_MEAN_DB + bed_db - 68.0) / 20.0)
            sp = c == 2
            left[sp] += g_bed * shape(m1, k)[sp]
            right[sp] += g_bed * shape(m2, k)[sp]
        x = np.stack([left, right], axis=2).reshape(-1)
        for g in gains:
            pcm = np.clip(np.rint(x * 10.0 ** (g / 20.0)), -32768, 32767).astype(np.int16)
            mid, side = sm.stereo_levels(pcm, base.FRAME, edges)
            out[g][0][f0:f0 + k], out[g][1][f0:f0 + k] = mid, side
    return cls, out


# the model's levels that stand for a count's cell: a threshold of BAND_T, mid above or below it, and a contrast that
# reaches exactly k of the candidates (one below the first for k = 0)
BAND_T, BAND_MID = 100, (40, 150)
REACHES = (-1,) + CANDIDATES


def encode(cls, mid, side, t):
    """Sparse counts [[class, active, candidates reached, count], ...]."""
    contrast = mid.astype(np.int64) - side.astype(np.int64)
    reached = sum((contrast >= c).astype(np.int64) for c in CANDIDATES)
    key = (cls.astype(np.int64) << 8) | ((mid.astype(np.int64) >= t).astype(np.int64) << 4) | reached
    ks, ns = np.unique(key, return_counts=True)
    return [[int(k >> 8), int((k >> 4) & 1), int(k & 15), int(n)] for k, n in zip(ks, ns)]


def figures(hist):
    """{c: the four shares} of one file from its counts, by the model's centre gate on the levels that stand for them."""
    h = np.asarray(hist, np.int64).reshape(-1, 4)
    cls, cnt = h[:, 0], h[:, 3]
    mid = np.array(BAND_MID, np.int64)[h[:, 1]]
    side = (mid - np.array(REACHES, np.int64)[h[:, 2]]).astype(np.uint8)
    mid = mid.astype(np.uint8)
    plain = am.speech(mid, BAND_T)
    share = lambda flags, members: float(cnt[flags & members].sum()) / int(cnt[members].sum()) if cnt[members].sum() else None
    out = {}
    for c in CANDIDATES:
        speech = am.speech(sm.centre_gate(mid, side, BAND_T, c)[0], BAND_T)
        out[str(c)] = dict(music_before=share(plain, cls == 3), music_after=share(speech, cls == 3),
                           speech_kept=share(speech, plain & (cls == 2)), quiet_labelled=share(speech, cls <= 1))
    return out


def with_figures(files):
    """The JSON's file entries (which keep the counts only) with their figures computed again."""
    return [dict(f, figures=figures(f["hist"])) for f in files]


def recommend(files):
    found = [f["figures"] for f in files if f["finds_speech"]]
    ok = [c for c in CANDIDATES[1:] if found and all(f[str(c)]["speech_kept"] >= KEEPS * f["0"]["speech_kept"] for f in found)]
    return max(ok) if ok else 0


def by_cell(files):
    """What DESIGN 3.28 quotes: per cell and candidate over the files (all gains) where the pick finds the speech."""
    table = []
    for cell in CELLS:
        rows = [f for f in files if f["cell"] == cell_name(cell) and f["finds_speech"]]
        line = dict(cell=cell_name(cell), files=len(rows))
        for c in CANDIDATES:
            fs = [f["figures"][str(c)] for f in rows]
            line[str(c)] = None if not fs else dict(
                music_before_min=min(x["music_before"] for x in fs), music_after=[min(x["music_after"] for x in fs), max(x["music_after"] for x in fs)],
                speech_kept_min=min(x["speech_kept"] for x in fs), quiet_labelled_max=max(x["quiet_labelled"] for x in fs))
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
    for cell in CELLS:
        for seed in range(a.seeds):
            silence = base.SILENCE_SHARES[seed % len(base.SILENCE_SHARES)]
            cls, levels = stereo_class_levels(1000 * DURATION + seed, silence, cell, base.GAINS_DB)
            for g in base.GAINS_DB:
                mid, side = levels[g]
                t = am.pick(am.level_hist(mid, 192), **pick)["threshold_bin"]
                recall = float(am.speech(mid, t)[cls == 2].mean())
                hist = encode(cls, mid, side, t)
                files.append(dict(cell=cell_name(cell), seed=seed, silence=silence, gain_db=g, threshold_bin=int(t), plain_recall=recall,
                                  finds_speech=bool(recall >= FOUND), hist=hist))
            print("%s seed %d" % (cell_name(cell), seed), file=sys.stderr)
    full = with_figures(files)
    json.dump(dict(measured="CPU model on synthetic PCM; no device, no real file", rate=base.RATE, frame_len=base.FRAME, duration=DURATION,
                   seeds=a.seeds, gains_db=list(base.GAINS_DB), candidates=list(CANDIDATES), rhos=list(RHOS), beds_db=list(BEDS_DB),
                   found=FOUND, keeps=KEEPS, shipped=dict(min_contrast_bins=recommend(full)), by_cell=by_cell(full), files=files),
              sys.stdout, separators=(",", ":"))


if __name__ == "__main__":
    main()
