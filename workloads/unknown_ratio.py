"""Seeded problems whose speed factor is NOT one of the seven framerate ratios: what ``ratio_sweep`` is for.

A problem is (reference, track): the track a seeded subtitle file (``synth.make_subtitle_records``), the reference a 0/1
activity vector at 100 Hz of the same cues on the clock ``t * true_ratio + TRUE_OFFSET_S``, 15 % of them dropped and every
edge moved by up to +-0.1 s -- a speech detector that mostly agrees with the subtitles.  Classes:

    free   true ratio U[0.92, 1.08], rounded to 1e-4 and at least 2e-3 away from every one of the seven
    seven  true ratio is one of the seven (seed picks which)
    wrong  the reference of ``seed`` against the track of another seed (nothing to find)
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE, candidate_ratios

from . import synth

TRUE_OFFSET_S = 12.34
CLASSES = ("free", "seven", "wrong")
_OTHER_SEED = 50021  # `wrong`: the track is that of seed + _OTHER_SEED


@dataclass
class UnknownRatioProblem:
    kind: str
    seed: int
    true_ratio: float  # reference clock = track clock * true_ratio + TRUE_OFFSET_S (nan for `wrong`)
    true_offset_samples: int
    reference: np.ndarray  # 0/1 float64
    track: Tuple[np.ndarray, np.ndarray, np.ndarray]  # (start_us, end_us, is_metadata)

    @property
    def problem(self):
        """(reference, track), as ``ratio_sweep.sweep_sync`` and every ``*_sync`` take it."""
        return self.reference, self.track


def true_ratio(kind: str, seed: int) -> float:
    rng = np.random.RandomState(seed + 9176)
    seven = candidate_ratios()
    if kind == "seven":
        return float(seven[int(rng.randint(len(seven)))])
    while True:
        r = float(np.round(rng.uniform(0.92, 1.08), 4))
        if min(abs(r - s) for s in seven) >= 2e-3:
            return r


def make_problem(kind: str, seed: int, duration_s: float = 600.0, sample_rate: int = SAMPLE_RATE) -> UnknownRatioProblem:
    if kind not in CLASSES:
        raise ValueError("kind=%r: expected one of %s" % (kind, ", ".join(CLASSES)))
    start_us, end_us, meta = synth.make_subtitle_records(seed, duration_s)
    ratio = true_ratio("free" if kind == "wrong" else kind, seed)
    rng = np.random.RandomState(seed + 31337)
    keep = rng.rand(start_us.size) > 0.15
    js = rng.uniform(-0.1, 0.1, start_us.size)
    je = rng.uniform(-0.1, 0.1, start_us.size)
    t0 = start_us / 1e6 * ratio + TRUE_OFFSET_S + js
    t1 = end_us / 1e6 * ratio + TRUE_OFFSET_S + je
    ok = keep & (t1 > t0)
    n = int((end_us.max() / 1e6 * ratio + TRUE_OFFSET_S) * sample_rate) + 2
    st = np.rint(t0[ok] * sample_rate).astype(np.int64)
    en = st + np.rint((t1[ok] - t0[ok]) * sample_rate).astype(np.int64)
    reference = synth.rasterize(n, st, en).astype(np.float64)
    track = (start_us, end_us, meta)
    if kind == "wrong":
        track = synth.make_subtitle_records(seed + _OTHER_SEED, duration_s)
        ratio = float("nan")
    return UnknownRatioProblem(kind, seed, ratio, int(round(TRUE_OFFSET_S * sample_rate)), reference, track)
