"""Seeded cut workloads: a subtitle made for another cut of the same film or episode (theatrical against extended or
director's cut, broadcast against home release).

A ``synth`` pair (reference activity + its subtitle track at the true framerate ratio, one global offset d0 within
+-60 s, one of the seven ratios) gets 8-40 scenes of 15 s-6 min, 2-8 min apart, +10...+50 min in total:

- ``up``: a theatrical subtitle on the extended video.  Filler activity is inserted into the reference at every scene;
  the offset steps UP by each scene's length along the film, and every cue has a match.
- ``down``: an extended subtitle on the theatrical video.  Every scene's stretch is cut from the reference; the offset
  steps DOWN by each scene's length, and the cues that start inside a cut stretch have no match ("unmatched").

Scene positions are in subtitle samples at the true ratio.  Ground truth: every cue's true offset in samples, or
``UNMATCHED``; the cue records (``track``) are the ratio-1.0 cues, which the seven-ratio solve scales onto the
problem's subtitle vector.  ``workloads/splits.py`` is the +-10 min, 1-3 event workload of ``split_align``.
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE
from workloads import splits, synth

UNMATCHED = None
MIN_SCENE_S, MAX_SCENE_S = 15.0, 360.0
MIN_GAP_S, MAX_GAP_S = 120.0, 480.0
MIN_TOTAL_S, MAX_TOTAL_S = 600.0, 3000.0
MIN_SCENES, MAX_SCENES = 8, 40
MAX_D0_S = 60.0


@dataclass
class CutProblem:
    seed: int
    direction: str  # "up" or "down"
    ref: np.ndarray  # uint8 0/1 reference: the video's activity, scenes applied
    sub: np.ndarray  # uint8 0/1 subtitle vector at the true framerate ratio
    sub_hi: float  # its upper level, min(1/ratio, 1)
    ratio: float
    ratio_index: int
    d0: int  # global offset (samples) before the first scene
    scenes: List[tuple]  # (start, length) in subtitle samples: an insertion point ("up") or a cut stretch ("down")
    cue_start: np.ndarray  # cue start / end samples of the subtitle vector (the true-ratio candidate's cues)
    cue_end: np.ndarray
    track: tuple  # (start_us, end_us, is_metadata) of the ratio-1.0 cues, for cut_sync
    cue_offset: np.ndarray  # int64 true offset per cue (valid where not cue_unmatched)
    cue_unmatched: np.ndarray  # bool: the cue starts inside a stretch the video does not have

    def true_offset(self, sample: int) -> Optional[int]:
        """True offset of subtitle sample ``sample``, or ``UNMATCHED``."""
        off = self.d0
        for start, length in self.scenes:
            if self.direction == "up":
                if sample >= start:
                    off += length
            else:
                if start <= sample < start + length:
                    return UNMATCHED
                if sample >= start + length:
                    off -= length
        return off


def _scenes(rng: np.random.RandomState, n_sub: int, direction: str):
    """Scene list in subtitle samples: walk the subtitle timeline with gaps of 2-8 min; a cut stretch ("down") takes its
    own length of the timeline too; stop at 40 scenes, 2 min before the end, or before the total passes a target drawn
    from 10-50 min."""
    sr = SAMPLE_RATE
    for _ in range(10000):
        target = rng.uniform(MIN_TOTAL_S, MAX_TOTAL_S) * sr
        scenes, cur, total = [], 0, 0
        while len(scenes) < MAX_SCENES:
            gap = int(round(rng.uniform(MIN_GAP_S, MAX_GAP_S) * sr))
            length = int(round(rng.uniform(MIN_SCENE_S, MAX_SCENE_S) * sr))
            pos = cur + gap
            end = pos + (length if direction == "down" else 0)
            if end > n_sub - int(MIN_GAP_S * sr) or total + length > target:
                break
            scenes.append((pos, length))
            total += length
            cur = end
        if len(scenes) >= MIN_SCENES and total >= MIN_TOTAL_S * sr:
            return scenes
    raise RuntimeError("no scene layout")


def make_problem(seed: int, duration_s: float = 7200.0, direction: Optional[str] = None) -> CutProblem:
    """One seeded problem; ``direction`` None alternates with the seed (even: "up", odd: "down")."""
    direction = ("up" if seed % 2 == 0 else "down") if direction is None else direction
    if direction not in ("up", "down"):
        raise ValueError("direction %r: need 'up' or 'down'" % (direction,))
    spec = synth.make_pair_spec(seed, duration_s, max_true_offset_s=MAX_D0_S)
    ref, cands = synth.pair_arrays(spec)
    ti = spec.true_ratio_index
    sub = cands[ti]
    d0 = spec.true_offset_samples
    rng = np.random.RandomState(seed + 52007)
    scenes = _scenes(rng, sub.size, direction)
    # apply the scenes to the reference in original coordinates: subtitle sample i meets ref[i + d0] everywhere
    pieces, prev = [], 0
    for pos, length in scenes:
        q = min(max(pos + d0, prev), ref.size)
        pieces.append(ref[prev:q])
        if direction == "up":
            pieces.append(splits._filler(rng, length))
            prev = q
        else:
            prev = min(q + length, ref.size)
    pieces.append(ref[prev:])
    ref = np.concatenate(pieces).astype(np.uint8)
    j1 = spec.ratios.index(1.0)
    st1, en1 = spec.cand_starts[j1].astype(np.int64), spec.cand_ends[j1].astype(np.int64)
    keep = en1 > st1
    track = (st1[keep] * 10000, en1[keep] * 10000, np.zeros(int(keep.sum()), np.uint8))
    out = CutProblem(seed, direction, ref, sub, spec.cand_amp[ti], spec.ratios[ti], ti, d0, scenes,
                     spec.cand_starts[ti].astype(np.int64), spec.cand_ends[ti].astype(np.int64), track,
                     np.zeros(0, np.int64), np.zeros(0, bool))
    out.cue_offset, out.cue_unmatched = cue_truth(out, cue_samples(out.track, out.ratio))
    return out


def cue_samples(track, ratio: float, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """Scaled start sample of every cue of ``track``: the sample ``map_cues`` / ``map_cues_refined`` place it by."""
    from datetime import timedelta

    from ffsubsync_amd.split_align import _scaled_us

    return np.array([int(round(timedelta(microseconds=_scaled_us(s, ratio)).total_seconds() * sample_rate))
                     for s in track[0]], dtype=np.int64)


def cue_truth(problem: CutProblem, samples) -> tuple:
    """(true offset int64, unmatched bool) of the cues starting at ``samples``."""
    offs = np.zeros(len(samples), np.int64)
    um = np.zeros(len(samples), bool)
    for i, x in enumerate(samples):
        t = problem.true_offset(int(x))
        if t is UNMATCHED:
            um[i] = True
        else:
            offs[i] = t
    return offs, um


def score_cues(problem: CutProblem, cue_offset, cue_unmatched) -> dict:
    """Counts of a solve's per-cue outcome (offset per cue, unmatched mask) against the truth: exact (matched cue at its
    true offset), wrong (matched cue elsewhere or reported unmatched), found (unmatched cue reported unmatched), missed
    (unmatched cue given an offset)."""
    t_off, t_um = problem.cue_offset, problem.cue_unmatched
    got_um = np.asarray(cue_unmatched, bool)
    got = np.asarray(cue_offset, np.int64)
    m = ~t_um
    return {"cues": int(t_um.size), "matched_cues": int(m.sum()), "cut_cues": int(t_um.sum()),
            "exact": int(np.sum(m & ~got_um & (got == t_off))), "false_unmatched": int(np.sum(m & got_um)),
            "found": int(np.sum(t_um & got_um)), "missed": int(np.sum(t_um & ~got_um))}
