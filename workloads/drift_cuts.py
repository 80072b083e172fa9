"""Seeded "another cut AND a re-encode, with a scene missing" workloads.  SYNTHETIC data.

A steep ``workloads/cut_drift.make_problem(seed, fixed=True)`` problem (a drifting pair whose reference gained 2-3 long
inserts) with one stretch of 60-240 s REMOVED from the reference: the subtitle's cues of that stretch belong nowhere in
the video.  The stretch lies at least 300 s plus its own length away from every insert and is drawn from
``RandomState(seed + 777)``.

The truth per cue (the runs of ones of ``sub``, or any start samples given to ``cue_truth``), from the cue's true
reference position BEFORE the removal, ``x + cut_drift's true_offset(x)``: unmatched if that position falls inside the
removed stretch; otherwise ``true_offset``, less the removed length when the position lies behind the stretch.
"""
from dataclasses import dataclass, field

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE
from workloads import cut_drift

MIN_CUT_S, MAX_CUT_S = 60.0, 240.0
MIN_GAP_S = 300.0  # between the removed stretch and any insert, plus the stretch's own length
EDGE_S = 60.0  # and this far from either end of the reference
OFFSET_TOL = 50  # samples: a matched cue further than this from its true offset is wrong


@dataclass
class DriftCutProblem:
    seed: int
    base: cut_drift.CutDriftProblem  # the problem before the removal
    ref: np.ndarray  # uint8 0/1 reference with the inserts, the stretch removed
    cut_ref: int  # the removed stretch [cut_ref, cut_ref + cut_len) in samples of base.ref
    cut_len: int
    cue_start: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # the runs of ones of `sub`
    cue_end: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    cue_offset: np.ndarray = field(default_factory=lambda: np.zeros(0))  # float64 truth (valid where not unmatched)
    cue_unmatched: np.ndarray = field(default_factory=lambda: np.zeros(0, bool))

    @property
    def sub(self):
        return self.base.sub

    @property
    def sub_hi(self):
        return self.base.sub_hi

    @property
    def ratio(self):
        return self.base.ratio

    @property
    def ratio_index(self):
        return self.base.ratio_index

    @property
    def track(self):
        return self.base.track


def _runs(v):
    s = np.concatenate([[0], (np.asarray(v) != 0).astype(np.int8), [0]])
    d = np.diff(s)
    return np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)


def insert_intervals(base: cut_drift.CutDriftProblem):
    """(start, end) samples of every insert in base.ref."""
    sr = SAMPLE_RATE
    pos = np.rint(base.insert_ref_s * sr).astype(np.int64)
    lens = np.rint(base.insert_len_s * sr).astype(np.int64)
    start = pos + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return start, start + lens


def cue_truth(problem: DriftCutProblem, samples):
    """(true offset float64, unmatched bool) of cues starting at the subtitle ``samples``."""
    x = np.asarray(samples, dtype=np.float64)
    off = problem.base.true_offset(x)
    at = x + off
    um = (at >= problem.cut_ref) & (at < problem.cut_ref + problem.cut_len)
    return np.where(at >= problem.cut_ref + problem.cut_len, off - problem.cut_len, off), um


def make_problem(seed: int, duration_s: float = cut_drift.DEFAULT_DURATION_S) -> DriftCutProblem:
    base = cut_drift.make_problem(seed, duration_s, fixed=True)
    sr = SAMPLE_RATE
    rng = np.random.RandomState(seed + 777)
    ins_lo, ins_hi = insert_intervals(base)
    n = base.ref.size
    for _ in range(100000):
        length = int(round(rng.uniform(MIN_CUT_S, MAX_CUT_S) * sr))
        a = int(rng.randint(int(EDGE_S * sr), n - int(EDGE_S * sr) - length))
        gap = int(MIN_GAP_S * sr) + length
        if np.all((a + length + gap <= ins_lo) | (a >= ins_hi + gap)):
            break
    else:
        raise ValueError("seed %d: no room for a removed stretch" % seed)
    ref = np.concatenate([base.ref[:a], base.ref[a + length:]]).astype(np.uint8)
    out = DriftCutProblem(seed, base, ref, a, length)
    out.cue_start, out.cue_end = _runs(base.sub)
    out.cue_offset, out.cue_unmatched = cue_truth(out, out.cue_start)
    return out


def score_cues(problem: DriftCutProblem, samples, cue_offset, cue_unmatched, tol: float = OFFSET_TOL) -> dict:
    """Counts of a mapping (offset in samples and unmatched mask per cue starting at ``samples``) against the truth:
    wrong = matched cues outside the removed stretch mapped more than ``tol`` samples from their true offset; found =
    cut-scene cues marked unmatched; false = other cues marked unmatched."""
    want, t_um = cue_truth(problem, samples)
    um = np.asarray(cue_unmatched, bool)
    got = np.asarray(cue_offset, dtype=np.float64)
    wrong = ~t_um & ~um & (np.abs(got - want) > tol)
    return {"cues": int(t_um.size), "cut_cues": int(t_um.sum()), "wrong": int(wrong.sum()),
            "found": int((t_um & um).sum()), "false": int((~t_um & um).sum())}


def seeds(n: int, min_cut_cues: int = 5, duration_s: float = cut_drift.DEFAULT_DURATION_S) -> list:
    """The first ``n`` seeds that are steep (``cut_drift.nominal_ratio_is_nearest``) and whose removed stretch holds at
    least ``min_cut_cues`` cues."""
    out, seed = [], 0
    while len(out) < n:
        p = make_problem(seed, duration_s)
        if cut_drift.nominal_ratio_is_nearest(p.base) and int(p.cue_unmatched.sum()) >= min_cut_cues:
            out.append(seed)
        seed += 1
    return out
