"""Seeded "another cut AND a re-encode" workloads: a drift pair whose reference gained whole scenes.  SYNTHETIC data.

A ``workloads/drift.make_problem`` pair (residual ratio ``eps``, optional wobble; no break of its own) with 2-3
stretches of filler (``workloads/splits._filler``) inserted into the reference, 22.5-30 minutes in all: the true offset
climbs past 131 072 samples, the reach of the windowed drift solve, and between the inserts it still moves by a sample
or two per block.  ``clean=True`` keeps the inserts and drops the drift (eps = 0, no wobble).

The truth: ``true_offset(sample)`` for samples of the candidate rasterised at ``ratio``, ``block_truth`` at block
centres, ``break_blocks`` (the blocks an insert falls into) and ``mean_block_error``, which leaves out the blocks near a
true break: one block next to a 70 000-sample jump would dominate the mean.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE, candidate_ratios
from workloads import drift, splits

DEFAULT_DURATION_S = 3600.0
MIN_TOTAL_S, MAX_TOTAL_S = 22.5 * 60.0, 30.0 * 60.0
MAX_BASE_OFFSET_S = 5.0  # the pair's own offset: small against the inserts, so their total alone passes 131 072 samples
FIXED_EPS = 6e-4  # the steep subset: eps = +-FIXED_EPS (sign by seed parity), no wobble


@dataclass
class CutDriftProblem:
    seed: int
    pair: drift.DriftProblem  # the pair before the inserts (its ``ref`` is the short reference)
    ref: np.ndarray  # uint8 0/1 reference with the inserts
    insert_ref_s: np.ndarray  # where each insert went, in seconds of the reference BEFORE any insert (ascending)
    insert_len_s: np.ndarray

    @property
    def sub(self):
        return self.pair.sub

    @property
    def sub_hi(self):
        return self.pair.sub_hi

    @property
    def ratio(self):
        return self.pair.ratio

    @property
    def ratio_index(self):
        return self.pair.ratio_index

    @property
    def eps(self):
        return self.pair.eps

    @property
    def track(self):
        return self.pair.track

    def to_ref(self, t_sub):
        """Reference-clock seconds (inserts included) of subtitle-clock seconds."""
        t = self.pair.to_ref(t_sub)
        k = np.searchsorted(self.insert_ref_s, t, side="right")
        return t + np.concatenate([[0.0], np.cumsum(self.insert_len_s)])[k]

    def true_offset(self, sample):
        """True offset (samples, float64) at samples of the candidate rasterised at ``ratio``."""
        i = np.asarray(sample, dtype=np.float64)
        return self.to_ref(i / SAMPLE_RATE / self.ratio) * SAMPLE_RATE - i

    @property
    def true_start_us(self):
        return self.to_ref(self.pair.start_us / 1e6) * 1e6

    def break_samples(self) -> np.ndarray:
        """Candidate sample at which each insert falls."""
        p = self.pair
        t = drift._to_sub(self.insert_ref_s, p.ratio, p.eps, p.offset_s, p.wobble_s, p.wobble_phase, p.period_s)
        return t * p.ratio * SAMPLE_RATE


def make_problem(seed: int, duration_s: float = DEFAULT_DURATION_S, clean: bool = False, eps: Optional[float] = None,
                 wobble_s: Optional[float] = None, fixed: bool = False) -> CutDriftProblem:
    """One seeded problem.  ``eps`` / ``wobble_s`` None = drawn as ``drift.make_problem`` draws them; ``fixed`` = the
    steep subset (eps = +-6e-4 by the seed's parity, no wobble); ``clean`` = the inserts without any drift."""
    if fixed:
        eps, wobble_s = (FIXED_EPS if seed % 2 == 0 else -FIXED_EPS), 0.0
    pair = drift.make_problem(seed, duration_s, clean=clean, eps=eps, wobble_s=wobble_s,
                              max_true_offset_s=MAX_BASE_OFFSET_S)
    sr = SAMPLE_RATE
    rng = np.random.RandomState(seed + 59021)
    n_ins = int(rng.randint(2, 4))
    total_s = float(rng.uniform(MIN_TOTAL_S, MAX_TOTAL_S))
    share = rng.uniform(0.6, 1.4, n_ins)
    lens = np.rint(share / share.sum() * total_s * sr).astype(np.int64)
    # one insert in each of n_ins equal parts of the middle 70 % of the film: never closer than 7 % of it to another
    part = 0.7 / n_ins
    at = 0.15 + part * (np.arange(n_ins) + rng.uniform(0.15, 0.85, n_ins))
    pos = np.rint(at * duration_s * sr).astype(np.int64)
    pieces, prev = [], 0
    for i in range(n_ins):
        pieces.append(pair.ref[prev:pos[i]])
        pieces.append(splits._filler(np.random.RandomState(seed + 59022 + i), int(lens[i])))
        prev = int(pos[i])
    pieces.append(pair.ref[prev:])
    ref = np.concatenate(pieces).astype(np.uint8)
    return CutDriftProblem(seed, pair, ref, pos / float(sr), lens / float(sr))


def block_truth(problem: CutDriftProblem, n_blocks: int, block_samples: int) -> np.ndarray:
    """True offset at the centre of every block of the candidate (the last block may be short)."""
    n = problem.sub.size
    lo = np.arange(n_blocks, dtype=np.float64) * block_samples
    hi = np.minimum(lo + block_samples, n)
    return problem.true_offset((lo + hi) / 2.0)


def break_blocks(problem: CutDriftProblem, block_samples: int) -> np.ndarray:
    """The block each insert falls into."""
    return np.floor(problem.break_samples() / block_samples).astype(np.int64)


def mean_block_error(problem: CutDriftProblem, block_offsets, block_samples: int, exclude: int = 2) -> float:
    """Mean absolute error (samples) of a solve's block offsets against ``block_truth`` over the blocks MORE than
    ``exclude`` blocks from a true break."""
    o = np.asarray(block_offsets, dtype=np.float64)
    b = np.arange(o.size)
    keep = np.ones(o.size, bool)
    for bb in break_blocks(problem, block_samples):
        keep &= np.abs(b - bb) > exclude
    return float(np.mean(np.abs(o - block_truth(problem, o.size, block_samples))[keep]))


def nominal_ratio_is_nearest(problem: CutDriftProblem) -> bool:
    """Whether the problem's ``ratio`` is the candidate framerate ratio nearest to its clock's real ratio,
    ``ratio * (1 + eps)``.  Neighbouring candidates lie 1.0e-3 apart (1.0 / 1.001 / 0.999, 0.96 / 0.95904), so a
    residual of 6e-4 towards a neighbour leaves the file 4e-4 from THAT candidate: the seven-ratio solve then rightly
    returns the neighbour, the drift left for the block DP is the 4e-4 against it, and ``true_offset`` (which is in
    samples of the candidate rasterised at ``ratio``) does not describe that solve."""
    ratios = np.array(list(candidate_ratios()))
    return int(np.argmin(np.abs(ratios - problem.ratio * (1.0 + problem.eps)))) == problem.ratio_index


def steep_seeds(n: int, duration_s: float = DEFAULT_DURATION_S) -> list:
    """The first ``n`` seeds whose ``fixed=True`` problem keeps its nominal ratio the nearest candidate: the steep
    subset on which a solve can be held against ``true_offset``."""
    out, seed = [], 0
    while len(out) < n:
        if nominal_ratio_is_nearest(make_problem(seed, duration_s, fixed=True)):
            out.append(seed)
        seed += 1
    return out
