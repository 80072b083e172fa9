"""Seeded drift workloads: synth pairs whose subtitle clock drifts slowly against the video's.  SYNTHETIC data.

Built like ``synth.make_pair_spec`` (speech runs of ``synth._speech_runs``, 15 % of the runs dropped from the subtitle
track, +-0.1 s jitter on every edge) with the subtitle clock

    t_ref = t_sub * ratio * (1 + eps) + offset + wobble(t_sub)

``ratio`` one of the seven candidate framerate ratios, ``eps`` a residual ratio with |eps| in [3e-4, 6e-4] (a re-encode
at 1.0004: right in the middle of the film, seconds out at the ends), ``wobble`` zero or one period of a sinusoid over
the file with up to 1.5 s amplitude (a capture whose clock wandered).  ``clean=True`` gives eps = 0 and no wobble: the
pair ``make_pair_spec`` would give.  Optionally one stretch of filler is inserted into the reference
(``workloads/splits.py``'s filler) so that a jump and drift meet in one problem.

A problem carries the reference, the subtitle track as cue records (millisecond stamps), the candidate rasterised at
``ratio`` with synth's conventions, and the truth: ``true_offset(sample)`` for samples of that candidate and
``true_start_us`` for every cue.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE, candidate_ratios
from workloads import splits, synth

MIN_EPS, MAX_EPS = 3e-4, 6e-4
MAX_WOBBLE_S = 1.5


@dataclass
class DriftProblem:
    seed: int
    ref: np.ndarray  # uint8 0/1 reference
    sub: np.ndarray  # uint8 0/1 subtitle vector rasterised at `ratio`
    sub_hi: float  # its upper level, min(1/ratio, 1)
    ratio: float
    ratio_index: int
    start_us: np.ndarray  # the subtitle track: cue records in the subtitle clock (int64 microseconds)
    end_us: np.ndarray
    meta: np.ndarray
    true_start_us: np.ndarray  # where every cue start belongs on the reference clock (float64 microseconds)
    eps: float
    offset_s: float
    wobble_s: float  # amplitude; 0.0 = none
    wobble_phase: float
    period_s: float  # the wobble's period in subtitle-clock seconds
    break_ref_s: Optional[float] = None  # reference time of the inserted stretch, and its length
    break_len_s: float = 0.0

    def to_ref(self, t_sub):
        """Reference-clock seconds of subtitle-clock seconds."""
        t_sub = np.asarray(t_sub, dtype=np.float64)
        t = t_sub * self.ratio * (1.0 + self.eps) + self.offset_s
        if self.wobble_s:
            t = t + self.wobble_s * np.sin(2.0 * np.pi * t_sub / self.period_s + self.wobble_phase)
        if self.break_ref_s is not None:
            t = np.where(t >= self.break_ref_s, t + self.break_len_s, t)
        return t

    def true_offset(self, sample):
        """True offset (samples, float64) at samples of the candidate rasterised at ``ratio``."""
        i = np.asarray(sample, dtype=np.float64)
        return self.to_ref(i / SAMPLE_RATE / self.ratio) * SAMPLE_RATE - i

    @property
    def track(self):
        return self.start_us, self.end_us, self.meta


def _to_sub(t_ref, ratio, eps, offset_s, wobble_s, phase, period_s):
    """Inverse of the clock without a break (fixed point: the wobble's slope is ~1e-3)."""
    t = (t_ref - offset_s) / (ratio * (1.0 + eps))
    for _ in range(12):
        w = wobble_s * np.sin(2.0 * np.pi * t / period_s + phase) if wobble_s else 0.0
        t = (t_ref - offset_s - w) / (ratio * (1.0 + eps))
    return t


def make_problem(seed: int, duration_s: float = 7200.0, clean: bool = False, eps: Optional[float] = None,
                 wobble_s: Optional[float] = None, insert_break: bool = False, max_true_offset_s: float = 45.0,
                 ratio_index: Optional[int] = None) -> DriftProblem:
    """One seeded problem.  ``eps`` / ``wobble_s`` None = drawn from the seed (|eps| in [3e-4, 6e-4] with either sign;
    no wobble for half the seeds, else an amplitude in [0.5, 1.5] s); ``clean`` overrides both with zero."""
    sr = SAMPLE_RATE
    ratios = list(candidate_ratios())
    rng = np.random.RandomState(seed)  # the draws of synth.make_pair_spec, in its order
    t0, t1 = synth._speech_runs(rng, duration_s)
    ref_len = int(round(duration_s * sr))
    rs = np.rint(t0 * sr).astype(np.int64)
    re = np.minimum(rs + np.rint((t1 - t0) * sr).astype(np.int64), ref_len)
    offset_s = float(np.round(rng.uniform(-max_true_offset_s, max_true_offset_s), 2))
    ti = int(rng.randint(len(ratios)))
    keep = rng.rand(t0.size) > 0.15
    js = rng.uniform(-0.1, 0.1, t0.size)
    je = rng.uniform(-0.1, 0.1, t0.size)
    if ratio_index is not None:
        ti = int(ratio_index)
    ratio = ratios[ti]
    rng2 = np.random.RandomState(seed + 47003)
    d_eps = float(rng2.uniform(MIN_EPS, MAX_EPS) * (1.0 if rng2.rand() < 0.5 else -1.0))
    d_wob = float(rng2.uniform(0.5, MAX_WOBBLE_S)) if rng2.rand() < 0.5 else 0.0
    phase = float(rng2.uniform(0.0, 2.0 * np.pi))
    break_at = float(rng2.uniform(0.3, 0.7))
    break_len_s = float(np.round(rng2.uniform(30.0, 240.0), 2))
    eps = d_eps if eps is None else float(eps)
    wobble_s = d_wob if wobble_s is None else float(wobble_s)
    if clean:
        eps, wobble_s = 0.0, 0.0
    period_s = duration_s / ratio
    s0 = _to_sub(t0 + js, ratio, eps, offset_s, wobble_s, phase, period_s)
    s1 = _to_sub(t1 + je, ratio, eps, offset_s, wobble_s, phase, period_s)
    ok = keep & (s0 >= 0.0) & (s1 > s0)
    s0, s1 = s0[ok], s1[ok]
    start_us = np.rint(s0 * 1e3).astype(np.int64) * 1000  # srt resolution
    end_us = np.maximum(np.rint(s1 * 1e3).astype(np.int64) * 1000, start_us + 1000)
    ref = synth.rasterize(ref_len, rs, re)
    out = DriftProblem(seed, ref, np.zeros(0, np.uint8), min(1.0 / ratio, 1.0), ratio, ti, start_us, end_us,
                       np.zeros(start_us.size, np.uint8), np.zeros(0), eps, offset_s, wobble_s, phase, period_s)
    if insert_break and not clean:
        q = int(round(break_at * duration_s * sr))
        n = int(round(break_len_s * sr))
        filler = splits._filler(np.random.RandomState(seed + 47004), n)
        out.ref = np.concatenate([ref[:q], filler, ref[q:]]).astype(np.uint8)
        out.break_ref_s, out.break_len_s = q / float(sr), n / float(sr)
    # the candidate at `ratio`, rasterised as synth.make_pair_spec does (SubtitleScaler, then the speech transformer)
    a0, a1 = start_us / 1e6 * ratio, end_us / 1e6 * ratio
    n = int(a1.max() * sr) + 2
    st = np.rint(a0 * sr).astype(np.int64)
    en = np.minimum(st + np.rint((a1 - a0) * sr).astype(np.int64), n)
    out.sub = synth.rasterize(n, st, en)
    out.true_start_us = out.to_ref(start_us / 1e6) * 1e6
    return out


def block_truth(problem: DriftProblem, n_blocks: int, block_samples: int) -> np.ndarray:
    """True offset at the centre of every block of the candidate (the last block may be short)."""
    n = problem.sub.size
    lo = np.arange(n_blocks, dtype=np.float64) * block_samples
    hi = np.minimum(lo + block_samples, n)
    return problem.true_offset((lo + hi) / 2.0)


def mean_block_error(problem: DriftProblem, block_offsets, block_samples: int) -> float:
    """Mean absolute error (samples) of a solve's block offsets against ``block_truth``."""
    o = np.asarray(block_offsets, dtype=np.float64)
    return float(np.mean(np.abs(o - block_truth(problem, o.size, block_samples))))
