"""Seeded split workloads: synth pairs whose video has breaks or cuts the subtitles do not share.

A ``synth`` pair (reference activity + its subtitle track at the true framerate ratio, one global offset d0) gets 1-3
events, each 30-240 s long, at least 10 min apart and at least 10 min from either end of the subtitle vector:

- ``insert``: filler activity is inserted into the reference (the video has extra content: an ad break, a recap).
  Every subtitle sample after the break meets the reference that much later: the offset jumps UP by the length.
- ``remove``: a stretch is cut from the reference (the subtitles have extra content).  The subtitle samples of the cut
  stretch meet nothing; every one after it meets the reference that much earlier: the offset jumps DOWN.  Where inside
  the unmatched stretch a solver puts the break is not determined by the data, so the truth is an interval.

Every piece's true offset stays inside the lag window [-W+1, W] with a margin of at least 10 s.  Ground truth: per event
the break interval [break_lo, break_hi] in subtitle samples (equal for insertions) and the offset of every piece.
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from ffsubsync_amd.constants import SAMPLE_RATE
from workloads import synth

MARGIN_S = 10.0
MIN_GAP_S = 600.0


@dataclass
class SplitProblem:
    seed: int
    ref: np.ndarray  # uint8 0/1 reference (the video's activity, events applied)
    sub: np.ndarray  # uint8 0/1 subtitle vector at the true framerate ratio
    sub_hi: float  # its upper level, min(1/ratio, 1)
    ratio: float
    kinds: List[str]  # per event: "insert" or "remove"
    breaks: List[tuple]  # per event: (break_lo, break_hi) in subtitle samples
    offsets: List[int]  # per piece (len(breaks) + 1): true offset in samples


def _filler(rng: np.random.RandomState, n: int) -> np.ndarray:
    t0, t1 = synth._speech_runs(rng, n / SAMPLE_RATE + 10.0)
    return synth.rasterize(n, np.rint(t0 * SAMPLE_RATE).astype(np.int64), np.rint(t1 * SAMPLE_RATE).astype(np.int64))


def make_problem(seed: int, duration_s: float = 7200.0, window_samples: int = 60000, n_events: Optional[int] = None,
                 min_event_s: float = 30.0, max_event_s: float = 240.0, clean: bool = False,
                 kinds: Optional[List[str]] = None) -> SplitProblem:
    """One seeded problem; ``clean`` gives the same pair without events (one piece at the global offset)."""
    margin = int(MARGIN_S * SAMPLE_RATE)
    lo_ok, hi_ok = -window_samples + 1 + margin, window_samples - margin
    max_d0_s = min(55.0, (window_samples - margin) / SAMPLE_RATE - 1.0)
    spec = synth.make_pair_spec(seed, duration_s, max_true_offset_s=max_d0_s)
    ref, cands = synth.pair_arrays(spec)
    ti = spec.true_ratio_index
    sub = cands[ti]
    d0 = spec.true_offset_samples
    out = SplitProblem(seed, ref, sub, spec.cand_amp[ti], spec.ratios[ti], [], [], [d0])
    if clean:
        return out
    rng = np.random.RandomState(seed + 91001)
    S = sub.size
    gap = int(MIN_GAP_S * SAMPLE_RATE)
    want = int(rng.randint(1, 4)) if n_events is None else int(n_events)
    for _ in range(1000):  # rejection sampling: positions, lengths and kinds that keep every offset in the window
        lens = np.rint(rng.uniform(min_event_s, max_event_s, want) * SAMPLE_RATE).astype(np.int64)
        kk = list(kinds) if kinds is not None else ["insert" if x else "remove" for x in rng.rand(want) < 0.5]
        # break positions: >= gap from both ends, >= gap (after a removal's unmatched stretch) apart
        pos, cur, ok = [], gap, True
        for e in range(want):
            room = S - gap - cur - sum(int(lens[x]) + gap for x in range(e + 1, want)) - (int(lens[e]) if kk[e] == "remove" else 0)
            if room < 0:
                ok = False
                break
            p = cur + int(rng.randint(0, room + 1))
            pos.append(p)
            cur = p + (int(lens[e]) if kk[e] == "remove" else 0) + gap
        if not ok:
            continue
        offs = [d0]
        for e in range(want):
            offs.append(offs[-1] + (int(lens[e]) if kk[e] == "insert" else -int(lens[e])))
        if all(lo_ok <= o <= hi_ok for o in offs):
            break
    else:
        raise RuntimeError("no event layout fits the window (seed %d)" % seed)
    # apply the events to the reference in original coordinates: subtitle sample i meets ref[i + d0] everywhere
    pieces, prev = [], 0
    for e in range(want):
        q = pos[e] + d0
        pieces.append(ref[prev:q])
        if kk[e] == "insert":
            pieces.append(_filler(rng, int(lens[e])))
            prev = q
        else:
            prev = q + int(lens[e])
    pieces.append(ref[prev:])
    out.ref = np.concatenate(pieces).astype(np.uint8)
    out.kinds = kk
    out.breaks = [(p, p + (int(n) if k == "remove" else 0)) for p, n, k in zip(pos, lens, kk)]
    out.offsets = offs
    return out


def found_breaks(block_offsets) -> List[int]:
    """Block indices b where the block offset changes from block b-1."""
    o = np.asarray(block_offsets)
    return [int(b) for b in np.flatnonzero(o[1:] != o[:-1]) + 1]


def check_recovery(problem: SplitProblem, block_offsets, block_samples: int, offset_tol: int = 2, block_tol: int = 1):
    """List of problems with a solve's block offsets against the truth (empty = recovered): the same number of pieces,
    every break within ``block_tol`` blocks of the blocks that hold its truth interval, every piece's offset within ``offset_tol``."""
    bad = []
    fb = found_breaks(block_offsets)
    if len(fb) != len(problem.breaks):
        return ["%d pieces found, %d true" % (len(fb) + 1, len(problem.breaks) + 1)]
    k = block_samples
    for b, (lo, hi) in zip(fb, problem.breaks):
        # the break's own block holds samples of both pieces: either of its boundaries is exact
        if not (lo // k - block_tol <= b <= -(-hi // k) + block_tol):
            bad.append("break at block %d (sample %d), truth [%d, %d]" % (b, b * k, lo, hi))
    o = np.asarray(block_offsets)
    starts = [0] + fb
    for s, want in zip(starts, problem.offsets):
        if abs(int(o[s]) - want) > offset_tol:
            bad.append("piece at block %d: offset %d, truth %d" % (s, int(o[s]), want))
    return bad
