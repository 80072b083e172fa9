"""Split-aware alignment you can trust: a quality report for every piece of a split solve, and evidence for every break.

A split solve (``split_align``) returns pieces, the DP's total and block scores, and nothing that says whether a piece or
a break is real: at low penalties spurious pieces appear, and a subtitle of another file still gets a tidy set of
pieces.  This module reports, per piece, the correlation curve of the piece's OWN subtitle samples over the whole lag
window -- computed exactly on the device from the split's block counts (``csrc/ffs_split_report.h``) in the same call --
and derives:

    psr       = (peak1 - mean) / std                how far the piece's best lag stands above its curve
    margin    = (peak1 - peak2) / std               ... above the best lag >= E samples away
    gain_prev = (c(o_i) - c(o_{i-1})) / std         how much the piece prefers its own offset to its neighbours'
    gain_next = (c(o_i) - c(o_{i+1})) / std

A break between pieces i and i+1 is SUPPORTED when both sides prefer their own offset: gain_next_i >= g and
gain_prev_{i+1} >= g.  ``checked_split_sync`` applies a split only when every piece passes ``min_piece_psr`` and every break
is supported, falls back to the single offset when the whole-file quality report (``quality``) trusts it, and otherwise
leaves the cues alone -- what upstream's ``--skip-sync-on-low-quality`` does.

Parity is against the in-repo numpy model ``tests/split_report_model.py``, bit for bit.  ``split_sync``,
``split_align_batch``, the ``quality`` functions and every existing entry point are unchanged.
"""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, quality
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import record_lists
from .split_align import (DEFAULT_BLOCK_SAMPLES, DEFAULT_SPLIT_PENALTY, Piece, SplitResult, _check_batch, _solve,
                          map_cues, solve_ratios, validate_args as validate_split_args)

DEFAULT_TOP_K = quality.DEFAULT_TOP_K
DEFAULT_EXCLUSION_SAMPLES = quality.DEFAULT_EXCLUSION_SAMPLES
# Chosen on the CPU model (profiles/split_report_calibration.py; synthetic data only, 64 seeds per class,
# +-10 min, K = 1024, E = 300): recovered true breaks gain >= 12.1 and their pieces psr >= 12.4; spurious breaks at
# P = 1000 gain <= 5.5 and spurious pieces psr <= 5.0; wrong pairs' breaks gain <= 6.4 and pieces psr <= 5.95
DEFAULT_MIN_GAIN = 8.0
DEFAULT_MIN_PIECE_PSR = 8.0


@dataclass
class PieceQuality:
    first_block: int
    end_block: int
    start_sample: int  # subtitle samples [start_sample, end_sample)
    end_sample: int
    offset: int
    own_score: float  # c(offset): the piece's curve at its own offset
    prev_score: float  # c at the previous piece's offset; NaN for the first piece
    next_score: float  # c at the next piece's offset; NaN for the last piece
    peaks: List[Tuple[float, int]]  # (score, offset in samples), the window maximum first
    mean: float
    std: float  # population standard deviation of the curve over the 2W lags
    n_lags: int
    psr: float  # (peak1 - mean) / std; 0 when std == 0
    margin: float  # (peak1 - peak2) / std; +inf with one peak; 0 when std == 0
    gain_prev: float  # (own - prev) / std; NaN for the first piece, 0 when std == 0
    gain_next: float  # (own - next) / std; NaN for the last piece, 0 when std == 0
    flags: int  # _native.QUALITY_FLAT / QUALITY_EMPTY_WINDOW / PIECE_OWN_NOT_PEAK

    @property
    def flat(self) -> bool:
        return bool(self.flags & _native.QUALITY_FLAT)

    @property
    def own_is_peak(self) -> bool:
        return not self.flags & _native.PIECE_OWN_NOT_PEAK


@dataclass
class SplitReport:
    split: SplitResult  # what split_align_batch returns for the pair, bit for bit
    pieces: List[PieceQuality]  # one per split.pieces entry, in order


@dataclass
class CheckedSplitResult:
    decision: str  # "split", "single" or "untrusted"
    reasons: List[str]  # why the split (and, for "untrusted", the single offset) is not trusted; empty for "split"
    ratio: float  # framerate ratio picked by the seven-ratio solve
    ratio_index: int
    global_offset: int  # that solve's single offset (samples)
    pieces: List[Piece]  # the split DP's pieces (what split_sync returns)
    piece_quality: List[PieceQuality]
    supported: List[bool]  # per break (between pieces i and i+1)
    quality: quality.AlignmentQuality  # whole-file report of the winning candidate
    cue_start_us: np.ndarray  # output cue times (int64 microseconds) of the decision
    cue_end_us: np.ndarray
    cue_piece: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # -1 for "untrusted"


def validate_args(block_samples, max_offset_samples, split_penalty, top_k, exclusion_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    validate_split_args(block_samples, max_offset_samples, split_penalty)
    quality.validate_args(None, top_k, exclusion_samples)


def from_record(rec) -> PieceQuality:
    """PieceQuality of one ``_native.PIECE_REPORT_DTYPE`` record, with psr, margin and the gains derived on the host."""
    peaks = [(float(rec["peak_score"][i]), int(rec["peak_offset"][i])) for i in range(int(rec["n_peaks"]))]
    mean, std = float(rec["mean"]), float(rec["std"])
    own, prev, nxt = float(rec["own_score"]), float(rec["prev_score"]), float(rec["next_score"])
    psr, margin, flags, (gain_prev, gain_next) = quality.derive(peaks, mean, std, int(rec["flags"]), own, (prev, nxt))
    return PieceQuality(int(rec["first_block"]), int(rec["end_block"]), int(rec["start_sample"]), int(rec["end_sample"]),
                        int(rec["offset"]), own, prev, nxt, peaks, mean, std, int(rec["n_lags"]), psr, margin, gain_prev,
                        gain_next, flags)


def break_support(pieces: Sequence[PieceQuality], min_gain: float = DEFAULT_MIN_GAIN) -> List[bool]:
    """Per break (between pieces i and i+1): both sides prefer their own offset by at least ``min_gain`` std."""
    return [bool(a.gain_next >= min_gain and b.gain_prev >= min_gain) for a, b in zip(pieces[:-1], pieces[1:])]


def assess_split(pieces: Sequence[PieceQuality], min_piece_psr: float = DEFAULT_MIN_PIECE_PSR,
                 min_gain: float = DEFAULT_MIN_GAIN) -> List[str]:
    """Reasons not to trust a split, worded like ``quality.assess``; an empty list means trust it."""
    reasons: List[str] = []
    for i, q in enumerate(pieces):
        if q.flat:
            reasons.append("piece %d: flat correlation (std 0)" % i)
        elif q.psr < min_piece_psr:
            reasons.append("piece %d: psr %.1f < %.1f" % (i, q.psr, min_piece_psr))
    for i, (a, b) in enumerate(zip(pieces[:-1], pieces[1:])):
        if not (a.gain_next >= min_gain and b.gain_prev >= min_gain):
            reasons.append("break %d (block %d): gain %.1f / %.1f < %.1f" % (i, b.first_block, a.gain_next, b.gain_prev,
                                                                              min_gain))
    return reasons


def split_report_batch(batch, max_offset_samples: int, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, top_k: int = DEFAULT_TOP_K,
                       exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, pairs_in_flight: Optional[int] = None,
                       raw: bool = False):
    """``split_align.split_align_batch`` (same inputs, same checks, bit-identical result) plus the quality report of
    every piece, in one device call.  Returns one ``SplitReport`` per pair, or with ``raw`` (SplitResults,
    ``_native.PIECE_REPORT_DTYPE`` records [n_pairs, max_b], piece counts)."""
    validate_args(block_samples, max_offset_samples, split_penalty, top_k, exclusion_samples)
    _check_batch(batch)
    res, recs, counts = _solve(batch, max_offset_samples, block_samples, split_penalty, pairs_in_flight,
                               report=(int(top_k), int(exclusion_samples)))
    if raw:
        return res, recs, counts
    return [SplitReport(r, q) for r, q in zip(res, record_lists(recs, counts, from_record))]


def checked_split_sync(problems, max_offset_seconds: float = 600, block_samples: int = DEFAULT_BLOCK_SAMPLES,
                       split_penalty: float = DEFAULT_SPLIT_PENALTY, top_k: int = DEFAULT_TOP_K,
                       exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, min_piece_psr: float = DEFAULT_MIN_PIECE_PSR,
                       min_gain: float = DEFAULT_MIN_GAIN, min_psr: float = quality.DEFAULT_MIN_PSR,
                       min_margin: float = quality.DEFAULT_MIN_MARGIN, sample_rate: int = SAMPLE_RATE,
                       ratios: Optional[Sequence[float]] = None) -> List[CheckedSplitResult]:
    """``split_align.split_sync`` with a decision per problem (``problems`` as it takes them):

    - "split": every piece passes ``min_piece_psr`` and every break is supported -- the cue times of ``split_sync``;
    - "single": some piece or break fails, but the whole-file quality report of the winning candidate passes
      ``quality.assess`` -- the cues scaled, then shifted by the single offset of the seven-ratio solve;
    - "untrusted": neither -- the input cue times, unmodified."""
    return _checked_split_sync(problems, max_offset_seconds, block_samples, split_penalty, top_k, exclusion_samples,
                               min_piece_psr, min_gain, min_psr, min_margin, sample_rate, ratios)[0]


def _checked_split_sync(problems, max_offset_seconds, block_samples, split_penalty, top_k, exclusion_samples, min_piece_psr,
                        min_gain, min_psr, min_margin, sample_rate, ratios):
    """``checked_split_sync``'s work; returns (its results, the one-candidate DeviceBatch it solved, the SplitReports)."""
    w = int(round(max_offset_seconds * sample_rate))
    validate_args(block_samples, w, split_penalty, top_k, exclusion_samples)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    chosen = db.select_candidates(best)
    reps = split_report_batch(chosen, w, block_samples, split_penalty, top_k, exclusion_samples)
    whole = quality.quality_batch(chosen, w, top_k, exclusion_samples)
    out = []
    for p, ((_, (start_us, end_us, _meta)), rep, q) in enumerate(zip(problems, reps, whole)):
        ratio = ratios[int(best[p])]
        g_off = int(pres[p]["offset"])
        reasons = assess_split(rep.pieces, min_piece_psr, min_gain)
        if not reasons:
            decision = "split"
            cs, ce, which = map_cues(start_us, end_us, ratio, rep.split.pieces, sample_rate)
        else:
            single_reasons = quality.assess(q, min_psr, min_margin)
            if not single_reasons:
                decision = "single"
                last = rep.split.pieces[-1]
                one = [Piece(0, last.end_block, 0, last.end_sample, g_off, float(pres[p]["score"]))]
                cs, ce, which = map_cues(start_us, end_us, ratio, one, sample_rate)
            else:
                decision = "untrusted"
                reasons = reasons + single_reasons
                cs = np.asarray(start_us, dtype=np.int64).copy()
                ce = np.asarray(end_us, dtype=np.int64).copy()
                which = np.full(len(cs), -1, np.int64)
        out.append(CheckedSplitResult(decision, reasons, ratio, int(best[p]), g_off, rep.split.pieces, rep.pieces,
                                      break_support(rep.pieces, min_gain), q, cs, ce, which))
    return out, chosen, reps
