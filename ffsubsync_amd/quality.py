"""Alignment quality report: runner-up peaks and the peak-to-sidelobe ratio of every solve.

A solve returns one number about how good it is, the raw correlation score at the winning lag.  Upstream's
``--skip-sync-on-low-quality`` thresholds that score (``--min-score``, ffsubsync.py:145-174), but its magnitude grows with
the file's length and speech density, so one threshold cannot serve a 10-minute episode and a 2-hour film.  This module
reports, per pair, statistics of the WHOLE correlation curve over the lag window -- computed exactly on the device
(``csrc/ffs_quality.h``) -- and derives two normalised ones:

    psr    = (peak1 - mean) / std                 how far the winner stands above the curve
    margin = (peak1 - peak2) / std                how far it stands above the best lag >= E samples away

where mean and std (ddof = 0) run over every lag of the window.  A wrong subtitle file (another episode, cut or
release) still gets an offset; its curve has no outstanding peak, and ``assess`` says so.

Parity is against the in-repo numpy model ``tests/quality_model.py``; peak 1 equals the solve's own record bit for bit.
Nothing here changes an existing entry point; nothing is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import bits_batch, check_two_level_batch, pairs_for_budget

DEFAULT_TOP_K = 3
DEFAULT_EXCLUSION_SAMPLES = 300  # 3 s at 100 Hz: a runner-up closer than that is the same peak's shoulder
# Chosen on the CPU model (synthetic data, 64 seeds each at 10 min and 2 h, +-60 s, E = 300): matched pairs
# psr >= 6.20, margin >= 4.64; wrong pairs psr <= 3.75, margin <= 1.78
DEFAULT_MIN_PSR = 5.0
DEFAULT_MIN_MARGIN = 3.0
MAX_TOP_K = _native.QUALITY_MAX_PEAKS


@dataclass
class AlignmentQuality:
    peaks: List[Tuple[float, int]]  # (score, offset in samples), the window maximum first
    mean: float  # of the scores over the lag window
    std: float  # population standard deviation of the same
    n_lags: int
    psr: float  # (peak1 - mean) / std; 0 when std == 0
    margin: float  # (peak1 - peak2) / std; +inf with one peak; 0 when std == 0
    flags: int  # _native.QUALITY_FLAT / QUALITY_EMPTY_WINDOW

    @property
    def flat(self) -> bool:
        return bool(self.flags & _native.QUALITY_FLAT)


@dataclass
class QualitySyncResult:
    ratio: float  # framerate ratio picked by the seven-ratio solve
    ratio_index: int
    offset: int  # that solve's offset (samples)
    score: float  # that solve's score (= quality.peaks[0][0])
    quality: AlignmentQuality
    reasons: List[str]  # assess(quality, ...): empty = trust the result


def validate_args(max_offset_samples, top_k, exclusion_samples) -> None:
    """Host-side checks of the call parameters (ValueError before any native call)."""
    if max_offset_samples is not None:
        w = int(max_offset_samples)
        if w != max_offset_samples or w < 1:
            raise ValueError("max_offset_samples=%r: need an integer W >= 1, or None" % (max_offset_samples,))
    k = int(top_k)
    if k != top_k or not 1 <= k <= MAX_TOP_K:
        raise ValueError("top_k=%r: need an integer in [1, %d]" % (top_k, MAX_TOP_K))
    e = int(exclusion_samples)
    if e != exclusion_samples or e < 1:
        raise ValueError("exclusion_samples=%r: need an integer >= 1" % (exclusion_samples,))


def derive(peaks, mean: float, std: float, flags: int, own: float = math.nan, others: Sequence[float] = ()):
    """The host derivation of every curve report (whole file, piece, segment): (psr, margin, flags, gains) of a curve
    with these ``peaks`` ((score, lag), the maximum first) and moments.  gains: (own - x) / std for each x of
    ``others`` (the curve at a neighbour's lag).  A curve with std 0 or no peak is flat: ``QUALITY_FLAT`` is set, psr and
    margin are 0, and a gain is 0 unless its x is NaN (there is no such neighbour), which stays NaN."""
    if std == 0 or not peaks:
        return 0.0, 0.0, flags | _native.QUALITY_FLAT, [math.nan if math.isnan(x) else 0.0 for x in others]
    psr = (peaks[0][0] - mean) / std
    margin = (peaks[0][0] - peaks[1][0]) / std if len(peaks) > 1 else math.inf
    return psr, margin, flags, [(own - x) / std for x in others]


def from_record(rec) -> AlignmentQuality:
    """AlignmentQuality of one ``_native.QUALITY_RESULT_DTYPE`` record, with psr and margin derived on the host."""
    peaks = [(float(rec["peak_score"][i]), int(rec["peak_offset"][i])) for i in range(int(rec["n_peaks"]))]
    mean, std = float(rec["mean"]), float(rec["std"])
    psr, margin, flags, _ = derive(peaks, mean, std, int(rec["flags"]))
    return AlignmentQuality(peaks, mean, std, int(rec["n_lags"]), psr, margin, flags)


def assess(q: AlignmentQuality, min_psr: float = DEFAULT_MIN_PSR, min_margin: float = DEFAULT_MIN_MARGIN) -> List[str]:
    """Reasons not to trust an alignment, worded like upstream's assess_alignment_quality (ffsubsync.py:145-174);
    an empty list means trust it."""
    if q.flags & _native.QUALITY_EMPTY_WINDOW:
        return ["empty lag window"]
    if q.flat:
        return ["flat correlation (std 0)"]
    reasons: List[str] = []
    if q.psr < min_psr:
        reasons.append("psr %.1f < %.1f" % (q.psr, min_psr))
    if q.margin < min_margin:
        reasons.append("margin %.1f < %.1f" % (q.margin, min_margin))
    return reasons


def _check_batch(batch) -> None:
    check_two_level_batch(batch, "quality_batch", float_ref_message=True, lists=True)


def n_lags(ref_len: int, sub_len: int, max_offset_samples: Optional[int]) -> int:
    """Size of the lag set of one pair (the reference's masked `convolve` entries, aligners.py:31-48)."""
    n = _native.fft_length(ref_len, sub_len)
    if max_offset_samples is None:
        return n
    w = int(max_offset_samples)

    def clamp(i):  # Python slice semantics of convolve[:i] / convolve[i:]
        i = i + n if i < 0 else i
        return min(max(i, 0), n)

    lo, hi = clamp(n - 1 - w - sub_len), clamp(n - 1 + w - sub_len)
    return max(hi - lo, 0)


_plans = _native.SidePlanCache(_native.QualityPlan)


def _get_plan(n_pairs: int, max_lags: int, max_samples: int, pairs_in_flight: Optional[int]):
    if pairs_in_flight is None:  # bound the workspace (12 B per lag: 144 KB per pair at +-60 s) to ~2 GiB
        pairs_in_flight = pairs_for_budget(n_pairs, 12 * max_lags + 1, cap=1024, budget=2 << 30)
    return _plans.get(pairs_in_flight, max_lags, max_samples)


def clear_plan_cache() -> None:
    _plans.clear()


def quality_batch(batch, max_offset_samples: Optional[int], top_k: int = DEFAULT_TOP_K,
                  exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, pairs_in_flight: Optional[int] = None,
                  raw: bool = False):
    """Quality report of every pair of a ``batch.DeviceBatch`` with ONE candidate per pair
    (``DeviceBatch.select_candidates``): bit-packed vectors are read as they are, 0/1 bytes go through ``to_bits()``,
    boundary lists are expanded to bits (``ffs_runs_to_bits``) in the plan's scratch buffer.  Lag window
    W = ``max_offset_samples`` (None: every lag, as FFTAligner(None)).  Returns one ``AlignmentQuality`` per pair, or with
    ``raw`` the ``_native.QUALITY_RESULT_DTYPE`` records."""
    validate_args(max_offset_samples, top_k, exclusion_samples)
    _check_batch(batch)
    torch = _native.require_gpu()
    ref_len, sub_len = batch.lens[:, 0].astype(np.int64), batch.lens[:, 1].astype(np.int64)
    n = batch.n_pairs
    max_lags = max(n_lags(int(r), int(s), max_offset_samples) for r, s in zip(ref_len, sub_len))
    plan = _get_plan(n, max(max_lags, 1), int(max(ref_len.max(), sub_len.max())), pairs_in_flight)
    batch = bits_batch(batch)
    args = list(batch.pair_arrays())
    if batch.dtype == _native.FFS_DTYPE_RUNS:
        words = (batch.lens.astype(np.int64) + 31) // 32
        slots = (words + 15) // 16 * 16  # 64-byte aligned images
        starts = np.concatenate([[0], np.cumsum(slots.ravel())[:-1]]).reshape(n, 2)
        scratch = plan.scratch_words(int(slots.sum()))
        bits_ptr = np.zeros((n, 2), dtype=np.uint64)
        st = _native.current_stream_ptr(torch)
        lib = _native.load()
        for p in range(n):
            for v in range(2):
                dst = scratch.data_ptr() + 4 * int(starts[p, v])
                _native.check(lib.ffs_runs_to_bits(int(args[4 * v][p]), int(batch.lens[p, v]), dst, st))
                bits_ptr[p, v] = dst
        args[0], args[4] = bits_ptr[:, 0], bits_ptr[:, 1]
    out = torch.empty(max(n, 1) * _native.QUALITY_RESULT_BYTES, dtype=torch.uint8, device=batch.data.device)
    plan.report(*args, max_offset_samples, top_k, exclusion_samples, out)
    recs = out.cpu().numpy().view(_native.QUALITY_RESULT_DTYPE)[:n]
    if raw:
        return recs
    return [from_record(r) for r in recs]


def quality_sync(problems, max_offset_seconds: float = 60, top_k: int = DEFAULT_TOP_K,
                 exclusion_samples: int = DEFAULT_EXCLUSION_SAMPLES, min_psr: float = DEFAULT_MIN_PSR,
                 min_margin: float = DEFAULT_MIN_MARGIN, sample_rate: int = SAMPLE_RATE,
                 ratios: Optional[Sequence[float]] = None) -> List[QualitySyncResult]:
    """Sync many files and say which results to trust.  ``problems``: as ``split_align.split_sync`` takes them, a list of
    (reference, track) with the reference a two-level host vector or a ``subtitle_raster.DeviceRaster`` and the track the
    (start_us, end_us, is_metadata) triple of ``subtitle_raster.subtitle_records``.  Per problem: the framerate ratio
    and offset of the existing seven-ratio batch solve, the quality report of the winning candidate over the same lag
    window, and ``assess``'s reasons (empty = trust it)."""
    from .split_align import solve_ratios

    w = int(round(max_offset_seconds * sample_rate))
    validate_args(w, top_k, exclusion_samples)
    ratios = list(candidate_ratios() if ratios is None else ratios)
    db, best, pres = solve_ratios(problems, w, ratios, sample_rate)
    qs = quality_batch(db.select_candidates(best), w, top_k, exclusion_samples)
    return [QualitySyncResult(ratios[int(best[p])], int(best[p]), int(pres[p]["offset"]), float(pres[p]["score"]), q,
                              assess(q, min_psr, min_margin)) for p, q in enumerate(qs)]
