"""Half-sample stability: an offset interval for every sync.

``surrogate.py`` answers "is this subtitle related to this audio at all"; a subtitle 3 s off inside the window is as
significant to it as one in place.  This module asks how precisely the offset is known, and whether the peak that won
would still win on a different half of the cues -- again with no tuned score threshold.  K HALF-SAMPLES of the subtitle,
each keeping a hashed half of its cue blocks with every position untouched, are solved beside the real one.  If the sync
is real every half peaks at the same lag and the spread of the K offsets is an interval for the offset; if the peak is a
chance maximum the halves peak all over the window.  K + 1 single-ratio solves a file are nothing on the run-boundary
path.

    subsample_lists       ``ffs_subsample_lists``: K thinned boundary lists per device-resident list, no host round trip
    offset_stats          ``ffs_offset_stats``: the K + 1 solve records of every file reduced on the device to one record
    stability_test_lists  both around ``align_batch(n * (K + 1), 1, RUNS, ...)`` for device-resident lists on both sides
    stable_sync           the seven-ratio solve of many files, the half-samples at the winning ratio, the interval

A half-sample cuts ALL runs of the list into blocks of ``block_runs`` consecutive runs and keeps block b iff bit 31 of
the surrogate hash of (seed, s >> 1, b), flipped for odd s, is set: half-samples 2j and 2j + 1 are complementary.
Seeds: file i of a call uses ``surrogate.file_seed(seed, i)`` unless the caller passes ``seeds``.

Shared with ``surrogate.py`` and kept in ``resample_call.py``: the seeds, the list checks, the block layout around the
native list call, the chunked solve with its careful redo, and the checks and first half of a sync.  This module's own:
its limits and their checks, the half-sample list maker and the reduction with its ``tol``, the record, the interval,
the verdict and its wording.

What it says and what it does not.  The interval is the central 90 % of the half-sample offsets (``off_lo``, ``off_hi``);
``max_dev`` and ``n_within`` count against the full solve's offset.  The defaults come from SYNTHETIC data only
(profiles/stability_calibration.json); nobody has measured real files.  By the rule of DESIGN 3.25 the calibration ships
NO default verdict: one half-sample in 64 of a matched ten-minute file with 8 to 10 blocks keeps next to nothing and peaks
anywhere, so the largest matched ``max_dev`` is 8182 samples, ``DEFAULT_TOL`` = twice that covers the whole window and
the classes do not separate at it (``DEFAULT_MIN_SHARE`` is None: ``stable`` is None unless the caller passes ``tol`` and
``min_share``).  The interval separates the classes in every cell (matched at most 5 samples wide, wrong at least 5203).
Parity is against the in-repo numpy model ``tests/stability_model.py``.  Nothing here changes an existing entry point;
nothing is reachable from the reference CLI.
"""
import functools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native, resample_call
from .constants import SAMPLE_RATE
# (the shared pieces keep their names here: tests reach them as ``stability.*``)
from .resample_call import (CHUNK_BUDGET, CHUNK_CAP, ResampleKind, _check_lists, _check_seed, _list_vector, _winning_lists,
                            file_seed, fmix32, list_blocks, test_lists)

# By the rules of DESIGN 3.25 on the CPU model (profiles/stability_calibration.json; synthetic data, 10 min and 1 h, 32 + 32
# files each, block_runs 1 and 8): twice the largest matched max_dev (8182: block_runs 8 at 10 min, a half-sample that kept
# next to nothing), and no share threshold, because matched (1.0) and wrong (1.0) do not separate at that tol
DEFAULT_TOL = 16364
DEFAULT_MIN_SHARE = None
DEFAULT_SUBSAMPLES = 64
MAX_SUBSAMPLES = _native.STAB_MAX_K
MAX_BLOCK_RUNS = _native.STAB_MAX_BLOCK_RUNS
MAX_BOUND = (1 << 28) - 2  # boundaries of a list whose block of n + 1 entries the ABI takes
MIN_BLOCKS = 8  # fewer blocks: a half-sample keeps none or one of them too often
_LIMIT_TEXT = "what a list block holds (%d)" % MAX_BOUND


@dataclass
class StabilityTest:
    records: np.ndarray  # one _native.STABILITY_RESULT_DTYPE record per file (host; with ``raw`` the uint8 CUDA tensor)
    table: "object"  # uint8 CUDA tensor: n * (K + 1) ffs_cand_result records, per file the real solve first
    status: np.ndarray  # int32 per file: _native.SUB_BAD_* bits of its subtitle list (0 = fine; with ``raw`` a CUDA tensor)
    seeds: np.ndarray  # uint32 per file
    stats: dict

    def solves(self) -> np.ndarray:
        """The solve records on the host: a [n, K + 1] ``_native.CAND_RESULT_DTYPE`` array (reads the table back)."""
        n = self.seeds.size
        return self.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * (self.stats["n_subsamples"] + 1)].reshape(n, -1)


@dataclass
class StabilityRecord:
    real_score: float
    real_offset: int
    off_min: int
    off_max: int
    off_median: int
    off_lo: int  # the central 90 % of the usable half-sample offsets
    off_hi: int
    max_dev: int  # max |offset - real_offset|
    max_pair_gap: int  # max |offset(2j) - offset(2j + 1)|
    pair_score_min: float
    n_sub: int  # usable half-sample records
    n_within: int  # of them with |offset - real_offset| <= tol
    n_pairs: int
    n_pairs_within: int
    tol: int
    flags: int  # _native.STAB_EMPTY / STAB_AMBIGUOUS / STAB_NO_PAIRS


@dataclass
class StableSyncResult:
    ratio: float
    ratio_index: int
    offset: int  # samples, at that ratio
    score: float
    record: StabilityRecord
    interval_samples: Tuple[int, int]  # (off_lo, off_hi)
    interval_seconds: Tuple[float, float]
    share_within: float  # n_within / n_sub
    blocks: int  # blocks the half-samples drew from
    stable: Optional[bool]  # not EMPTY and share_within >= min_share; None without a min_share
    reasons: List[str]


def n_blocks(n_boundaries: int, block_runs: int) -> int:
    """Blocks of a list with ``n_boundaries`` entries: ceil((n / 2) / block_runs)."""
    return (int(n_boundaries) // 2 + int(block_runs) - 1) // int(block_runs)


def _check_resample(n_subsamples, block_runs) -> None:
    k, b = int(n_subsamples), int(block_runs)
    if k != n_subsamples or not 1 <= k <= MAX_SUBSAMPLES:
        raise ValueError("n_subsamples=%r: need an integer in [1, %d]" % (n_subsamples, MAX_SUBSAMPLES))
    if b != block_runs or not 1 <= b <= MAX_BLOCK_RUNS:
        raise ValueError("block_runs=%r: need an integer in [1, %d]" % (block_runs, MAX_BLOCK_RUNS))


def _check_tol(tol) -> int:
    if int(tol) != tol or tol < 0:
        raise ValueError("tol=%r: need an integer >= 0" % (tol,))
    return int(tol)


def subsample_lists(list_ptr, n_bound, lens, seeds, n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, raw: bool = False):
    """``ffs_subsample_lists`` on the current stream.  Per vector: the device pointer of its ``ffs_runs_list``, a
    host-known bound of its length (``vec_max_boundaries``' convention), its length in samples and its uint32 seed.
    Returns (uint8 CUDA buffer, int64 [n, K] byte offsets of every half-sample's list block, status: ``_native.SUB_BAD_*``
    bits per vector -- all half-samples of a list whose header breaks the contract are empty lists).  Every block holds
    ``n_bound + 1`` entries.  With ``raw`` the status is the int32 CUDA tensor and nothing is waited for or read back;
    otherwise it is read back to a host array."""
    _check_resample(n_subsamples, block_runs)
    out, offs, status = list_blocks("subsample_lists", _native.subsample_lists, MAX_BOUND, _LIMIT_TEXT, list_ptr, n_bound, lens,
                                    seeds, n_subsamples, block_runs)
    return out, offs, status if raw else status.cpu().numpy()


def offset_stats(table, n_files: int, n_subsamples: int, tol: int = DEFAULT_TOL, raw: bool = False):
    """``ffs_offset_stats``: ``table`` a CUDA tensor of n_files * (n_subsamples + 1) ffs_cand_result records, per file the
    real list's solve first.  Returns one ``_native.STABILITY_RESULT_DTYPE`` record per file (a host array); with ``raw``
    the uint8 CUDA tensor that holds them."""
    k = int(n_subsamples)
    if k != n_subsamples or not 1 <= k <= MAX_SUBSAMPLES:
        raise ValueError("n_subsamples=%r: need an integer in [1, %d]" % (n_subsamples, MAX_SUBSAMPLES))
    if int(n_files) != n_files or n_files < 0:
        raise ValueError("n_files=%r: need an integer >= 0" % (n_files,))
    out = _native.offset_stats(table, int(n_files), k, _check_tol(tol))
    if raw:
        return out
    return out.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:int(n_files)]


_raw_lists = functools.partial(subsample_lists, raw=True)
_careful = functools.partial(resample_call._careful, _raw_lists)  # (ref, sub, seed, k, block_runs, w)
_KIND = ResampleKind("stability_test_lists", _raw_lists, _native.STABILITY_RESULT_DTYPE, _native.STAB_AMBIGUOUS, "n_subsamples",
                     "block_runs", MAX_BOUND, _LIMIT_TEXT)


def stability_test_lists(ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples: int,
                         n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, seed: int = 0, tol: int = DEFAULT_TOL,
                         ref_lo=None, ref_hi=None, sub_lo=None, sub_hi=None, seeds=None, budget_bytes: int = CHUNK_BUDGET,
                         raw: bool = False) -> StabilityTest:
    """The half-sample offsets of n files whose vectors are device-resident boundary lists on both sides.  Per file: the
    device pointer, length in samples and host-known list bound of its reference and of its subtitle list (and their
    levels: 0 / 1 by default; a track rasterised at ratio r has ``sub_hi`` = min(1 / r, 1)).

    Per chunk of files -- as many as ``budget_bytes`` of half-sample blocks hold -- one ``ffs_subsample_lists`` call and ONE
    ``align_batch(files * (K + 1), 1, RUNS, ...)``: every pair of a file points at the same reference list, pair 0 at
    the real list, pair 1 + s at half-sample s; the bounds travel as ``vec_max_boundaries``, so nothing waits.  The table
    is reduced by ``ffs_offset_stats`` and one record per file comes back (with the lists' status).  A file whose records
    carry ``FFS_FLAG_AMBIGUOUS`` is redone on the careful per-file path, as ``surrogate.null_test_lists`` redoes it.

    With ``raw`` everything is queued on the current stream and nothing is read back: ``records`` and ``status`` of the
    result are the CUDA tensors (uint8 records, int32 status) and no file is redone -- the caller looks at
    ``STAB_AMBIGUOUS`` itself."""
    _check_resample(n_subsamples, block_runs)
    seed = _check_seed(seed)
    tol = _check_tol(tol)
    return StabilityTest(*test_lists(_KIND, functools.partial(_native.offset_stats, tol=tol), ref_ptr, ref_len, ref_bound,
                                     sub_ptr, sub_len, sub_bound, max_offset_samples, n_subsamples, block_runs, seed, ref_lo,
                                     ref_hi, sub_lo, sub_hi, seeds, budget_bytes, raw))


def record_of(rec) -> StabilityRecord:
    """StabilityRecord of one ``_native.STABILITY_RESULT_DTYPE`` record."""
    return StabilityRecord(float(rec["real_score"]), *[int(rec[name]) for name in (
        "real_offset", "off_min", "off_max", "off_median", "off_lo", "off_hi", "max_dev", "max_pair_gap")],
        float(rec["pair_score_min"]), *[int(rec[name]) for name in ("n_sub", "n_within", "n_pairs", "n_pairs_within", "tol", "flags")])


def share_within(record: StabilityRecord) -> float:
    """n_within / n_sub (0 without a usable half-sample)."""
    return record.n_within / record.n_sub if record.n_sub else 0.0


def stable(record: StabilityRecord, min_share: Optional[float] = DEFAULT_MIN_SHARE) -> Optional[bool]:
    """The verdict: a usable record whose half-samples agree with the full solve, ``share_within`` >= ``min_share``.  None
    without a ``min_share``: the calibration ships no default, the interval stands alone."""
    if min_share is None:
        return None
    return not (record.flags & _native.STAB_EMPTY) and share_within(record) >= min_share


def assess(record: StabilityRecord, blocks: int, min_share: Optional[float] = DEFAULT_MIN_SHARE) -> List[str]:
    """What speaks against a result, worded like ``surrogate.assess``."""
    reasons: List[str] = []
    if record.flags & _native.STAB_EMPTY:
        reasons.append("empty record (no usable half-sample solve)")
    elif min_share is not None and share_within(record) < min_share:
        reasons.append("%d of %d half-samples within %d samples of the offset (share %.2f < %.2f; 90 %% interval [%d, %d])"
                       % (record.n_within, record.n_sub, record.tol, share_within(record), min_share, record.off_lo, record.off_hi))
    if blocks < MIN_BLOCKS:
        reasons.append("too few cues to resample (%d blocks < %d)" % (blocks, MIN_BLOCKS))
    return reasons


def _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_share):
    """Host checks of ``stable_sync`` (ValueError before any native call); returns (window in samples, ratios)."""
    resample_call._check_start("stable_sync", start_seconds)
    if min_share is not None and not (math.isfinite(min_share) and 0 <= min_share <= 1):
        raise ValueError("min_share=%r: need a number in [0, 1] (or None: no verdict)" % (min_share,))
    return resample_call._check_ratios_and_problems(problems, max_offset_seconds, ratios, sample_rate)


def stable_sync(problems, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
                n_subsamples: int = DEFAULT_SUBSAMPLES, block_runs: int = 1, seed: int = 0, tol: int = DEFAULT_TOL,
                min_share: Optional[float] = DEFAULT_MIN_SHARE, sample_rate: int = SAMPLE_RATE,
                start_seconds: float = 0) -> List[StableSyncResult]:
    """Sync many files and say how precisely every offset is known.  ``problems``: as ``quality.quality_sync`` takes
    them, a list of (reference, track) with the reference a two-level host vector or a ``subtitle_raster.DeviceRaster``
    and the track a (start_us, end_us, is_metadata) triple.  Per problem: the ratio, offset and score of the seven-ratio
    solve (the first maximal candidate), the track rasterised to a boundary list at that ratio (amplitude min(1 / r, 1)),
    its half-samples (``stability_test_lists``; file i resampled with ``file_seed(seed, i)``), the interval
    (off_lo, off_hi) in samples and seconds, ``share_within`` = n_within / n_sub and, with a ``min_share``, the verdict:
    ``stable`` iff the record is not EMPTY and ``share_within`` >= ``min_share``.

    Refused by name before any device work: multi-level float references, ``start_seconds`` > 0, a host reference too
    dense for a boundary list (counted on the host; a reference that is already on the device is refused once its list
    has been counted there)."""
    _check_resample(n_subsamples, block_runs)
    _check_seed(seed)
    _check_tol(tol)
    w, ratios = _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_share)
    if not problems:
        return []
    solver, recs, best, best_ratio, (data, offs, lens, bounds), n_sub = _winning_lists("stable_sync", problems, ratios, w, sample_rate)
    test = stability_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, np.uint64(data.data_ptr()) + offs.astype(np.uint64),
                                lens, bounds, w, n_subsamples, block_runs, seed, tol, solver.ref_lo, solver.ref_hi, None,
                                np.minimum(1.0 / best_ratio, 1.0))
    out = []
    for f in range(len(problems)):
        record = record_of(test.records[f])
        blocks = n_blocks(int(n_sub[f]), block_runs)
        out.append(StableSyncResult(*resample_call._sync_head(recs, best, best_ratio, f), record, (record.off_lo, record.off_hi),
                                    (record.off_lo / float(sample_rate), record.off_hi / float(sample_rate)),
                                    share_within(record), blocks, stable(record, min_share), assess(record, blocks, min_share)))
    return out
