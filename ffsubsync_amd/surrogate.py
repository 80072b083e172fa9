"""Shuffled-cue significance: an empirical null for every alignment score.

Every "can I trust this sync?" answer of ``quality.py``, ``match.py`` and ``ratio_sweep.py`` rests on psr / margin
thresholds tuned on synthetic data.  This module asks the question that needs no tuned threshold: is the window-maximum
score of the real subtitle larger than the window-maximum scores of K SURROGATE subtitles that keep everything about the
file -- the same cues, the same silences, the same length, the same number of speech samples, the same reference -- except
which cue sits where?  Under "this subtitle has nothing to do with this audio" the real score is exchangeable with the
surrogates', so ``p = (1 + #{null >= real}) / (K + 1)`` has a false-alarm rate known by construction, whatever the file's
length or speech density.  K + 1 single-ratio solves a file are nothing on the run-boundary path.

    surrogate_lists   ``ffs_surrogate_lists``: K shuffled boundary lists per device-resident list, no host round trip
    null_stats        ``ffs_null_stats``: the K + 1 solve records of every file reduced on the device to one record
    null_test_lists   both around ``align_batch(n * (K + 1), 1, RUNS, ...)`` for device-resident lists on both sides
    null_sync         the seven-ratio solve of many files, the null at the winning ratio, z, p and the reasons

A surrogate cuts the list into units (a run and the silence behind it; the silence in front of the first run, the last
run and the tail stay), groups ``block_units`` consecutive units into blocks and places the blocks in the order of a
hash of (seed, surrogate, block).  ``block_units`` = 1 shuffles single cues; a larger value keeps stretches of dialogue
intact (the null then keeps scene-level clustering too, and is wider).

Seeds: file i of a call is shuffled with ``fmix32(seed + i)`` (``file_seed``), so a file's null depends on its position
in the call unless the caller passes ``seeds`` (one uint32 per file) to ``null_test_lists`` itself.

Shared with ``stability.py`` and kept in ``resample_call.py``: the seeds, the list checks, the block layout around the
native list call, the chunked solve with its careful redo, and the checks and first half of a sync.  This module's own:
its limits and their checks, the surrogate list maker and the reduction, the record, z, p, the verdict and its wording.

What the test says and what it does not: it tests "related at all", not "offset correct to the sample"; it covers the
+-W lag window only; its z threshold (``DEFAULT_MIN_Z``) is calibrated on synthetic data, the ``n_ge == 0`` half of the
verdict is not calibrated at all.  Parity is against the in-repo numpy model ``tests/surrogate_model.py``.  Nothing here
changes an existing entry point; nothing is reachable from the reference CLI.
"""
import functools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native, resample_call
from .constants import SAMPLE_RATE
# (the shared pieces keep their names here: callers, profiles and tests reach them as ``surrogate.*``)
from .resample_call import (CHUNK_BUDGET, CHUNK_CAP, ResampleKind, _check_lists, _check_seed, _host_boundaries, _list_vector,
                            _winning_lists, file_seed, fmix32, list_blocks, test_lists)

# Chosen on the CPU model by the rule of DESIGN 3.24 (profiles/null_calibration.json; synthetic data, 10 min and 1 h,
# 32 + 32 files each, block_units 1 and 8): the midpoint between the smallest matched z and the largest wrong z
DEFAULT_MIN_Z = 6.7  # matched >= 9.31 (block_units 8, 10 min; >= 21.97 at block_units 1), wrong <= 4.02
DEFAULT_SURROGATES = 64
MAX_SURROGATES = _native.SURR_MAX_K
MAX_UNITS = _native.SURR_MAX_UNITS
MAX_BOUND = 2 * MAX_UNITS + 2  # boundaries of a list with MAX_UNITS units
MIN_BLOCKS = 8  # fewer blocks: K surrogates repeat the few orders there are
_LIMIT_TEXT = "the unit limit (%d units, %d boundaries)" % (MAX_UNITS, MAX_BOUND)


@dataclass
class NullTest:
    records: np.ndarray  # one _native.NULL_RESULT_DTYPE record per file (host; with ``raw`` the uint8 CUDA tensor of them)
    table: "object"  # uint8 CUDA tensor: n * (K + 1) ffs_cand_result records, per file the real solve first
    status: np.ndarray  # int32 per file: _native.SURR_BAD_* bits of its subtitle list (0 = fine; with ``raw`` a CUDA tensor)
    seeds: np.ndarray  # uint32 per file
    stats: dict

    def solves(self) -> np.ndarray:
        """The solve records on the host: a [n, K + 1] ``_native.CAND_RESULT_DTYPE`` array (reads the table back)."""
        n = self.records.size
        return self.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * (self.stats["n_surrogates"] + 1)].reshape(n, -1)


@dataclass
class NullRecord:
    real_score: float
    null_mean: float
    null_std: float
    null_min: float
    null_max: float
    n_null: int  # usable null records
    n_ge: int  # of them with score >= real_score
    n_gt: int
    flags: int  # _native.NULL_FLAT / NULL_EMPTY / NULL_AMBIGUOUS


@dataclass
class NullSyncResult:
    ratio: float
    ratio_index: int
    offset: int  # samples, at that ratio
    score: float
    null: NullRecord
    z: float  # (real - null mean) / null std; 0 when the null is flat
    p: float  # (1 + n_ge) / (1 + n_null)
    blocks: int  # blocks the shuffle had to place
    trusted: bool  # n_ge == 0 and z >= min_z
    reasons: List[str]  # what speaks against the result (the last kind, "too few cues", is a warning about the null)


def n_blocks(n_boundaries: int, block_units: int) -> int:
    """Blocks of a list with ``n_boundaries`` entries: ceil((n / 2 - 1) / block_units)."""
    return (max(int(n_boundaries) // 2 - 1, 0) + int(block_units) - 1) // int(block_units)


def _check_shuffle(n_surrogates, block_units) -> None:
    k, b = int(n_surrogates), int(block_units)
    if k != n_surrogates or not 1 <= k <= MAX_SURROGATES:
        raise ValueError("n_surrogates=%r: need an integer in [1, %d]" % (n_surrogates, MAX_SURROGATES))
    if b != block_units or not 1 <= b <= MAX_UNITS:
        raise ValueError("block_units=%r: need an integer in [1, %d]" % (block_units, MAX_UNITS))


def surrogate_lists(list_ptr, n_bound, lens, seeds, n_surrogates: int = DEFAULT_SURROGATES, block_units: int = 1):
    """``ffs_surrogate_lists`` on the current stream.  Per vector: the device pointer of its ``ffs_runs_list``, a
    host-known bound of its length (``vec_max_boundaries``' convention), its length in samples and its uint32 seed.
    Returns (uint8 CUDA buffer, int64 [n, K] byte offsets of every surrogate's list block, int32 CUDA status tensor:
    ``_native.SURR_BAD_*`` bits of a list whose header breaks the contract -- all its surrogates are empty lists then).
    Every block holds ``n_bound + 1`` entries.  Nothing is waited for or read back."""
    _check_shuffle(n_surrogates, block_units)
    return list_blocks("surrogate_lists", _native.surrogate_lists, MAX_BOUND, _LIMIT_TEXT, list_ptr, n_bound, lens, seeds,
                       n_surrogates, block_units)


def null_stats(table, n_files: int, n_surrogates: int, raw: bool = False):
    """``ffs_null_stats``: ``table`` a CUDA tensor of n_files * (n_surrogates + 1) ffs_cand_result records, per file the
    real list's solve first.  Returns one ``_native.NULL_RESULT_DTYPE`` record per file (a host array); with ``raw`` the
    uint8 CUDA tensor that holds them."""
    k = int(n_surrogates)
    if k != n_surrogates or not 1 <= k <= MAX_SURROGATES:
        raise ValueError("n_surrogates=%r: need an integer in [1, %d]" % (n_surrogates, MAX_SURROGATES))
    if int(n_files) != n_files or n_files < 0:
        raise ValueError("n_files=%r: need an integer >= 0" % (n_files,))
    out = _native.null_stats(table, int(n_files), k)
    if raw:
        return out
    return out.cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:int(n_files)]


_careful = functools.partial(resample_call._careful, surrogate_lists)  # (ref, sub, seed, k, block_units, w)
_KIND = ResampleKind("null_test_lists", surrogate_lists, _native.NULL_RESULT_DTYPE, _native.NULL_AMBIGUOUS, "n_surrogates",
                     "block_units", MAX_BOUND, _LIMIT_TEXT)


def null_test_lists(ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples: int,
                    n_surrogates: int = DEFAULT_SURROGATES, block_units: int = 1, seed: int = 0, ref_lo=None, ref_hi=None,
                    sub_lo=None, sub_hi=None, seeds=None, budget_bytes: int = CHUNK_BUDGET, raw: bool = False) -> NullTest:
    """The empirical null of n files whose vectors are device-resident boundary lists on both sides.  Per file: the
    device pointer, length in samples and host-known list bound of its reference and of its subtitle list (and their
    levels: 0 / 1 by default; a track rasterised at ratio r has ``sub_hi`` = min(1 / r, 1)).

    Per chunk of files -- as many as ``budget_bytes`` of surrogate blocks hold -- one ``ffs_surrogate_lists`` call and ONE
    ``align_batch(files * (K + 1), 1, RUNS, ...)``: every pair of a file points at the same reference list, pair 0 at
    the real list, pair j at surrogate j - 1; the bounds travel as ``vec_max_boundaries``, so nothing waits.  The table is
    reduced by ``ffs_null_stats`` and one record per file comes back (with the lists' status).  A file whose records carry
    ``FFS_FLAG_AMBIGUOUS`` is redone on the careful per-file path, as ``ratio_sweep`` redoes it.

    With ``raw`` everything is queued on the current stream and nothing is read back: ``records`` and ``status`` of the
    result are the CUDA tensors (uint8 records, int32 status) and no file is redone -- the caller looks at
    ``NULL_AMBIGUOUS`` itself."""
    _check_shuffle(n_surrogates, block_units)
    seed = _check_seed(seed)
    return NullTest(*test_lists(_KIND, _native.null_stats, ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound,
                                max_offset_samples, n_surrogates, block_units, seed, ref_lo, ref_hi, sub_lo, sub_hi, seeds,
                                budget_bytes, raw))


def record_of(rec) -> NullRecord:
    """NullRecord of one ``_native.NULL_RESULT_DTYPE`` record."""
    return NullRecord(float(rec["real_score"]), float(rec["null_mean"]), float(rec["null_std"]), float(rec["null_min"]),
                      float(rec["null_max"]), int(rec["n_null"]), int(rec["n_ge"]), int(rec["n_gt"]), int(rec["flags"]))


def derive(null: NullRecord):
    """(z, p) of a record: z = (real - mean) / std, 0 when the null is flat; p = (1 + n_ge) / (1 + n_null)."""
    flat = (null.flags & _native.NULL_FLAT) != 0 or null.null_std == 0
    z = 0.0 if flat else (null.real_score - null.null_mean) / null.null_std
    return z, (1.0 + null.n_ge) / (1.0 + null.n_null)


def trusted(null: NullRecord, min_z: float = DEFAULT_MIN_Z) -> bool:
    """The verdict: no surrogate reached the real score, and the real score stands ``min_z`` null deviations above the
    null's mean."""
    z, _ = derive(null)
    return not (null.flags & _native.NULL_EMPTY) and null.n_ge == 0 and z >= min_z


def assess(null: NullRecord, blocks: int, min_z: float = DEFAULT_MIN_Z) -> List[str]:
    """What speaks against a result, worded like ``quality.assess``."""
    reasons: List[str] = []
    z, p = derive(null)
    if null.flags & _native.NULL_EMPTY:
        reasons.append("empty null (no usable surrogate score)")
    else:
        if null.flags & _native.NULL_FLAT:
            reasons.append("flat null (std 0)")
        if null.n_ge > 0:
            reasons.append("%d of %d nulls reached the score (p = %.3f)" % (null.n_ge, null.n_null, p))
        if not null.flags & _native.NULL_FLAT and z < min_z:
            reasons.append("z %.1f < %.1f" % (z, min_z))
    if blocks < MIN_BLOCKS:
        reasons.append("too few cues to shuffle (%d blocks < %d)" % (blocks, MIN_BLOCKS))
    return reasons


def _speech_cues(track) -> int:
    """Cues of a track that the rasteriser looks at (not metadata): the one bound of its runs that the host knows before
    the winning ratio is known -- how many cues merge depends on the ratio and on the rounding to the sample grid."""
    meta = track[2]
    return len(track[0]) if meta is None else int(len(track[0]) - np.count_nonzero(np.asarray(meta)))


def _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_z):
    """Host checks of ``null_sync`` (ValueError before any native call); returns (window in samples, ratios)."""
    resample_call._check_start("null_sync", start_seconds)
    if not math.isfinite(min_z):
        raise ValueError("min_z=%r: need a finite number" % (min_z,))
    w, ratios = resample_call._check_ratios_and_problems(problems, max_offset_seconds, ratios, sample_rate)
    for i, (_, track) in enumerate(problems):
        cues = _speech_cues(track)
        if cues > MAX_UNITS + 1:
            raise ValueError("track %d has %d cues that are not metadata: above the unit limit of a surrogate list (%d units)"
                             % (i, cues, MAX_UNITS))
    return w, ratios


def null_sync(problems, max_offset_seconds: float = 60, ratios: Optional[Sequence[float]] = None,
              n_surrogates: int = DEFAULT_SURROGATES, block_units: int = 1, seed: int = 0, min_z: float = DEFAULT_MIN_Z,
              sample_rate: int = SAMPLE_RATE, start_seconds: float = 0) -> List[NullSyncResult]:
    """Sync many files and say which results are more than chance.  ``problems``: as ``quality.quality_sync`` takes
    them, a list of (reference, track) with the reference a two-level host vector or a ``subtitle_raster.DeviceRaster``
    and the track a (start_us, end_us, is_metadata) triple.  Per problem: the ratio, offset and score of the seven-ratio
    solve (the first maximal candidate), the track rasterised to a boundary list at that ratio (amplitude min(1 / r, 1)),
    its empirical null (``null_test_lists``; file i shuffled with ``file_seed(seed, i)``), z, p, and the verdict:
    ``trusted`` iff no surrogate reached the score and z >= ``min_z``.

    Refused by name before any device work: multi-level float references, ``start_seconds`` > 0, a track with more cues
    that are not metadata than a surrogate list has runs (the host's bound: cues that would merge on the sample grid
    still count one each), a host reference too dense for a boundary list (counted on the host; a reference that is
    already on the device is refused once its list has been counted there)."""
    _check_shuffle(n_surrogates, block_units)
    _check_seed(seed)
    w, ratios = _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_z)
    if not problems:
        return []
    n = len(problems)
    solver, recs, best, best_ratio, (data, offs, lens, bounds), n_sub = _winning_lists("null_sync", problems, ratios, w, sample_rate)
    test = null_test_lists(solver.ref_ptr, solver.ref_len, solver.ref_bound, np.uint64(data.data_ptr()) + offs.astype(np.uint64),
                           lens, bounds, w, n_surrogates, block_units, seed, solver.ref_lo, solver.ref_hi, None,
                           np.minimum(1.0 / best_ratio, 1.0))
    out = []
    for f in range(n):
        null = record_of(test.records[f])
        z, p = derive(null)
        blocks = n_blocks(int(n_sub[f]), block_units)
        out.append(NullSyncResult(*resample_call._sync_head(recs, best, best_ratio, f), null, z, p, blocks, trusted(null, min_z),
                                  assess(null, blocks, min_z)))
    return out
