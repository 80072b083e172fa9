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

What the test says and what it does not: it tests "related at all", not "offset correct to the sample"; it covers the
+-W lag window only; its z threshold (``DEFAULT_MIN_Z``) is calibrated on synthetic data, the ``n_ge == 0`` half of the
verdict is not calibrated at all.  Parity is against the in-repo numpy model ``tests/surrogate_model.py``.  Nothing here
changes an existing entry point; nothing is reachable from the reference CLI.
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .constants import SAMPLE_RATE, candidate_ratios
from .side_call import pairs_for_budget

# Chosen on the CPU model by the rule of DESIGN 3.24 (profiles/null_calibration.json; synthetic data, 10 min and 1 h,
# 32 + 32 files each, block_units 1 and 8): the midpoint between the smallest matched z and the largest wrong z
DEFAULT_MIN_Z = 6.7  # matched >= 9.31 (block_units 8, 10 min; >= 21.97 at block_units 1), wrong <= 4.02
DEFAULT_SURROGATES = 64
MAX_SURROGATES = _native.SURR_MAX_K
MAX_UNITS = _native.SURR_MAX_UNITS
MAX_BOUND = 2 * MAX_UNITS + 2  # boundaries of a list with MAX_UNITS units
MIN_BLOCKS = 8  # fewer blocks: K surrogates repeat the few orders there are
CHUNK_BUDGET = 2 << 30  # bytes of surrogate list blocks one chunk may hold
CHUNK_CAP = 1 << 16  # solves per align_batch call at most


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


def fmix32(h: int) -> int:
    """The 32-bit finaliser of the surrogate hash (include/ffsubsync_amd.h)."""
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def file_seed(seed: int, index: int) -> int:
    """The seed of file ``index`` of a call made with ``seed``."""
    return fmix32((int(seed) + int(index)) & 0xFFFFFFFF)


def n_blocks(n_boundaries: int, block_units: int) -> int:
    """Blocks of a list with ``n_boundaries`` entries: ceil((n / 2 - 1) / block_units)."""
    return (max(int(n_boundaries) // 2 - 1, 0) + int(block_units) - 1) // int(block_units)


def _check_shuffle(n_surrogates, block_units) -> None:
    k, b = int(n_surrogates), int(block_units)
    if k != n_surrogates or not 1 <= k <= MAX_SURROGATES:
        raise ValueError("n_surrogates=%r: need an integer in [1, %d]" % (n_surrogates, MAX_SURROGATES))
    if b != block_units or not 1 <= b <= MAX_UNITS:
        raise ValueError("block_units=%r: need an integer in [1, %d]" % (block_units, MAX_UNITS))


def _check_seed(seed) -> int:
    if int(seed) != seed or not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("seed=%r: need an integer in [0, 2^32)" % (seed,))
    return int(seed)


def _check_lists(what, ptr, n_bound, lens):
    ptr = np.ascontiguousarray(ptr, dtype=np.uint64).ravel()
    n_bound = np.ascontiguousarray(n_bound, dtype=np.int64).ravel()
    lens = np.ascontiguousarray(lens, dtype=np.int64).ravel()
    if not ptr.size == n_bound.size == lens.size:
        raise ValueError("%s: pointers, bounds and lengths of different sizes" % what)
    if (ptr == 0).any() or (ptr & np.uint64(7)).any():
        raise ValueError("%s: a list pointer is null or not 8-byte aligned" % what)
    if (lens < 1).any():
        raise ValueError("%s: a vector of %d samples" % (what, int(lens.min())))
    if (n_bound < 0).any():
        raise ValueError("%s: a negative list bound" % what)
    return ptr, n_bound, lens


def surrogate_lists(list_ptr, n_bound, lens, seeds, n_surrogates: int = DEFAULT_SURROGATES, block_units: int = 1):
    """``ffs_surrogate_lists`` on the current stream.  Per vector: the device pointer of its ``ffs_runs_list``, a
    host-known bound of its length (``vec_max_boundaries``' convention), its length in samples and its uint32 seed.
    Returns (uint8 CUDA buffer, int64 [n, K] byte offsets of every surrogate's list block, int32 CUDA status tensor:
    ``_native.SURR_BAD_*`` bits of a list whose header breaks the contract -- all its surrogates are empty lists then).
    Every block holds ``n_bound + 1`` entries.  Nothing is waited for or read back."""
    _check_shuffle(n_surrogates, block_units)
    ptr, n_bound, lens = _check_lists("surrogate_lists", list_ptr, n_bound, lens)
    seeds = np.ascontiguousarray(seeds, dtype=np.int64).ravel()
    if seeds.size != ptr.size or (seeds < 0).any() or (seeds > 0xFFFFFFFF).any():
        raise ValueError("surrogate_lists: need one seed in [0, 2^32) per vector")
    if (n_bound > MAX_BOUND).any():
        raise ValueError("surrogate_lists: a list of up to %d boundaries is above the unit limit (%d units, %d boundaries)"
                         % (int(n_bound.max()), MAX_UNITS, MAX_BOUND))
    torch = _native.require_gpu()
    k = int(n_surrogates)
    caps = n_bound + 1
    block = 16 + 8 * caps
    first = np.zeros(ptr.size, dtype=np.int64)
    if ptr.size:
        np.cumsum((block * k)[:-1], out=first[1:])
    total = int((block * k).sum())
    out = torch.empty(max(total, 8), dtype=torch.uint8, device="cuda")
    status = torch.empty(max(ptr.size, 1), dtype=torch.int32, device="cuda")
    _native.surrogate_lists(ptr, n_bound, seeds, first, caps, k, int(block_units), out, status)
    return out, first[:, None] + block[:, None] * np.arange(k, dtype=np.int64)[None, :], status[:ptr.size]


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


def _levels(values, n, default):
    if values is None:
        return np.full(n, default, dtype=np.float64)
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    if values.size != n or not np.all(np.isfinite(values)):
        raise ValueError("null_test_lists: need one finite level per file")
    return values


def _list_vector(ptr: int, length: int, lo: float, hi: float):
    """The vector of a device-resident list on the host, as the careful path wants it."""
    torch = _native.require_gpu()
    words = torch.empty(_native.packed_words(length), dtype=torch.int32, device="cuda")
    _native.check(_native.load().ffs_runs_to_bits(int(ptr), int(length), words.data_ptr(), _native.current_stream_ptr(torch)))
    bits = _native.unpack_bits(words, length).cpu().numpy()
    return lo + (hi - lo) * bits.astype(np.float64)


def _careful(ref, sub, seed, k, block_units, w) -> np.ndarray:
    """The K + 1 records of one file through the drop-in's ``solve_pairs`` (ambiguity handling), as ``ratio_sweep``
    redoes a file: ``ref`` / ``sub`` = (list pointer, bound, length, lo, hi)."""
    from .aligners import _Vec, solve_pairs

    buf, offs, _ = surrogate_lists([sub[0]], [sub[1]], [sub[2]], [seed], k, block_units)
    ref_vec = _Vec(_list_vector(ref[0], ref[2], ref[3], ref[4]))
    ptrs = [int(sub[0])] + [buf.data_ptr() + int(o) for o in offs[0]]
    pairs = [(ref_vec, [_Vec(_list_vector(p, sub[2], sub[3], sub[4]))]) for p in ptrs]
    cres, _ = solve_pairs(pairs, w)
    return np.ascontiguousarray(cres[:, 0])


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
    w = int(max_offset_samples)
    if w != max_offset_samples or w < 1:
        raise ValueError("max_offset_samples=%r: need a window of at least one sample" % (max_offset_samples,))
    if int(budget_bytes) < 1:
        raise ValueError("budget_bytes=%r: need a positive number of bytes" % (budget_bytes,))
    ref_ptr, ref_bound, ref_len = _check_lists("null_test_lists (references)", ref_ptr, ref_bound, ref_len)
    sub_ptr, sub_bound, sub_len = _check_lists("null_test_lists (subtitles)", sub_ptr, sub_bound, sub_len)
    n = sub_ptr.size
    if ref_ptr.size != n:
        raise ValueError("null_test_lists: %d references for %d subtitle lists" % (ref_ptr.size, n))
    if (sub_bound > MAX_BOUND).any():
        raise ValueError("null_test_lists: a subtitle list of up to %d boundaries is above the unit limit (%d units, %d "
                         "boundaries)" % (int(sub_bound.max()), MAX_UNITS, MAX_BOUND))
    if (ref_bound >= 32768).any():
        raise ValueError("null_test_lists: a reference of %d or more run boundaries is too dense for a list" % 32768)
    ref_lo, ref_hi = _levels(ref_lo, n, 0.0), _levels(ref_hi, n, 1.0)
    sub_lo, sub_hi = _levels(sub_lo, n, 0.0), _levels(sub_hi, n, 1.0)
    if seeds is None:
        seeds = np.array([file_seed(seed, i) for i in range(n)], dtype=np.int64)
    else:
        seeds = np.ascontiguousarray(seeds, dtype=np.int64).ravel()
        if seeds.size != n or (seeds < 0).any() or (seeds > 0xFFFFFFFF).any():
            raise ValueError("null_test_lists: need one seed in [0, 2^32) per file")
    torch = _native.require_gpu()
    k = int(n_surrogates)
    stats = {"files": n, "n_surrogates": k, "block_units": int(block_units), "chunks": 0, "careful_files": 0}
    table = torch.empty(max(n * (k + 1), 1) * 24, dtype=torch.uint8, device="cuda")
    if n == 0:
        return NullTest(np.zeros(0, _native.NULL_RESULT_DTYPE), table, np.zeros(0, np.int32), seeds.astype(np.uint32), stats)
    per_file = k * (16 + 8 * (int(sub_bound.max()) + 1))
    chunk = pairs_for_budget(n, per_file, cap=max(CHUNK_CAP // (k + 1), 1), budget=int(budget_bytes))
    n_fft = max(_native.plan_length(int(r), int(s), w) for r, s in zip(ref_len, sub_len))
    if n_fft > _native.MAX_FFT_LENGTH:
        raise ValueError("inputs too long for the device transform (N=%d > 2^24)" % n_fft)
    plan = _native.get_plan(n_fft, pairs_in_flight=min(chunk * (k + 1), 512), max_cand=1)
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    pair_out = torch.empty(chunk * (k + 1) * 24, dtype=torch.uint8, device="cuda")
    runs = (_native.FFS_DTYPE_RUNS, _native.FFS_DTYPE_RUNS)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        m = (b - a) * (k + 1)
        buf, offs, st = surrogate_lists(sub_ptr[a:b], sub_bound[a:b], sub_len[a:b], seeds[a:b], k, block_units)
        status[a:b] = st
        cand = np.empty((b - a, k + 1), dtype=np.uint64)
        cand[:, 0] = sub_ptr[a:b]
        cand[:, 1:] = np.uint64(buf.data_ptr()) + offs.astype(np.uint64)
        rep = lambda x: np.repeat(x[a:b], k + 1)
        ptrs, lens = np.empty(2 * m, np.uint64), np.empty(2 * m, np.int64)
        lo, hi, bounds = np.empty(2 * m), np.empty(2 * m), np.empty(2 * m, np.int32)
        ptrs[0::2], lens[0::2], lo[0::2], hi[0::2], bounds[0::2] = rep(ref_ptr), rep(ref_len), rep(ref_lo), rep(ref_hi), np.maximum(rep(ref_bound), 2)
        ptrs[1::2], lens[1::2], lo[1::2], hi[1::2], bounds[1::2] = cand.ravel(), rep(sub_len), rep(sub_lo), rep(sub_hi), np.maximum(rep(sub_bound), 2)
        plan.align_batch(m, 1, runs, ptrs, lens, lo, hi, w, None, table[a * (k + 1) * 24:], pair_out, vec_max_boundaries=bounds)
        stats["chunks"] += 1
        del buf  # (stream-ordered: the allocator hands the block out again only behind the solve)
    out = _native.null_stats(table, n, k)
    if raw:
        return NullTest(out, table, status, seeds.astype(np.uint32), stats)
    records = out.cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:n].copy()
    status_h = status.cpu().numpy()
    amb = np.flatnonzero((records["flags"] & _native.NULL_AMBIGUOUS) != 0)
    if amb.size:  # degenerate input (e.g. a silent reference): the careful path, file by file
        for f in amb:
            recs = _careful((ref_ptr[f], ref_bound[f], ref_len[f], ref_lo[f], ref_hi[f]),
                            (sub_ptr[f], sub_bound[f], sub_len[f], sub_lo[f], sub_hi[f]), int(seeds[f]), k, block_units, w)
            table[f * (k + 1) * 24:(f + 1) * (k + 1) * 24] = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            stats["careful_files"] += 1
        records = _native.null_stats(table, n, k).cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:n].copy()
    return NullTest(records, table, status_h, seeds.astype(np.uint32), stats)


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


def _host_boundaries(vec) -> int:
    """Run boundaries of a two-level host vector (``aligners._Vec``), counted on the host."""
    if vec.packed is not None:
        bits = np.unpackbits(np.asarray(vec.packed, dtype=np.uint8), bitorder="little")[:len(vec)]
    else:
        bits = np.asarray(vec.bits, dtype=np.uint8)
    return int(np.count_nonzero(np.diff(bits, prepend=0, append=0)))


def _check_sync(problems, max_offset_seconds, ratios, sample_rate, start_seconds, min_z):
    """Host checks of ``null_sync`` (ValueError before any native call); returns (window in samples, ratios)."""
    from .ratio_sweep import _check_problems

    if start_seconds > 0:
        raise ValueError("null_sync needs start_seconds <= 0: boundary lists cannot hold the negative start samples of "
                         "start_seconds > 0")
    if not math.isfinite(min_z):
        raise ValueError("min_z=%r: need a finite number" % (min_z,))
    ratios = [float(r) for r in (candidate_ratios() if ratios is None else ratios)]
    if not ratios or not all(math.isfinite(r) and r > 0 for r in ratios):
        raise ValueError("ratios=%r: need at least one finite ratio > 0" % (ratios,))
    w = _check_problems(problems, max_offset_seconds, sample_rate, CHUNK_BUDGET)
    for i, (_, track) in enumerate(problems):
        cues = _speech_cues(track)
        if cues > MAX_UNITS + 1:
            raise ValueError("track %d has %d cues that are not metadata: above the unit limit of a surrogate list (%d units)"
                             % (i, cues, MAX_UNITS))
    return w, ratios


def _winning_lists(who, problems, ratios, w, sample_rate):
    """The first half of ``null_sync`` (and of ``stability.stable_sync``): the seven-ratio solve of every problem and the
    winners rasterised to boundary lists.  Returns (solver, records [n, ratios], winning index per file, winning ratio
    per file, (buffer, byte offsets, lengths, bounds) of the lists, their boundary counts read back from the headers).
    Refuses by name (``who``) a multi-level or too dense reference before any device work."""
    from .aligners import _Vec
    from .batch_gss import PreparedRatioSolve
    from .ratio_sweep import _careful as careful_ratios

    ref_vecs = [_Vec(ref) for ref, _ in problems]
    for v in ref_vecs:
        if not v.two_level:
            raise ValueError("%s needs a two-level reference: a multi-level float reference (FFS_DTYPE_F64) is not "
                             "supported" % who)
        if v.raster is None and _host_boundaries(v) >= PreparedRatioSolve.LIST_CAP:
            raise ValueError("%s: a reference has %d or more run boundaries: too dense for a boundary list"
                             % (who, PreparedRatioSolve.LIST_CAP))
    torch = _native.require_gpu()
    n, g = len(problems), len(ratios)
    tracks = [(np.asarray(s), np.asarray(e), None if m is None else np.asarray(m)) for _, (s, e, m) in problems]
    solver = PreparedRatioSolve(ref_vecs, tracks, w, sample_rate, 0, max(ratios), n * g, max_cand=1)
    if not solver.use_lists:  # (a reference that was already on the device: counted there)
        raise ValueError("%s: a reference has %d or more run boundaries: too dense for a boundary list"
                         % (who, PreparedRatioSolve.LIST_CAP))
    # the seven-ratio solve: one rasteriser call, one align_batch
    which, rs = np.repeat(np.arange(n), g), np.tile(np.array(ratios, dtype=np.float64), n)
    seven = torch.empty(n * g * 24, dtype=torch.uint8, device="cuda")
    solver.evaluate(which, rs, seven)
    recs = seven.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * g].reshape(n, g).copy()
    for f in np.flatnonzero(((recs["flags"] & _native.FLAG_AMBIGUOUS) != 0).any(axis=1)):
        recs[f] = careful_ratios(ref_vecs[f], problems[f][1], ratios, w, sample_rate)
    best = np.array([int(np.argmax(r["score"])) for r in recs])  # (the first maximal candidate, aligners.py:154-167)
    best_ratio = np.array([ratios[j] for j in best], dtype=np.float64)
    # the winners as lists and their headers (one small read-back: how many boundaries there are to work on)
    data, offs, lens, bounds = solver.tracks.rasterize_runs(np.arange(n), best_ratio, sample_rate, 0)
    n_sub = data.view(torch.int32)[torch.from_numpy(offs // 4).to(data.device)].cpu().numpy()
    return solver, recs, best, best_ratio, (data, offs, lens, bounds), n_sub


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
        out.append(NullSyncResult(float(best_ratio[f]), int(best[f]), int(recs[f][best[f]]["offset"]),
                                  float(recs[f][best[f]]["score"]), null, z, p, blocks, trusted(null, min_z),
                                  assess(null, blocks, min_z)))
    return out
