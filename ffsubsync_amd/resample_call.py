"""What the resampling tests share (host wrappers): seeds, the list checks, the layout of K resampled
list blocks per vector, the chunked solve of ``files * (K + 1)`` pairs with its careful redo, and the checks and the first
half of a sync.

The shuffled-cue null (``surrogate.py``) and the half-sample stability test (``stability.py``) run the same steps around
two kernels of their own: K resampled boundary lists per file, ONE ``align_batch(files * (K + 1), 1, RUNS, ...)`` a chunk,
one reduction of the K + 1 records per file.  The steps live here once; a module keeps what is its own: its limits and
their checks, its list maker and reduction, its record dtype, dataclasses, verdict and wording.  What differs travels as
an argument (a ``ResampleKind``, a function, a name); nothing here knows which test is calling.
"""
import math
from typing import Callable, NamedTuple

import numpy as np

from . import _native
from .constants import candidate_ratios
from .side_call import pairs_for_budget

CHUNK_BUDGET = 2 << 30  # bytes of resampled list blocks one chunk may hold
CHUNK_CAP = 1 << 16  # solves per align_batch call at most


class ResampleKind(NamedTuple):
    """What ``test_lists`` needs to know of the test it runs."""
    name: str  # the entry point, for messages
    make_lists: Callable  # (list_ptr, n_bound, lens, seeds, k, block) -> (buffer, [n, K] byte offsets, CUDA status)
    record_dtype: np.dtype  # of the reduction's record
    ambiguous: int  # the record's flag of a file to redo on the careful path
    k_name: str  # the ``stats`` keys of K and of the block size
    block_name: str
    max_bound: int  # the largest subtitle list bound, and what it is the limit of
    limit_text: str


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


def _check_seeds(who, seeds, n, per):
    seeds = np.ascontiguousarray(seeds, dtype=np.int64).ravel()
    if seeds.size != n or (seeds < 0).any() or (seeds > 0xFFFFFFFF).any():
        raise ValueError("%s: need one seed in [0, 2^32) per %s" % (who, per))
    return seeds


def _check_bound(who, what, n_bound, max_bound, limit_text) -> None:
    if (n_bound > max_bound).any():
        raise ValueError("%s: a %s of up to %d boundaries is above %s" % (who, what, int(n_bound.max()), limit_text))


def list_blocks(who, native_lists, max_bound, limit_text, list_ptr, n_bound, lens, seeds, k: int, block: int):
    """K resampled lists per vector by ``native_lists`` (``_native.surrogate_lists`` / ``subsample_lists``) on the current
    stream, for the entry point ``who`` whose own checks of ``k`` and ``block`` have passed.  Every list gets a block of
    ``n_bound + 1`` entries (16 + 8 * (n_bound + 1) bytes), the K blocks of a vector back to back.  Returns (uint8 CUDA
    buffer, int64 [n, K] byte offsets of every block, int32 CUDA status tensor); nothing is waited for or read back."""
    ptr, n_bound, lens = _check_lists(who, list_ptr, n_bound, lens)
    seeds = _check_seeds(who, seeds, ptr.size, "vector")
    _check_bound(who, "list", n_bound, max_bound, limit_text)
    torch = _native.require_gpu()
    k = int(k)
    caps = n_bound + 1
    block_bytes = 16 + 8 * caps
    first = np.zeros(ptr.size, dtype=np.int64)
    if ptr.size:
        np.cumsum((block_bytes * k)[:-1], out=first[1:])
    total = int((block_bytes * k).sum())
    out = torch.empty(max(total, 8), dtype=torch.uint8, device="cuda")
    status = torch.empty(max(ptr.size, 1), dtype=torch.int32, device="cuda")
    native_lists(ptr, n_bound, seeds, first, caps, k, int(block), out, status)
    return out, first[:, None] + block_bytes[:, None] * np.arange(k, dtype=np.int64)[None, :], status[:ptr.size]


def _levels(who, values, n, default):
    if values is None:
        return np.full(n, default, dtype=np.float64)
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    if values.size != n or not np.all(np.isfinite(values)):
        raise ValueError("%s: need one finite level per file" % who)
    return values


def _list_vector(ptr: int, length: int, lo: float, hi: float):
    """The vector of a device-resident list on the host, as the careful path wants it."""
    torch = _native.require_gpu()
    words = torch.empty(_native.packed_words(length), dtype=torch.int32, device="cuda")
    _native.check(_native.load().ffs_runs_to_bits(int(ptr), int(length), words.data_ptr(), _native.current_stream_ptr(torch)))
    bits = _native.unpack_bits(words, length).cpu().numpy()
    return lo + (hi - lo) * bits.astype(np.float64)


def _careful(make_lists, ref, sub, seed, k, block, w) -> np.ndarray:
    """The K + 1 records of one file through the drop-in's ``solve_pairs`` (ambiguity handling), as ``ratio_sweep``
    redoes a file: ``ref`` / ``sub`` = (list pointer, bound, length, lo, hi), the K lists by ``make_lists``."""
    from .aligners import _Vec, solve_pairs

    buf, offs, _ = make_lists([sub[0]], [sub[1]], [sub[2]], [seed], k, block)
    ref_vec = _Vec(_list_vector(ref[0], ref[2], ref[3], ref[4]))
    ptrs = [int(sub[0])] + [buf.data_ptr() + int(o) for o in offs[0]]
    pairs = [(ref_vec, [_Vec(_list_vector(p, sub[2], sub[3], sub[4]))]) for p in ptrs]
    cres, _ = solve_pairs(pairs, w)
    return np.ascontiguousarray(cres[:, 0])


def test_lists(kind: ResampleKind, stats_call, ref_ptr, ref_len, ref_bound, sub_ptr, sub_len, sub_bound, max_offset_samples,
               k: int, block: int, seed: int, ref_lo, ref_hi, sub_lo, sub_hi, seeds, budget_bytes, raw: bool):
    """The K + 1 solves and the reduced record of n files whose vectors are device-resident boundary lists on both
    sides, for the entry point ``kind.name`` whose own checks of ``k``, ``block`` and ``seed`` have passed.

    Per chunk of files -- as many as ``budget_bytes`` of list blocks hold -- one ``kind.make_lists`` call and ONE
    ``align_batch(files * (K + 1), 1, RUNS, ...)``: every pair of a file points at the same reference list, pair 0 at
    the real list, pair 1 + s at resampled list s; the bounds travel as ``vec_max_boundaries``, so nothing waits.
    ``stats_call(table, n, K)`` reduces the table to the uint8 CUDA tensor of one ``kind.record_dtype`` record per file.
    A file whose record carries ``kind.ambiguous`` is redone on the careful per-file path; with ``raw`` nothing is read
    back and no file is redone.  Returns (records, table, status, uint32 seeds, stats): the fields of the caller's
    result, in order."""
    who = kind.name
    w = int(max_offset_samples)
    if w != max_offset_samples or w < 1:
        raise ValueError("max_offset_samples=%r: need a window of at least one sample" % (max_offset_samples,))
    if int(budget_bytes) < 1:
        raise ValueError("budget_bytes=%r: need a positive number of bytes" % (budget_bytes,))
    ref_ptr, ref_bound, ref_len = _check_lists(who + " (references)", ref_ptr, ref_bound, ref_len)
    sub_ptr, sub_bound, sub_len = _check_lists(who + " (subtitles)", sub_ptr, sub_bound, sub_len)
    n = sub_ptr.size
    if ref_ptr.size != n:
        raise ValueError("%s: %d references for %d subtitle lists" % (who, ref_ptr.size, n))
    _check_bound(who, "subtitle list", sub_bound, kind.max_bound, kind.limit_text)
    if (ref_bound >= 32768).any():
        raise ValueError("%s: a reference of %d or more run boundaries is too dense for a list" % (who, 32768))
    ref_lo, ref_hi = _levels(who, ref_lo, n, 0.0), _levels(who, ref_hi, n, 1.0)
    sub_lo, sub_hi = _levels(who, sub_lo, n, 0.0), _levels(who, sub_hi, n, 1.0)
    if seeds is None:
        seeds = np.array([file_seed(seed, i) for i in range(n)], dtype=np.int64)
    else:
        seeds = _check_seeds(who, seeds, n, "file")
    torch = _native.require_gpu()
    k = int(k)
    stats = {"files": n, kind.k_name: k, kind.block_name: int(block), "chunks": 0, "careful_files": 0}
    table = torch.empty(max(n * (k + 1), 1) * 24, dtype=torch.uint8, device="cuda")
    if n == 0:
        return np.zeros(0, kind.record_dtype), table, np.zeros(0, np.int32), seeds.astype(np.uint32), stats
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
        buf, offs, st = kind.make_lists(sub_ptr[a:b], sub_bound[a:b], sub_len[a:b], seeds[a:b], k, block)
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
    out = stats_call(table, n, k)
    if raw:
        return out, table, status, seeds.astype(np.uint32), stats
    records = out.cpu().numpy().view(kind.record_dtype)[:n].copy()
    status_h = status.cpu().numpy()
    amb = np.flatnonzero((records["flags"] & kind.ambiguous) != 0)
    if amb.size:  # degenerate input (e.g. a silent reference): the careful path, file by file
        for f in amb:
            recs = _careful(kind.make_lists, (ref_ptr[f], ref_bound[f], ref_len[f], ref_lo[f], ref_hi[f]),
                            (sub_ptr[f], sub_bound[f], sub_len[f], sub_lo[f], sub_hi[f]), int(seeds[f]), k, block, w)
            table[f * (k + 1) * 24:(f + 1) * (k + 1) * 24] = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            stats["careful_files"] += 1
        records = stats_call(table, n, k).cpu().numpy().view(kind.record_dtype)[:n].copy()
    return records, table, status_h, seeds.astype(np.uint32), stats


def _check_start(who, start_seconds) -> None:
    if start_seconds > 0:
        raise ValueError("%s needs start_seconds <= 0: boundary lists cannot hold the negative start samples of "
                         "start_seconds > 0" % who)


def _check_ratios_and_problems(problems, max_offset_seconds, ratios, sample_rate):
    """The ratios (the seven candidates by default) and the problems of a sync; returns (window in samples, ratios)."""
    from .ratio_sweep import _check_problems

    ratios = [float(r) for r in (candidate_ratios() if ratios is None else ratios)]
    if not ratios or not all(math.isfinite(r) and r > 0 for r in ratios):
        raise ValueError("ratios=%r: need at least one finite ratio > 0" % (ratios,))
    return _check_problems(problems, max_offset_seconds, sample_rate, CHUNK_BUDGET), ratios


def _host_boundaries(vec) -> int:
    """Run boundaries of a two-level host vector (``aligners._Vec``), counted on the host."""
    if vec.packed is not None:
        bits = np.unpackbits(np.asarray(vec.packed, dtype=np.uint8), bitorder="little")[:len(vec)]
    else:
        bits = np.asarray(vec.bits, dtype=np.uint8)
    return int(np.count_nonzero(np.diff(bits, prepend=0, append=0)))


def _winning_lists(who, problems, ratios, w, sample_rate):
    """The first half of a sync (``null_sync``, ``stable_sync``): the seven-ratio solve of every problem and the
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


def _sync_head(recs, best, best_ratio, f):
    """The first fields of file ``f``'s sync result: ratio, index, offset and score of its winner."""
    return float(best_ratio[f]), int(best[f]), int(recs[f][best[f]]["offset"]), float(recs[f][best[f]]["score"])
