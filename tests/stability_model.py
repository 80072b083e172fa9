"""Numpy statement of the half-sample stability test: the thinned lists of ``ffs_subsample_lists`` byte for
byte, the half-samples' solve records by ``tests/exact_reference.py`` on the expanded lists, the record of
``ffs_offset_stats`` and ``stable_sync``'s verdict.  It does not import ``ffsubsync_amd.stability``: that module and the
device are pinned against this file, and this file against brute force (tests/test_stability_model_host.py).  The hash,
``boundaries``, ``expand`` and ``encode`` are the surrogate model's.

  - a list of n boundaries has m = n / 2 runs, cut into nb = ceil(m / B) blocks of B consecutive runs: all of them, the
    first and the last run included; the last block may be short
  - subsample s keeps block b iff ((key(seed, s >> 1, b) >> 31) ^ (s & 1)) == 1, key the surrogate's: subsamples 2j and
    2j + 1 are complementary
  - the output is the list of the kept runs, positions untouched, ones_before recomputed
  - a record is USABLE when its score is finite and its flags do not carry EMPTY_WINDOW; with the c usable subsample
    offsets sorted ascending: median = sorted[(c - 1) // 2], lo = sorted[(c - 1) // 20], hi = sorted[c - 1 - (c - 1) // 20]
  - the seed of file i of a call is fmix32(seed + i)
"""
import numpy as np

import surrogate_model as sm
from surrogate_model import boundaries, encode, expand, file_seed, fmix32, key, keys  # noqa: F401

FLAG_EMPTY_WINDOW, FLAG_AMBIGUOUS = sm.FLAG_EMPTY_WINDOW, sm.FLAG_AMBIGUOUS
EMPTY, AMBIGUOUS, NO_PAIRS = 1, 2, 4  # FFS_STAB_*
BAD_ODD, BAD_TRUNCATED, BAD_BOUND = 1, 2, 4  # FFS_SUB_BAD_*
MAX_K, MAX_BLOCK_RUNS = 4096, 1 << 24
MIN_BLOCKS = 8  # fewer blocks than this: "too few cues to resample"
INT32_MAX = sm.INT32_MAX
SEVEN = sm.SEVEN
FIELDS = ("real_score", "real_offset", "off_min", "off_max", "off_median", "off_lo", "off_hi", "max_dev", "max_pair_gap",
          "pair_score_min", "n_sub", "n_within", "n_pairs", "n_pairs_within", "tol", "flags")


def n_blocks(n, block_runs):
    return (n // 2 + block_runs - 1) // block_runs


def keep_mask(seed, s, nb):
    """Which of the blocks 0..nb-1 subsample s keeps (bool)."""
    return ((keys(seed, s >> 1, nb) >> np.uint64(31)) ^ np.uint64(s & 1)) == 1


def subsample(pos, seed, s, block_runs):
    """``pos`` of subsample s (int64): the boundaries of the kept runs, in input order."""
    pos = np.asarray(pos, dtype=np.int64)
    m = pos.size // 2
    keep = keep_mask(seed, s, n_blocks(pos.size, block_runs))[np.arange(m) // block_runs]
    return pos.reshape(m, 2)[keep].ravel()


def empty_block(length, cap):
    return sm.empty_block(length, cap)


def status(n, cap, n_bound):
    """The status bits of a list with header (n, cap) under the host's bound."""
    bad = 0
    if n & 1:
        bad |= BAD_ODD
    if n < 0 or n >= cap:
        bad |= BAD_TRUNCATED
    if n > n_bound:
        bad |= BAD_BOUND
    return bad


def usable(scores, flags):
    return sm.usable(scores, flags)


def offset_stats(scores, offsets, flags, tol):
    """The record of one file: entry 0 of every array the real solve, entry 1 + s subsample s.  A dict of
    ffs_stability_result's fields (Python ints and floats)."""
    scores, flags = np.asarray(scores, dtype=np.float64), np.asarray(flags)
    offsets = [int(o) for o in offsets]
    k = len(offsets) - 1
    ok = usable(scores, flags)
    real_ok, real = bool(ok[0]), offsets[0]
    offs = sorted(offsets[1 + s] for s in range(k) if ok[1 + s])
    c = len(offs)
    fl = AMBIGUOUS if ((flags & FLAG_AMBIGUOUS) != 0).any() else 0
    out = dict.fromkeys(FIELDS, 0)
    out.update(real_score=float(scores[0]), real_offset=real, n_sub=c, tol=int(tol), pair_score_min=0.0)
    if real_ok and c:
        out.update(off_min=offs[0], off_max=offs[-1], off_median=offs[(c - 1) // 2], off_lo=offs[(c - 1) // 20],
                   off_hi=offs[c - 1 - (c - 1) // 20], max_dev=max(abs(o - real) for o in offs),
                   n_within=sum(1 for o in offs if abs(o - real) <= tol))
    else:
        fl |= EMPTY
    pairs = [(1 + 2 * j, 2 + 2 * j) for j in range(k // 2) if ok[1 + 2 * j] and ok[2 + 2 * j]]
    if pairs:
        gaps = [abs(offsets[a] - offsets[b]) for a, b in pairs]
        sums = np.array([scores[a] + scores[b] for a, b in pairs], dtype=np.float64)
        low = float(sums.min())
        if low == 0.0 and np.signbit(sums[sums == 0.0]).any():
            low = -0.0  # (the device orders -0.0 below +0.0)
        out.update(max_pair_gap=max(gaps), pair_score_min=low, n_pairs=len(pairs),
                   n_pairs_within=sum(1 for g in gaps if g <= tol))
    else:
        fl |= NO_PAIRS
    out["flags"] = fl
    return out


def half_records(ref, sub01, ref_levels, sub_levels, max_offset_samples, seed, n_subsamples, block_runs):
    """(scores float64, offsets int64, flags int32), each [K + 1]: the exact solve record of the real vector and of its K
    half-samples against ``ref`` (a 0/1 vector or an ``exact_reference.RefSpectrum``)."""
    import exact_reference as er

    ref = ref if isinstance(ref, er.RefSpectrum) else er.RefSpectrum(np.asarray(ref) != 0)
    sub01 = np.asarray(sub01) != 0
    pos = boundaries(sub01)
    k = n_subsamples
    sc, off, fl = np.zeros(k + 1), np.zeros(k + 1, np.int64), np.zeros(k + 1, np.int32)
    for j in range(k + 1):
        v = sub01 if j == 0 else expand(subsample(pos, seed, j - 1, block_runs), sub01.size)
        rec = er.candidate(ref, v, ref_levels, sub_levels, max_offset_samples)
        sc[j], off[j], fl[j] = rec["score"], rec["offset"], rec["flags"]
    return sc, off, fl


def share_within(rec):
    return rec["n_within"] / rec["n_sub"] if rec["n_sub"] else 0.0


def stable(rec, min_share):
    """The verdict: a usable record, and at least ``min_share`` of the half-samples within tol of the full solve."""
    return not rec["flags"] & EMPTY and share_within(rec) >= min_share


def reasons(rec, blocks, min_share):
    """Reasons not to call a result stable, in ``stability.assess``'s words; empty = stable."""
    out = []
    if rec["flags"] & EMPTY:
        out.append("empty record (no usable half-sample solve)")
    elif share_within(rec) < min_share:
        out.append("%d of %d half-samples within %d samples of the offset (share %.2f < %.2f; 90 %% interval [%d, %d])"
                   % (rec["n_within"], rec["n_sub"], rec["tol"], share_within(rec), min_share, rec["off_lo"], rec["off_hi"]))
    if blocks < MIN_BLOCKS:
        out.append("too few cues to resample (%d blocks < %d)" % (blocks, MIN_BLOCKS))
    return out


def stable_sync(reference, track, max_offset_samples=6000, ratios=None, n_subsamples=64, block_runs=1, seed=0, index=0,
                tol=0, min_share=None, sample_rate=100, levels=(0.0, 1.0)):
    """One problem through the model: the seven-ratio solve (the first maximal candidate), then the half-samples at the
    winning ratio.  dict(ratio, offset, score, record, share_within, blocks, scores, offsets, stable and reasons (None
    without ``min_share``)).  ``levels``: the two values the reference's samples take, (lo, hi)."""
    import exact_reference as er
    from oracle import raster_oracle as ro

    ratios = list(SEVEN if ratios is None else ratios)
    spec = er.RefSpectrum(np.asarray(reference) != levels[0])
    best = None
    for r in ratios:
        v = ro.rasterize(track[0], track[1], track[2], float(r), sample_rate, 0) > 0
        rec = er.candidate(spec, v, levels, (0.0, min(1.0 / r, 1.0)), max_offset_samples)
        if best is None or rec["score"] > best[1]["score"]:
            best = (r, rec, v)
    r, rec, v = best
    sc, off, fl = half_records(spec, v, levels, (0.0, min(1.0 / r, 1.0)), max_offset_samples, file_seed(seed, index),
                               n_subsamples, block_runs)
    record = offset_stats(sc, off, fl, tol)
    blocks = n_blocks(boundaries(v).size, block_runs)
    return dict(ratio=float(r), offset=int(rec["offset"]), score=float(rec["score"]), record=record,
                share_within=share_within(record), blocks=blocks, scores=sc, offsets=off,
                interval_samples=(record["off_lo"], record["off_hi"]),
                reasons=None if min_share is None else reasons(record, blocks, min_share),
                stable=None if min_share is None else stable(record, min_share))
