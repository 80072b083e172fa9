"""Numpy statement of the shuffled-cue significance test: the surrogate lists of ``ffs_surrogate_lists``
byte for byte, the null scores by ``tests/exact_reference.py`` on the expanded lists, the record of ``ffs_null_stats`` and
``null_sync``'s verdict.  It does not import ``ffsubsync_amd.surrogate``: that module and the device are pinned against
this file, and this file against brute force (tests/test_surrogate_model_host.py).

  - a list of n boundaries has m = n / 2 runs; unit j < m - 1 = run j and the silence behind it; the silence in front of
    run 0, the last run and the tail stay where they are
  - the U = m - 1 units are cut into nb = ceil(U / B) blocks of B consecutive units (the last may be short); surrogate s
    places the blocks in ascending order of (key(seed, s, b), b), units keeping their order inside a block
  - key = fmix32(fmix32(seed + 0x9E3779B9 * (s + 1)) ^ b), all uint32
  - a record is USABLE when its score is finite and its flags do not carry EMPTY_WINDOW; mean and population std over the
    usable nulls, two passes; all equal -> (that score, 0.0, FLAT); p = (1 + n_ge) / (1 + n_null)
  - the seed of file i of a call is fmix32(seed + i)
"""
import math

import numpy as np

FLAG_EMPTY_WINDOW = 1  # FFS_FLAG_EMPTY_WINDOW of a solve record
FLAG_AMBIGUOUS = 2  # FFS_FLAG_AMBIGUOUS of a solve record
FLAT, EMPTY, AMBIGUOUS = 1, 2, 4  # FFS_NULL_*
BAD_ODD, BAD_TRUNCATED, BAD_BOUND, BAD_UNITS = 1, 2, 4, 8  # FFS_SURR_BAD_*
MAX_UNITS, MAX_K = 8192, 4096
MIN_BLOCKS = 8  # fewer blocks than this: "too few cues to shuffle"
INT32_MAX = 2 ** 31 - 1
_M32 = 0xFFFFFFFF
_FRAMERATE_RATIOS = [24.0 / 23.976, 25.0 / 23.976, 25.0 / 24.0]  # ffsubsync/constants.py:9
SEVEN = [1.0] + _FRAMERATE_RATIOS + [1.0 / r for r in _FRAMERATE_RATIOS]  # ffsubsync.py:131-141


def fmix32(h):
    h &= _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    h ^= h >> 16
    return h


def key(seed, s, b):
    return fmix32(fmix32((seed + 0x9E3779B9 * (s + 1)) & _M32) ^ b)


def keys(seed, s, nb):
    """uint32 keys of blocks 0..nb-1 (numpy, the same arithmetic)."""
    h = np.full(nb, fmix32((seed + 0x9E3779B9 * (s + 1)) & _M32), np.uint64) ^ np.arange(nb, dtype=np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(_M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(_M32)
    h ^= h >> np.uint64(16)
    return h


def block_order(seed, s, nb):
    """The source block at every place of surrogate s: ascending (key, b)."""
    k = keys(seed, s, nb)
    return np.lexsort((np.arange(nb), k))


def file_seed(seed, index):
    return fmix32((int(seed) + int(index)) & _M32)


def boundaries(v01):
    """Positions where a 0/1 vector changes (a run that reaches the end closes at len): the ``pos`` of its list."""
    v = np.concatenate([[0], (np.asarray(v01) != 0).astype(np.int8), [0]])
    return np.flatnonzero(np.diff(v)).astype(np.int64)


def expand(pos, length):
    v = np.zeros(length + 1, np.int32)
    np.add.at(v, np.asarray(pos[0::2], dtype=np.int64), 1)
    np.add.at(v, np.asarray(pos[1::2], dtype=np.int64), -1)
    return (np.cumsum(v[:-1]) > 0).astype(np.uint8)


def n_blocks(n, block_units):
    u = max(n // 2 - 1, 0)
    return (u + block_units - 1) // block_units


def surrogate(pos, seed, s, block_units):
    """``pos`` of surrogate s (int64): per-unit spans and run lengths gathered in the new order and summed up."""
    pos = np.asarray(pos, dtype=np.int64)
    n = pos.size
    u = max(n // 2 - 1, 0)
    if u == 0:
        return pos.copy()
    nb = (u + block_units - 1) // block_units
    order = block_order(seed, s, nb)
    units = order[:, None] * block_units + np.arange(min(block_units, u))[None, :]  # a row per place, in the new order
    units = units[units < u]  # (row-major: the short last block loses its missing units wherever it landed)
    span = pos[2:2 * u + 2:2] - pos[0:2 * u:2]
    run = pos[1:2 * u:2] - pos[0:2 * u:2]
    start = pos[0] + np.concatenate([[0], np.cumsum(span[units])[:-1]])
    out = pos.copy()
    out[0:2 * u:2] = start
    out[1:2 * u:2] = start + run[units]
    return out


def encode(pos, length, cap):
    """The words of a list block that are written: header and n + 1 entries (int32)."""
    pos = np.asarray(pos, dtype=np.int64)
    n = pos.size
    ones_before = np.zeros(n, np.int64)
    runs = pos[1::2] - pos[0::2]
    before = np.concatenate([[0], np.cumsum(runs)])
    ones_before[0::2] = before[:-1]
    ones_before[1::2] = before[1:]
    ones = int(runs.sum())
    words = np.zeros(4 + 2 * (n + 1), np.int32)
    words[:4] = (n, ones, length, cap)
    words[4:4 + 2 * n:2] = pos
    words[5:5 + 2 * n:2] = ones_before
    words[4 + 2 * n:] = (INT32_MAX, ones)
    return words


def empty_block(length, cap):
    return np.array([0, 0, length, cap, INT32_MAX, 0], np.int32)


def status(n, cap, n_bound):
    """The status bits of a list with header (n, cap) under the host's bound."""
    bad = 0
    if n & 1:
        bad |= BAD_ODD
    if n < 0 or n >= cap:
        bad |= BAD_TRUNCATED
    if n > n_bound:
        bad |= BAD_BOUND
    if int(n / 2) - 1 > MAX_UNITS:
        bad |= BAD_UNITS
    return bad


def usable(scores, flags):
    return np.isfinite(scores) & ((np.asarray(flags) & FLAG_EMPTY_WINDOW) == 0)


def stats(scores, flags):
    """The record of one file: ``scores[0]`` / ``flags[0]`` the real solve, the rest the nulls'.  A dict of
    ffs_null_result's fields."""
    scores, flags = np.asarray(scores, dtype=np.float64), np.asarray(flags)
    real, real_ok = float(scores[0]), bool(usable(scores[:1], flags[:1])[0])
    ok = usable(scores[1:], flags[1:])
    sc = scores[1:][ok]
    fl = AMBIGUOUS if ((flags & FLAG_AMBIGUOUS) != 0).any() else 0
    out = dict(real_score=real, null_mean=0.0, null_std=0.0, null_min=0.0, null_max=0.0, n_null=int(sc.size),
               n_ge=int((sc >= real).sum()) if real_ok else 0, n_gt=int((sc > real).sum()) if real_ok else 0)
    if sc.size == 0:
        fl |= FLAT | EMPTY
    else:
        out.update(null_min=float(sc.min()), null_max=float(sc.max()))
        if sc.min() == sc.max():
            fl |= FLAT
            out["null_mean"] = float(sc[0])
        else:
            mean = float(sc.sum()) / sc.size
            out.update(null_mean=mean, null_std=float(np.sqrt(float(((sc - mean) ** 2).sum()) / sc.size)))
    if not real_ok:
        fl |= EMPTY
    out["flags"] = fl
    return out


def z_p(rec):
    z = 0.0 if (rec["flags"] & FLAT) or rec["null_std"] == 0 else (rec["real_score"] - rec["null_mean"]) / rec["null_std"]
    return z, (1.0 + rec["n_ge"]) / (1.0 + rec["n_null"])


def null_scores(ref, sub01, ref_levels, sub_levels, max_offset_samples, seed, n_surrogates, block_units):
    """(scores float64 [K + 1], flags int32 [K + 1]): the exact window-maximum score of the real vector and of its K
    surrogates against ``ref`` (a 0/1 vector or an ``exact_reference.RefSpectrum``)."""
    import exact_reference as er

    ref = ref if isinstance(ref, er.RefSpectrum) else er.RefSpectrum(np.asarray(ref) != 0)
    sub01 = np.asarray(sub01) != 0
    pos = boundaries(sub01)
    sc, fl = np.zeros(n_surrogates + 1), np.zeros(n_surrogates + 1, np.int32)
    for j in range(n_surrogates + 1):
        v = sub01 if j == 0 else expand(surrogate(pos, seed, j - 1, block_units), sub01.size)
        rec = er.candidate(ref, v, ref_levels, sub_levels, max_offset_samples)
        sc[j], fl[j] = rec["score"], rec["flags"]
    return sc, fl


def trusted(rec, min_z):
    """The verdict: no usable null reached the real score and z >= min_z."""
    return not rec["flags"] & EMPTY and rec["n_ge"] == 0 and z_p(rec)[0] >= min_z


def reasons(rec, blocks, min_z):
    """Reasons not to trust a result, in ``surrogate.assess``'s words; empty = trust it."""
    out = []
    if rec["flags"] & EMPTY:
        out.append("empty null (no usable surrogate score)")
    elif rec["flags"] & FLAT:
        out.append("flat null (std 0)")
    z, p = z_p(rec)
    if not rec["flags"] & EMPTY:
        if rec["n_ge"] > 0:
            out.append("%d of %d nulls reached the score (p = %.3f)" % (rec["n_ge"], rec["n_null"], p))
        if not rec["flags"] & FLAT and z < min_z:
            out.append("z %.1f < %.1f" % (z, min_z))
    if blocks < MIN_BLOCKS:
        out.append("too few cues to shuffle (%d blocks < %d)" % (blocks, MIN_BLOCKS))
    return out


def null_sync(reference, track, max_offset_samples=6000, ratios=None, n_surrogates=64, block_units=1, seed=0, index=0,
              min_z=None, sample_rate=100, levels=(0.0, 1.0)):
    """One problem through the model: the seven-ratio solve (the first maximal candidate), then the null at the winning
    ratio.  dict(ratio, offset, score, record, z, p, blocks, scores, reasons (None without ``min_z``)).  ``levels``: the
    two values the reference's samples take, (lo, hi)."""
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
    sc, fl = null_scores(spec, v, levels, (0.0, min(1.0 / r, 1.0)), max_offset_samples, file_seed(seed, index),
                         n_surrogates, block_units)
    record = stats(sc, fl)
    z, p = z_p(record)
    blocks = n_blocks(boundaries(v).size, block_units)
    return dict(ratio=float(r), offset=int(rec["offset"]), score=float(rec["score"]), record=record, z=z, p=p, blocks=blocks,
                scores=sc, reasons=None if min_z is None else reasons(record, blocks, min_z),
                trusted=None if min_z is None else trusted(record, min_z))
