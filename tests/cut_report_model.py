"""TEST INFRASTRUCTURE ONLY -- numpy model of the per-piece quality report of a split solve over any lag range
[lag_lo, lag_hi] (the full-range counterpart of tests/split_report_model.py): the contract a device report over the range
is held to, bit for bit.

Per piece i (a maximal run [f, e) of equal block offsets, subtitle samples [f K, min(e K, S)), offset o_i):
  - curve c_i(d), d in [lag_lo, lag_hi] (lag index j = d - lag_lo): n11 = the exact integer count over the piece's samples
    that meet the reference (from the runs of the piece's subtitle bits and the reference's prefix popcounts), ov / n1x
    / nx1 from prefix popcounts, scored by split_model's fp64 expression (every operation rounded on its own); exactly
    0.0 where the overlap is empty (those lags count in the moments)
  - moments and peaks: split_report_model's device-order helpers over n_lags = lag_hi - lag_lo + 1
  - own / prev / next: c_i at o_i, o_{i-1}, o_{i+1} (NaN without that neighbour); OWN_NOT_PEAK when peak 1 is not at o_i
At [-W+1, W] the records equal split_report_model.report's for the same block offsets.
"""
import numpy as np

import split_model as sm
import split_report_model as srm
from ffsubsync_amd import _native


def piece_n11(rb, sb, lo, hi, lag_lo, lag_hi):
    """n11 of subtitle samples [lo, hi) at every lag of [lag_lo, lag_hi] (int64), exact: the sum over the runs [u, v)
    of the piece's set bits of pr[v + d] - pr[u + d] on the reference's prefix popcounts."""
    r = (np.asarray(rb) != 0).astype(np.int64)
    s = (np.asarray(sb) != 0).astype(np.int64)
    R = r.size
    pr = np.concatenate([[0], np.cumsum(r)])
    lag = np.arange(int(lag_lo), int(lag_hi) + 1, dtype=np.int64)
    blk = s[lo:hi]
    edges = np.flatnonzero(np.diff(np.concatenate([[0], blk, [0]])))
    out = np.zeros(lag.size, dtype=np.int64)
    for u, v in zip(edges[0::2] + lo, edges[1::2] + lo):
        out += pr[np.clip(v + lag, 0, R)] - pr[np.clip(u + lag, 0, R)]
    return out


def piece_curve(rb, sb, ref_levels, sub_levels, lo, hi, lag_lo, lag_hi, n11=None):
    """c(d) for d in [lag_lo, lag_hi] of the subtitle samples [lo, hi)."""
    r = (np.asarray(rb) != 0).astype(np.int64)
    s = (np.asarray(sb) != 0).astype(np.int64)
    R = r.size
    if n11 is None:
        n11 = piece_n11(rb, sb, lo, hi, lag_lo, lag_hi)
    ps = np.concatenate([[0], np.cumsum(s)])
    pr = np.concatenate([[0], np.cumsum(r)])
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    c00, c01, c10, c11 = s0 * r0, s0 * r1, s1 * r0, s1 * r1
    lag = np.arange(int(lag_lo), int(lag_hi) + 1, dtype=np.int64)
    a = np.maximum(lo, -lag)
    e = np.minimum(hi, R - lag)
    ok = e > a
    a = np.where(ok, a, 0)
    e = np.where(ok, e, 0)
    ov = e - a
    m11 = np.where(ok, np.asarray(n11, dtype=np.int64), 0)
    n1x = ps[e] - ps[a]
    nx1 = np.where(ok, pr[np.clip(e + lag, 0, R)] - pr[np.clip(a + lag, 0, R)], 0)
    n10 = n1x - m11
    n01 = nx1 - m11
    n00 = ov - m11 - n10 - n01
    f = lambda x: x.astype(np.float64)
    c = ((f(n00) * c00 + f(n01) * c01) + f(n10) * c10) + f(m11) * c11
    return np.where(ok, c, 0.0)


def brute_curve(rb, sb, ref_levels, sub_levels, lo, hi, lag_lo, lag_hi):
    """The same curve by direct counting over the piece's slice at every lag (no runs, no prefix sums)."""
    r = np.asarray(rb) != 0
    s = np.asarray(sb) != 0
    R = r.size
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    c00, c01, c10, c11 = s0 * r0, s0 * r1, s1 * r0, s1 * r1
    out = np.zeros(int(lag_hi) - int(lag_lo) + 1)
    for j, d in enumerate(range(int(lag_lo), int(lag_hi) + 1)):
        a, e = max(lo, -d), min(hi, R - d)
        if e <= a:
            continue
        x, y = s[a:e], r[a + d:e + d]
        n11, n10, n01 = int(np.sum(x & y)), int(np.sum(x & ~y)), int(np.sum(~x & y))
        n00 = (e - a) - n11 - n10 - n01
        out[j] = ((np.float64(n00) * c00 + np.float64(n01) * c01) + np.float64(n10) * c10) + np.float64(n11) * c11
    return out


def pieces_of(offsets, block_samples, sub_len):
    """[(first_block, end_block, start_sample, end_sample, offset)] of the maximal runs of equal block offsets."""
    k, o = int(block_samples), np.asarray(offsets, dtype=np.int64)
    out, b0 = [], 0
    for b in range(1, o.size + 1):
        if b == o.size or o[b] != o[b0]:
            out.append((b0, b, b0 * k, min(b * k, int(sub_len)), int(o[b0])))
            b0 = b
    return out


def report(rb, sb, ref_levels, sub_levels, block_samples, lag_lo, lag_hi, offsets, top_k=3, exclusion_samples=300,
           which=None):
    """(PIECE_REPORT_DTYPE records of the pieces of ``offsets``, their curves).  ``which``: only these piece indices get
    their curve, moments and peaks (the others keep the piece table fields alone); None = every piece."""
    S = np.asarray(sb).size
    lo_l, hi_l = int(lag_lo), int(lag_hi)
    pieces = pieces_of(offsets, block_samples, S)
    if any(not lo_l <= p[4] <= hi_l for p in pieces):
        raise ValueError("a block offset lies outside the lag range")
    w = 1 - lo_l  # srm.peaks numbers lag index j as j - (w - 1) = j + lag_lo
    recs = np.zeros(len(pieces), dtype=_native.PIECE_REPORT_DTYPE)
    curves = {}
    for i, (f, e, lo, hi, off) in enumerate(pieces):
        rec = recs[i]
        rec["first_block"], rec["end_block"], rec["start_sample"], rec["end_sample"], rec["offset"] = f, e, lo, hi, off
        if which is not None and i not in which:
            continue
        c = piece_curve(rb, sb, ref_levels, sub_levels, lo, hi, lo_l, hi_l)
        curves[i] = c
        mean, std, flags = srm.moments(c)
        pk = srm.peaks(c, w, top_k, exclusion_samples)
        rec["own_score"] = c[off - lo_l]
        rec["prev_score"] = c[pieces[i - 1][4] - lo_l] if i > 0 else np.nan
        rec["next_score"] = c[pieces[i + 1][4] - lo_l] if i + 1 < len(pieces) else np.nan
        rec["mean"], rec["std"], rec["n_lags"] = mean, std, c.size
        for q, (ps, po) in enumerate(pk):
            rec["peak_score"][q], rec["peak_offset"][q] = ps, po
        rec["n_peaks"] = len(pk)
        rec["flags"] = flags | (srm.OWN_NOT_PEAK if not pk or pk[0][1] != off else 0)
    return recs, curves
