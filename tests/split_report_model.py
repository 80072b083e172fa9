"""TEST INFRASTRUCTURE ONLY -- numpy model of the split solve's per-piece quality report (csrc/ffs_split_report.h,
ffsubsync_amd.split_report), built on tests/split_model.py: the contract the device is held to, bit for bit.

Per piece i (a maximal run [f, e) of equal block offsets, subtitle samples [f K, min(e K, S)), offset o_i):
  - curve c_i(d), d in [-W+1, W]: n11 = the exact sum of the piece's block counts, ov / n1x / nx1 over the piece's samples
    that meet the reference, scored by split_model's fp64 expression (every operation rounded on its own); exactly 0.0
    where the overlap is empty
  - moments: min / max, then the sum in the device's order (QUAL_PEAK_THREADS = 1024 threads, thread t adds lags t,
    t + 1024, ... from 0.0; the 64 lanes of a wave by xor butterfly; the 16 waves in order), mean = sum / n, then the
    centred sum of squares in the same order, std = sqrt(css / n); all scores equal -> (that score, 0.0, FLAT)
  - peaks: greedy, largest lag on ties, each at least E from every earlier one
  - own / prev / next: c_i at o_i, o_{i-1}, o_{i+1} (NaN without that neighbour); OWN_NOT_PEAK when peak 1 is not at o_i
The records are ``_native.PIECE_REPORT_DTYPE`` arrays, so the host derivation (split_report.from_record) applies as is.
"""
import numpy as np

import split_model as sm
from ffsubsync_amd import _native

THREADS = 1024
FLAT = 1
OWN_NOT_PEAK = 4


def piece_curve(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, lo, hi, n11):
    """c(d) for d = j - W + 1, j in [0, 2W), of the subtitle samples [lo, hi) with the given n11 row."""
    r = (np.asarray(rb) != 0).astype(np.int64)
    s = (np.asarray(sb) != 0).astype(np.int64)
    R = r.size
    w = int(max_offset_samples)
    ps = np.concatenate([[0], np.cumsum(s)])
    pr = np.concatenate([[0], np.cumsum(r)])
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    c00, c01, c10, c11 = s0 * r0, s0 * r1, s1 * r0, s1 * r1
    lag = np.arange(2 * w, dtype=np.int64) - (w - 1)
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


def brute_curve(rb, sb, ref_levels, sub_levels, max_offset_samples, lo, hi):
    """The same curve by direct counting over the piece's slice at every lag (no block counts, no prefix sums)."""
    r = np.asarray(rb) != 0
    s = np.asarray(sb) != 0
    R = r.size
    w = int(max_offset_samples)
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    c00, c01, c10, c11 = s0 * r0, s0 * r1, s1 * r0, s1 * r1
    out = np.zeros(2 * w)
    for j in range(2 * w):
        d = j - (w - 1)
        a, e = max(lo, -d), min(hi, R - d)
        if e <= a:
            continue
        x, y = s[a:e], r[a + d:e + d]
        n11, n10, n01 = int(np.sum(x & y)), int(np.sum(x & ~y)), int(np.sum(~x & y))
        n00 = (e - a) - n11 - n10 - n01
        out[j] = ((np.float64(n00) * c00 + np.float64(n01) * c01) + np.float64(n10) * c10) + np.float64(n11) * c11
    return out


def device_sum(x):
    """Sum of x in the device's order (quality_block_sum over thread-strided partial sums)."""
    x = np.asarray(x, dtype=np.float64)
    part = np.zeros(THREADS)
    for r0 in range(0, x.size, THREADS):
        row = x[r0:r0 + THREADS]
        part[:row.size] = part[:row.size] + row
    v = part.reshape(THREADS // 64, 64)
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ s]
    total = v[0, 0]
    for wv in range(1, THREADS // 64):
        total = total + v[wv, 0]
    return np.float64(total)


def moments(c):
    """(mean, std, flags) of a curve (never empty: 2W >= 2 lags)."""
    if c.min() == c.max():
        return np.float64(c.max()), np.float64(0.0), FLAT
    n = np.float64(c.size)
    mean = device_sum(c) / n
    e = c - mean
    return mean, np.sqrt(device_sum(e * e) / n), 0


def peaks(c, w, top_k, exclusion_samples):
    """Greedy peaks [(score, lag)], ties to the largest lag."""
    lags = np.arange(c.size, dtype=np.int64) - (w - 1)
    out = []
    ok = np.ones(c.size, bool)
    for _ in range(top_k):
        if not ok.any():
            break
        best = c[ok].max()
        i = int(np.flatnonzero(ok & (c == best))[-1])
        out.append((float(c[i]), int(lags[i])))
        ok &= np.abs(lags - lags[i]) >= exclusion_samples
    return out


def report(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, split_penalty, top_k=3,
           exclusion_samples=300, n11_blocks=None):
    """(split_model.solve's (offsets, scores, total, pieces), PIECE_REPORT_DTYPE records of the pieces, piece curves)."""
    k, w = int(block_samples), int(max_offset_samples)
    S = np.asarray(sb).size
    if n11_blocks is None:
        n11_blocks = sm.block_counts(rb, sb, k, w)
    m = sm.block_scores(rb, sb, ref_levels, sub_levels, k, w, n11=n11_blocks)
    o, total = sm.dp(m, split_penalty)
    scores = m[np.arange(m.shape[0]), o]
    offsets = o - (w - 1)
    solved = _pieces(offsets, scores, k, S)
    pieces = solved
    recs = np.zeros(len(pieces), dtype=_native.PIECE_REPORT_DTYPE)
    curves = []
    for i, (f, e, lo, hi, off, _) in enumerate(pieces):
        c = piece_curve(rb, sb, ref_levels, sub_levels, k, w, lo, hi, n11_blocks[f:e].sum(axis=0))
        curves.append(c)
        mean, std, flags = moments(c)
        pk = peaks(c, w, top_k, exclusion_samples)
        rec = recs[i]
        rec["first_block"], rec["end_block"], rec["start_sample"], rec["end_sample"], rec["offset"] = f, e, lo, hi, off
        rec["own_score"] = c[off + w - 1]
        rec["prev_score"] = c[pieces[i - 1][4] + w - 1] if i > 0 else np.nan
        rec["next_score"] = c[pieces[i + 1][4] + w - 1] if i + 1 < len(pieces) else np.nan
        rec["mean"], rec["std"], rec["n_lags"] = mean, std, 2 * w
        for q, (ps, po) in enumerate(pk):
            rec["peak_score"][q], rec["peak_offset"][q] = ps, po
        rec["n_peaks"] = len(pk)
        rec["flags"] = flags | (OWN_NOT_PEAK if not pk or pk[0][1] != off else 0)
    return (offsets, scores, float(total), solved), recs, curves


def _pieces(offsets, scores, k, S):
    out = []
    b0 = 0
    for b in range(1, offsets.size + 1):
        if b == offsets.size or offsets[b] != offsets[b0]:
            sc = 0.0
            for x in scores[b0:b]:
                sc += float(x)
            out.append((b0, b, b0 * k, min(b * k, S), int(offsets[b0]), sc))
            b0 = b
    return out
