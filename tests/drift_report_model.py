"""TEST INFRASTRUCTURE ONLY -- numpy model of the drift solve's per-segment path report (csrc/ffs_drift_report.h,
ffsubsync_amd.drift_report), built on tests/drift_model.py, split_model.py and split_report_model.py: the contract the
device is held to, bit for bit.

Per segment i (a maximal run [f, e) of blocks with no jump inside, block offsets o_b, o_min / o_max over them):
  - shift set delta in [-W+1-o_min, W-o_max] (n_lags = 2W - (o_max - o_min) shifts, shift index t = delta - delta_lo):
    every block's lag o_b + delta stays inside the window, so block b reads its count row at index t + (o_b - o_min)
  - path curve p_i(delta): OV, N11, N1X, NX1 summed over the segment's blocks as exact integers -- block b at lag
    d = o_b + delta contributes the samples [max(bK, -d), min((b+1)K, S, R-d)), n11 from the block counts -- then ONE
    split_mix expression, every fp64 operation rounded on its own; exactly 0.0 where OV = 0
  - moments and greedy peaks over the shifts as split_report_model's (peaks reported as shifts; 0 is the path itself)
  - own = p_i(0); prev = p_i(last_{i-1} - first_i), next = p_i(first_{i+1} - last_i): the path moved so that it continues
    the neighbour without a jump; NaN without that neighbour or when the shift lies outside the shift set
  - flat = max over d in [o_min, o_max] of the segment's constant-lag piece curve (split_report_model.piece_curve), the
    largest such d on ties: the best the segment can do without drifting
The records are ``_native.SEGMENT_REPORT_DTYPE`` arrays, so the host derivation (drift_report.from_record) applies.
"""
import numpy as np

import drift_model as dm
import split_model as sm
import split_report_model as srm
from ffsubsync_amd import _native

FLAT = srm.FLAT
OWN_NOT_PEAK = 4


def segments_of(jump):
    """[(first_block, end_block)] of the maximal runs of blocks with no jump inside."""
    jump = np.asarray(jump)
    out, b0 = [], 0
    for b in range(1, jump.size + 1):
        if b == jump.size or jump[b]:
            out.append((b0, b))
            b0 = b
    return out


def _coeffs(ref_levels, sub_levels):
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    return s0 * r0, s0 * r1, s1 * r0, s1 * r1


def _mix(ov, n11, n1x, nx1, coeffs):
    c00, c01, c10, c11 = coeffs
    n10 = n1x - n11
    n01 = nx1 - n11
    n00 = ov - n11 - n10 - n01
    f = lambda x: x.astype(np.float64)
    c = ((f(n00) * c00 + f(n01) * c01) + f(n10) * c10) + f(n11) * c11
    return np.where(ov > 0, c, 0.0)


def path_curve(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, first_block, end_block, offsets,
               n11_blocks):
    """p(delta) over the shift set of blocks [first_block, end_block) with block offsets ``offsets`` (all blocks' array)."""
    r = (np.asarray(rb) != 0).astype(np.int64)
    s = (np.asarray(sb) != 0).astype(np.int64)
    R, S = r.size, s.size
    k, w = int(block_samples), int(max_offset_samples)
    o = np.asarray(offsets, dtype=np.int64)[first_block:end_block]
    o_min, o_max = int(o.min()), int(o.max())
    n = 2 * w - (o_max - o_min)
    ps = np.concatenate([[0], np.cumsum(s)])
    pr = np.concatenate([[0], np.cumsum(r)])
    t = np.arange(n, dtype=np.int64)
    ov = np.zeros(n, np.int64)
    n11 = np.zeros(n, np.int64)
    n1x = np.zeros(n, np.int64)
    nx1 = np.zeros(n, np.int64)
    for b in range(first_block, end_block):
        sh = int(o[b - first_block]) - o_min
        lag = t + sh - (w - 1)
        blo, bhi = b * k, min((b + 1) * k, S)
        a = np.maximum(blo, -lag)
        e = np.minimum(bhi, R - lag)
        ok = e > a
        a = np.where(ok, a, 0)
        e = np.where(ok, e, 0)
        ov += e - a
        n11 += np.where(ok, n11_blocks[b, sh:sh + n], 0)
        n1x += ps[e] - ps[a]
        nx1 += np.where(ok, pr[np.clip(e + lag, 0, R)] - pr[np.clip(a + lag, 0, R)], 0)
    return _mix(ov, n11, n1x, nx1, _coeffs(ref_levels, sub_levels))


def brute_path_curve(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, first_block, end_block, offsets):
    """The same curve by direct counting: every block's slice against the reference at lag o_b + delta (no block
    counts, no prefix sums)."""
    r = np.asarray(rb) != 0
    s = np.asarray(sb) != 0
    R, S = r.size, s.size
    k, w = int(block_samples), int(max_offset_samples)
    o = [int(x) for x in np.asarray(offsets)[first_block:end_block]]
    d_lo, d_hi = -w + 1 - min(o), w - max(o)
    c00, c01, c10, c11 = _coeffs(ref_levels, sub_levels)
    out = np.zeros(d_hi - d_lo + 1)
    for q, delta in enumerate(range(d_lo, d_hi + 1)):
        ov = n11 = n10 = n01 = 0
        for b, ob in zip(range(first_block, end_block), o):
            d = ob + delta
            a, e = max(b * k, -d), min((b + 1) * k, S, R - d)
            if e <= a:
                continue
            x, y = s[a:e], r[a + d:e + d]
            ov += e - a
            n11 += int(np.sum(x & y))
            n10 += int(np.sum(x & ~y))
            n01 += int(np.sum(~x & y))
        if ov:
            n00 = ov - n11 - n10 - n01
            out[q] = ((np.float64(n00) * c00 + np.float64(n01) * c01) + np.float64(n10) * c10) + np.float64(n11) * c11
    return out


def shift_peaks(c, shift_lo, top_k, exclusion_samples):
    """Greedy peaks [(score, shift)] of a path curve, ties to the largest shift."""
    return [(v, idx + shift_lo) for v, idx in srm.peaks(c, 1, top_k, exclusion_samples)]  # w = 1: lag = index


def report(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, split_penalty, max_step, step_cost,
           top_k=3, exclusion_samples=300, n11_blocks=None):
    """((block offsets, block scores, jump flags, total) of drift_model.solve, SEGMENT_REPORT_DTYPE records of the
    segments, their path curves)."""
    k, w = int(block_samples), int(max_offset_samples)
    S = np.asarray(sb).size
    if n11_blocks is None:
        n11_blocks = sm.block_counts(rb, sb, k, w)
    m = sm.block_scores(rb, sb, ref_levels, sub_levels, k, w, n11=n11_blocks)
    offsets, scores, jump, total = dm.solve(None, None, None, None, k, w, split_penalty, max_step, step_cost, m=m)
    segs = segments_of(jump)
    recs = np.zeros(len(segs), dtype=_native.SEGMENT_REPORT_DTYPE)
    curves = []
    for i, (f, e) in enumerate(segs):
        o = offsets[f:e]
        o_min, o_max = int(o.min()), int(o.max())
        d_lo, d_hi = -w + 1 - o_min, w - o_max
        c = path_curve(rb, sb, ref_levels, sub_levels, k, w, f, e, offsets, n11_blocks)
        curves.append(c)
        lo, hi = f * k, min(e * k, S)
        mean, std, flags = srm.moments(c)
        pk = shift_peaks(c, d_lo, top_k, exclusion_samples)
        q = srm.piece_curve(rb, sb, ref_levels, sub_levels, k, w, lo, hi, n11_blocks[f:e].sum(axis=0))
        qs = q[o_min + w - 1:o_max + w]
        flat_j = qs.size - 1 - int(np.argmax(qs[::-1]))

        def at(delta):
            return c[delta - d_lo] if d_lo <= delta <= d_hi else np.nan

        rec = recs[i]
        rec["first_block"], rec["end_block"], rec["start_sample"], rec["end_sample"] = f, e, lo, hi
        rec["first_offset"], rec["last_offset"], rec["min_offset"], rec["max_offset"] = int(o[0]), int(o[-1]), o_min, o_max
        rec["own_score"] = at(0)
        rec["prev_score"] = at(int(offsets[f - 1]) - int(o[0])) if i > 0 else np.nan
        rec["next_score"] = at(int(offsets[e]) - int(o[-1])) if i + 1 < len(segs) else np.nan
        rec["flat_score"], rec["flat_offset"] = qs[flat_j], o_min + flat_j
        rec["mean"], rec["std"], rec["n_lags"] = mean, std, c.size
        for z, (ps_, sh) in enumerate(pk):
            rec["peak_score"][z], rec["peak_shift"][z] = ps_, sh
        rec["n_peaks"] = len(pk)
        rec["flags"] = flags | (OWN_NOT_PEAK if not pk or pk[0][1] != 0 else 0)
    return (offsets, scores, jump, float(total)), recs, curves
