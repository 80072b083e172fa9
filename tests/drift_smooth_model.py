"""TEST INFRASTRUCTURE ONLY -- numpy model of the smooth drift fit (csrc/ffs_drift_smooth.h, ffsubsync_amd.drift_smooth),
built on tests/drift_model.py, drift_report_model.py and split_model.py: the contract the device is held to, bit for bit.

Inputs: a drift solve (block offsets o_b, jump flags, the block counts) and knot_blocks M in [1, 256], radius R in
[0, 16], bend_cost lambda (finite, >= 0).  Per segment [f, e) of the solve (drift_report_model.segments_of):
  - a one-block segment is returned as it is: its block is its only knot, fit_total = line_score = bend_total = 0.0
  - knots, n = e - 1 - f >= 1: I = max(1, (n + M // 2) // M) intervals, k_i = f + i M for i < I, k_I = e - 1; interval i
    has n_i = k_{i+1} - k_i blocks and holds the blocks k_i <= b < k_{i+1}, the last interval b = k_I too
  - candidates: knot i at lag c_i = o_{k_i} + u, u in [-R, R], valid where -W + 1 <= c_i <= W
  - digital line: block b of interval i has lag d_b = c_i + floor((2 (c_{i+1} - c_i) (b - k_i) + n_i) / (2 n_i)), int64
  - line score T_i(c_i, c_{i+1}): ov / n1x / nx1 / n11 of drift_report_model's path curve summed as exact integers over
    the interval's blocks at their lags d_b, then ONE split_mix expression, exactly 0.0 where the overlap is empty;
    -inf where either end is not a valid candidate
  - bend cost at the interior knot i: g = |D2 n_a - D1 n_b| (int64; D1 = c_i - c_{i-1} over n_a blocks, D2 = c_{i+1} - c_i
    over n_b), then ((lambda * float(g)) * float(M)) / float(n_a n_b), each operation rounded on its own
  - optimum by a Viterbi pass over the state (c_{i-1}, c_i):  V_1 = T_0;  for i = 1 .. I-1
        V_{i+1}(c_i, c_{i+1}) = max over c_{i-1} of (V_i(c_{i-1}, c_i) - bend_i(c_{i-1}, c_i, c_{i+1}))  +  T_i(c_i, c_{i+1})
    fit_total = max of V_I.
THE TIE RULE, once: candidates are tried in the order u = 0, +1, -1, +2, -2, ... and one replaces the best so far only
when it is strictly greater -- over the predecessor c_{i-1} at every step, and over the final state with u_I as the outer
and u_{I-1} as the inner loop.  Ties stay on the path.
  - line_score = the chosen T_i summed in interval order from 0.0; bend_total = the chosen bend costs in knot order from
    0.0 (fit_total is the Viterbi value itself, NOT line_score - bend_total recomputed).
Records are ``_native.SMOOTH_SEGMENT_DTYPE`` arrays.
"""
import itertools

import numpy as np

import drift_model as dm
import drift_report_model as drm
import split_model as sm
from ffsubsync_amd import _native

MAX_KNOT_BLOCKS = 256
MAX_RADIUS = 16


def validate(knot_blocks, radius, bend_cost):
    m, r = int(knot_blocks), int(radius)
    if m != knot_blocks or not 1 <= m <= MAX_KNOT_BLOCKS:
        raise ValueError("knot_blocks=%r: need an integer in [1, %d]" % (knot_blocks, MAX_KNOT_BLOCKS))
    if r != radius or not 0 <= r <= MAX_RADIUS:
        raise ValueError("radius=%r: need an integer in [0, %d]" % (radius, MAX_RADIUS))
    lam = float(bend_cost)
    if not np.isfinite(lam) or lam < 0:
        raise ValueError("bend_cost=%r: need a finite number >= 0" % (bend_cost,))
    return m, r, np.float64(lam)


def tie_order(radius):
    """u = 0, +1, -1, +2, -2, ..., +R, -R."""
    out = [0]
    for a in range(1, int(radius) + 1):
        out += [a, -a]
    return out


def knots_of(first_block, end_block, knot_blocks):
    """Knot blocks [k_0, ..., k_I] of the segment [first_block, end_block); [first_block] for a one-block segment."""
    f, e, m = int(first_block), int(end_block), int(knot_blocks)
    n = e - 1 - f
    if n < 1:
        return [f]
    intervals = max(1, (n + m // 2) // m)
    return [f + i * m for i in range(intervals)] + [e - 1]


def digital_line(c0, c1, n, j):
    """Lag of the block j blocks after a knot at lag c0, the next knot n blocks on at lag c1 (int64 arrays or ints)."""
    c0, c1, j = np.asarray(c0, np.int64), np.asarray(c1, np.int64), np.asarray(j, np.int64)
    return c0 + (2 * (c1 - c0) * j + n) // (2 * n)  # numpy's // floors for either sign


class Counts:
    """What the line scores read: the block counts, the prefix popcounts of both vectors and the score coefficients."""

    def __init__(self, rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, n11_blocks=None):
        r = (np.asarray(rb) != 0).astype(np.int64)
        s = (np.asarray(sb) != 0).astype(np.int64)
        self.R, self.S = r.size, s.size
        self.k, self.w = int(block_samples), int(max_offset_samples)
        self.n11 = sm.block_counts(r, s, self.k, self.w) if n11_blocks is None else n11_blocks
        self.ps = np.concatenate([[0], np.cumsum(s)])
        self.pr = np.concatenate([[0], np.cumsum(r)])
        self.coeffs = drm._coeffs(ref_levels, sub_levels)
        self.n_blocks = self.n11.shape[0]

    def valid(self, lag):
        return (lag >= -self.w + 1) & (lag <= self.w)

    def block_terms(self, b, lag):
        """(ov, n11, n1x, nx1) of block b at the lags ``lag`` (int64 array, every one inside the window)."""
        blo, bhi = b * self.k, min((b + 1) * self.k, self.S)
        a = np.maximum(blo, -lag)
        e = np.minimum(bhi, self.R - lag)
        ok = e > a
        a = np.where(ok, a, 0)
        e = np.where(ok, e, 0)
        n11 = np.where(ok, self.n11[b, lag + (self.w - 1)], 0)
        nx1 = np.where(ok, self.pr[np.clip(e + lag, 0, self.R)] - self.pr[np.clip(a + lag, 0, self.R)], 0)
        return e - a, n11, self.ps[e] - self.ps[a], nx1


def line_table(cnt, offsets, k0, n, last, radius):
    """T[u_i + R, u_{i+1} + R] of the interval that starts at knot block k0 and has n blocks (and block k0 + n too when
    ``last``); -inf where an end is not a valid candidate."""
    r = int(radius)
    u = np.arange(-r, r + 1, dtype=np.int64)
    c0 = (int(offsets[k0]) + u)[:, None] + 0 * u[None, :]
    c1 = (int(offsets[k0 + n]) + u)[None, :] + 0 * u[:, None]
    ok = cnt.valid(c0) & cnt.valid(c1)
    c0s, c1s = np.where(ok, c0, int(offsets[k0])), np.where(ok, c1, int(offsets[k0 + n]))  # u = 0 where invalid: in range
    ov = np.zeros(c0.shape, np.int64)
    n11, n1x, nx1 = ov.copy(), ov.copy(), ov.copy()
    for j in range(n + (1 if last else 0)):
        t = cnt.block_terms(k0 + j, digital_line(c0s, c1s, n, j))
        ov += t[0]
        n11 += t[1]
        n1x += t[2]
        nx1 += t[3]
    return np.where(ok, drm._mix(ov, n11, n1x, nx1, cnt.coeffs), -np.inf)


def bend_table(offsets, ka, na, nb, knot_blocks, radius, bend_cost):
    """bend[u_{i-1} + R, u_i + R, u_{i+1} + R] at the knot ka + na between an interval of na blocks from ka and one of nb."""
    r = int(radius)
    u = np.arange(-r, r + 1, dtype=np.int64)
    ca = int(offsets[ka]) + u[:, None, None]
    cb = int(offsets[ka + na]) + u[None, :, None]
    cc = int(offsets[ka + na + nb]) + u[None, None, :]
    g = np.abs((cc - cb) * na - (cb - ca) * nb)
    return ((np.float64(bend_cost) * g.astype(np.float64)) * np.float64(knot_blocks)) / np.float64(na * nb)


def viterbi(tables, bends, radius):
    """(fit_total, [u_0 .. u_I]) over line tables T_0 .. T_{I-1} and bend tables bend_1 .. bend_{I-1}, ties as stated."""
    r = int(radius)
    order = np.array(tie_order(r), dtype=np.int64) + r  # candidate indices in the order they are tried
    v = tables[0]
    back = []
    for t, bend in zip(tables[1:], bends):
        cand = (v[:, :, None] - bend)[order]  # [rank of u_{i-1}, u_i, u_{i+1}]
        rank = np.argmax(cand, axis=0)  # the first maximum in the order tried
        back.append(order[rank])
        v = np.take_along_axis(cand, rank[None], axis=0)[0] + t
    fin = v[order][:, order].T  # [rank of u_I, rank of u_{I-1}]
    q = int(np.argmax(fin))
    b, a = order[q // order.size], order[q % order.size]  # u_I (outer), u_{I-1} (inner)
    total = v[a, b]
    path = [b, a]
    for arg in reversed(back):
        a, b = arg[a, b], a
        path.append(a)
    return total, [int(x) - r for x in reversed(path)]


def fit_segment(cnt, offsets, first_block, end_block, knot_blocks, radius, bend_cost, tables=None):
    """(smooth offsets of the segment's blocks, knot blocks, knot lags, fit_total, line_score, bend_total)."""
    m, r, lam = validate(knot_blocks, radius, bend_cost)
    f, e = int(first_block), int(end_block)
    ks = knots_of(f, e, m)
    if len(ks) == 1:
        return np.array([int(offsets[f])], np.int64), ks, [int(offsets[f])], 0.0, 0.0, 0.0
    n_int = len(ks) - 1
    ns = [ks[i + 1] - ks[i] for i in range(n_int)]
    if tables is None:
        tables = [line_table(cnt, offsets, ks[i], ns[i], i == n_int - 1, r) for i in range(n_int)]
    bends = [bend_table(offsets, ks[i - 1], ns[i - 1], ns[i], m, r, lam) for i in range(1, n_int)]
    total, us = viterbi(tables, bends, r)
    lags = [int(offsets[k]) + u for k, u in zip(ks, us)]
    line = np.float64(0.0)
    for i in range(n_int):
        line = line + tables[i][us[i] + r, us[i + 1] + r]
    bend = np.float64(0.0)
    for i in range(1, n_int):
        bend = bend + bends[i - 1][us[i - 1] + r, us[i] + r, us[i + 1] + r]
    out = np.zeros(e - f, np.int64)
    for i in range(n_int):
        j = np.arange(ns[i] + (1 if i == n_int - 1 else 0), dtype=np.int64)
        out[ks[i] - f + j] = digital_line(lags[i], lags[i + 1], ns[i], j)
    return out, ks, lags, float(total), float(line), float(bend)


def fit(cnt, offsets, jump, knot_blocks, radius, bend_cost, table_cache=None):
    """(smooth_offset [B] int64, knot [B] uint8, SMOOTH_SEGMENT_DTYPE records of the segments) of a drift solve.
    ``table_cache``: a dict that keeps the line tables per (segment, M, R) across calls that differ in bend_cost only."""
    m, r, _ = validate(knot_blocks, radius, bend_cost)
    offsets = np.asarray(offsets, dtype=np.int64)
    segs = drm.segments_of(jump)
    smooth = np.zeros(offsets.size, np.int64)
    knot = np.zeros(offsets.size, np.uint8)
    recs = np.zeros(len(segs), dtype=_native.SMOOTH_SEGMENT_DTYPE)
    for i, (f, e) in enumerate(segs):
        tables = None
        if table_cache is not None and e - f > 1:
            key = (f, e, m, r)
            if key not in table_cache:
                ks = knots_of(f, e, m)
                table_cache[key] = [line_table(cnt, offsets, ks[q], ks[q + 1] - ks[q], q == len(ks) - 2, r)
                                    for q in range(len(ks) - 1)]
            tables = table_cache[key]
        so, ks, _, total, line, bend = fit_segment(cnt, offsets, f, e, m, r, bend_cost, tables)
        smooth[f:e] = so
        knot[ks] = 1
        recs[i]["fit_total"], recs[i]["line_score"], recs[i]["bend_total"], recs[i]["n_knots"] = total, line, bend, len(ks)
    return smooth, knot, recs


def solve(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, split_penalty, max_step, step_cost,
          knot_blocks, radius, bend_cost, n11_blocks=None):
    """((block offsets, block scores, jump flags, total) of drift_model.solve, smooth offsets, knot flags, records)."""
    cnt = Counts(rb, sb, ref_levels, sub_levels, block_samples, max_offset_samples, n11_blocks)
    mtab = sm.block_scores(rb, sb, ref_levels, sub_levels, cnt.k, cnt.w, n11=cnt.n11)
    drift = dm.solve(None, None, None, None, cnt.k, cnt.w, split_penalty, max_step, step_cost, m=mtab)
    smooth, knot, recs = fit(cnt, drift[0], drift[2], knot_blocks, radius, bend_cost)
    return drift, smooth, knot, recs


# ---- slow references for the tests ----------------------------------------------------------------------------------

def brute_line_score(rb, sb, ref_levels, sub_levels, block_samples, blocks, lags):
    """One line's score by direct counting: block b of ``blocks`` against the reference at its lag (no block counts, no
    prefix sums)."""
    r = np.asarray(rb) != 0
    s = np.asarray(sb) != 0
    k = int(block_samples)
    ov = n11 = n10 = n01 = 0
    for b, d in zip(blocks, lags):
        a, e = max(b * k, -d), min((b + 1) * k, s.size, r.size - d)
        if e <= a:
            continue
        x, y = s[a:e], r[a + d:e + d]
        ov += e - a
        n11 += int(np.sum(x & y))
        n10 += int(np.sum(x & ~y))
        n01 += int(np.sum(~x & y))
    if not ov:
        return 0.0
    c00, c01, c10, c11 = drm._coeffs(ref_levels, sub_levels)
    n00 = ov - n11 - n10 - n01
    return ((np.float64(n00) * c00 + np.float64(n01) * c01) + np.float64(n10) * c10) + np.float64(n11) * c11


def brute_force_total(tables, bends, radius):
    """Maximum of sum T_i - sum bend_i over ALL knot lags by exhaustive enumeration (tiny problems; real-number sums, so
    compare on tables whose arithmetic is exact)."""
    s = 2 * int(radius) + 1
    best = -np.inf
    for us in itertools.product(range(s), repeat=len(tables) + 1):
        tot = 0.0
        for i, t in enumerate(tables):
            tot += t[us[i], us[i + 1]]
        for i, bd in enumerate(bends):
            tot -= bd[us[i], us[i + 1], us[i + 2]]
        best = max(best, tot)
    return best
