"""TEST INFRASTRUCTURE ONLY -- an independent reference for the optimum the drift aligners promise
(ffsubsync_amd/drift_align.py, drift_range.py; the smooth fits of drift_smooth.py and drift_range_smooth.py by
definition).

The drift models (drift_model, drift_range_model, drift_smooth_model) restate the kernels' recurrence, their block-score
table and their backtrack, so a mistake they share goes unseen.  This module shares nothing with them.  It stands on
``piecewise_reference.Reference``, whose ``rows[b, j]`` are the block scores I_b(d) from their definition (mapped levels
2 * level - 1, direct sums or an integer FFT rounded to integers, samples outside the reference absent, 0 where the
overlap is empty), and states the drift objective over LAG PATHS:

    objective(o, jump) = sum_b rows[b, o_b] - sum_{b >= 1} cost_b
    cost_b = P where the solver flags block b as a jump, else Q * |o_b - o_(b-1)|

An unflagged transition of more than max_step lags is a defect, and so is a flagged one that does not move (the
contract's strict ``T > top`` cannot produce one for P >= 0).  The optimum is

    max over all lag paths of sum_b rows[b, o_b] - sum_{b >= 1} c(o_b - o_(b-1))
    c(0) = 0,  c(D) = min(Q |D|, P) for 0 < |D| <= s,  c(D) = P otherwise

P = inf, and DBL_MAX treated as inf, meaning "never".  It is found by a BACKWARD pass (last block to first, the
value-to-go W_b[j] = rows[b, j] + max_j' (W_(b+1)[j'] - c(j' - j))), not the kernels' forward lag-state recurrence
with its option order, in two forms that check each other: a dense one that builds the L x L cost matrix from c
literally, and a banded one (shifted maxima plus one global maximum) for any L; a small enumerator of all L^B paths
checks both.  No tie rule exists here: only the optimal VALUE is compared, a solver's path is checked through its
objective.

Exactness.  With integer mapped levels and dyadic P and Q every quantity is an integer multiple of a small power of two
below 2^53, every sum is exact in any order, and the checks are equalities.  Otherwise ``tolerance`` bounds what two
correct fp64 evaluations of one path can differ by, the way ``Reference.tolerance`` does: a sum of B block scores and
B - 1 costs makes fewer than 2B additions, each rounded within eps of a partial sum that is at most sum|terms| + the
costs paid; a block score itself is within 3 eps of its real sum; so 8 eps B (sum|terms| + costs) covers both sides
with room.  The costs: a path that pays more than 2 sum|products| in transitions scores below the constant path
(every path's rows sum to within +-sum|products|), so an optimal path pays at most min((B - 1) max(P, Q s),
2 sum|products|).  The bound is this reference's own property; it is never tuned on a solver's output.
"""
import itertools
import math
import sys

import numpy as np

import piecewise_reference as pw

EPS = pw.EPS
DBL_MAX = sys.float_info.max
DENSE_LAGS = 2048  # the dense form builds an L x L matrix


def penalty_of(split_penalty):
    """P as a float, DBL_MAX as inf ("never")."""
    p = float(split_penalty)
    return math.inf if p >= DBL_MAX else p


def cost(delta, P, s, Q):
    """c(delta) of the optimum's definition."""
    a = abs(int(delta))
    p = penalty_of(P)
    if a == 0:
        return 0.0
    if a <= int(s):
        return min(float(Q) * a, p)
    return p


def dense_optimum(rows, P, s, Q):
    """(optimal value, W_0) by the backward pass over the literal L x L cost matrix."""
    rows = np.asarray(rows, dtype=np.float64)
    B, L = rows.shape
    assert L <= DENSE_LAGS, L
    by_delta = np.array([cost(d, P, s, Q) for d in range(L)])  # c is even
    j = np.arange(L)
    C = by_delta[np.abs(j[:, None] - j[None, :])]  # C[j, j']
    w = rows[B - 1].copy()
    for b in range(B - 2, -1, -1):
        w = rows[b] + np.max(w[None, :] - C, axis=1)
    return float(np.max(w)), w


def _step(f, p, s, q):
    """max_j' (f[j'] - c(j' - j)) for every j (c is even, so this serves a pass in either direction)."""
    L = f.size
    out = f.copy()
    if math.isfinite(p):
        out = np.maximum(out, float(np.max(f)) - p)
    for a in range(1, s + 1):
        if a >= L:
            break
        out[:L - a] = np.maximum(out[:L - a], f[a:] - q * a)
        out[a:] = np.maximum(out[a:], f[:L - a] - q * a)
    return out


def banded_optimum(rows, P, s, Q):
    """(optimal value, W_0) by the backward pass with shifted maxima: the successor sits at the same lag, at a distance
    a <= s for Q a, or anywhere for P (a move dearer than P loses to that, so min(Q a, P) needs no case of its own)."""
    rows = np.asarray(rows, dtype=np.float64)
    B, L = rows.shape
    p, s, q = penalty_of(P), int(s), float(Q)
    w = rows[B - 1].copy()
    for b in range(B - 2, -1, -1):
        w = rows[b] + _step(w, p, s, q)
    return float(np.max(w)), w


def optimum(rows, P, s, Q):
    """The optimal value, by the banded form (``check_solution`` holds the dense form against it where L allows)."""
    return banded_optimum(rows, P, s, Q)[0]


def enumerate_optimum(rows, P, s, Q, limit=50000):
    """The optimal value over all L^B lag paths of block rows [B, L], one path at a time."""
    rows = np.asarray(rows, dtype=np.float64)
    B, L = rows.shape
    assert L ** B <= limit, (L, B)
    by_delta = [cost(d, P, s, Q) for d in range(L)]
    top = -math.inf
    for path in itertools.product(range(L), repeat=B):
        v = float(rows[0, path[0]])
        for b in range(1, B):
            v = v - by_delta[abs(path[b] - path[b - 1])] + float(rows[b, path[b]])
        top = max(top, v)
    return top


def objective(rows, path, jump, P, s, Q):
    """(objective of the lag-index path with the solver's jump flags, defects): the value from its definition and a list
    of transitions that no solver may return."""
    p, s, q = penalty_of(P), int(s), float(Q)
    total, defects = float(rows[0, path[0]]), []
    for b in range(1, len(path)):
        d = int(path[b]) - int(path[b - 1])
        if jump[b]:
            if d == 0:
                defects.append(("jump that does not move", b))
            total -= p
        else:
            if abs(d) > s:
                defects.append(("unflagged move beyond max_step", b, d))
            total -= q * abs(d)
        total += float(rows[b, path[b]])
    if len(jump) and jump[0]:
        defects.append(("block 0 flagged as a jump", 0))
    return total, defects


def tolerance(ref, P, s, Q):
    """0 on the exact path; otherwise 8 eps B (sum|terms| + costs), see the module docstring."""
    if ref.exact:
        return 0.0
    p = penalty_of(P)
    per = max(p if math.isfinite(p) else 0.0, float(Q) * int(s))
    costs = min(per * max(ref.B - 1, 0), 2.0 * ref.abs_terms)
    return 8.0 * EPS * ref.B * (ref.abs_terms + costs)


def segments_of(jump):
    """[(first_block, end_block)] of the maximal jump-free runs."""
    out, b0 = [], 0
    for b in range(1, len(jump) + 1):
        if b == len(jump) or jump[b]:
            out.append((b0, b))
            b0 = b
    return out


def check_solution(ref, P, s, Q, block_offsets, block_jump, total, block_scores=None, segments=None):
    """Problems with a solver's answer against the reference (empty list = none):
      1. total == the optimum over lag paths (within ``tolerance``);
      2. objective(path, flags) == total, no unflagged move beyond max_step, no jump that stays;
      3. every offset inside the lag set, one per block;
      4. block_scores[b] == rows[b, o_b] (when given);
      5. ``segments`` (when given): [(first_block, end_block, first_offset, last_offset, score)] as the solver reports
         them are the maximal jump-free runs, each score the sum of its blocks' rows."""
    bad = []
    tol = tolerance(ref, P, s, Q)
    want = optimum(ref.rows, P, s, Q)
    if ref.L <= DENSE_LAGS:
        dense = dense_optimum(ref.rows, P, s, Q)[0]
        if not abs(dense - want) <= tol:
            bad.append(("reference: dense != banded", dense, want))
    if not abs(float(total) - want) <= tol:
        bad.append(("total", float(total), want, tol))
    offs = [int(x) for x in block_offsets]
    jump = [int(x) for x in block_jump]
    if len(offs) != ref.B or len(jump) != ref.B:
        return bad + [("blocks", len(offs), len(jump), ref.B)]
    outside = [(b, o) for b, o in enumerate(offs) if not ref.lo <= o <= ref.hi]
    if outside:
        return bad + [("offset outside the lag set", outside[:3])]
    path = [ref.lag_index(o) for o in offs]
    got, defects = objective(ref.rows, path, jump, P, s, Q)
    bad += defects
    if not abs(got - float(total)) <= tol:
        bad.append(("path objective != total", got, float(total), tol))
    if block_scores is not None:
        for b, j in enumerate(path):
            if not abs(float(block_scores[b]) - float(ref.rows[b, j])) <= tol:
                bad.append(("block score", b, offs[b], float(block_scores[b]), float(ref.rows[b, j])))
    if segments is not None:
        runs = segments_of(jump)
        if [(g[0], g[1]) for g in segments] != runs:
            bad.append(("segments", [(g[0], g[1]) for g in segments], runs))
        else:
            for f, e, first, last, score in segments:
                acc = 0.0
                for b in range(f, e):
                    acc += float(ref.rows[b, path[b]])
                if (int(first), int(last)) != (offs[f], offs[e - 1]) or not abs(float(score) - acc) <= tol:
                    bad.append(("segment", f, e, int(first), int(last), float(score), offs[f], offs[e - 1], acc))
    return bad


def path_facts(ref, P, s, Q, block_offsets, block_jump):
    """(moves, jumps, ties) of a solution already known to be optimal: unflagged transitions that move, flagged ones,
    and transitions at which two or more predecessors of (b, o_b) reach the same best value -- an exact STAY, move or
    jump tie on the path (exact problems only; 0 otherwise).  The predecessors' values are the forward values
    F_(b-1)[j'] - c(o_b - j'), F from the same pass over the rows in reverse order (c is even)."""
    offs = [int(x) for x in block_offsets]
    moves = sum(1 for b in range(1, ref.B) if not block_jump[b] and offs[b] != offs[b - 1])
    jumps = sum(1 for b in range(1, ref.B) if block_jump[b])
    ties = 0
    if ref.exact and ref.B > 1:
        p, s, q = penalty_of(P), int(s), float(Q)
        f = ref.rows[0].copy()
        for b in range(1, ref.B):
            j = ref.lag_index(offs[b])
            val = f - p if math.isfinite(p) else np.full(ref.L, -math.inf)
            lo, hi = max(0, j - s), min(ref.L, j + s + 1)
            near = f[lo:hi] - np.minimum(q * np.abs(np.arange(lo, hi) - j), p)
            val[lo:hi] = near  # min(Q a, P) <= P, and a = 0 costs nothing
            ties += int(np.count_nonzero(val == val.max()) >= 2)
            f = _step(f, p, s, q) + ref.rows[b]
    return moves, jumps, ties


# ---- the smooth fits, by the definition in csrc/ffs_drift_smooth.h ---------------------------------------------------

def knots_of(f, e, m):
    """Knot blocks of the segment [f, e): I = max(1, (n + M/2) / M) intervals over n = e - 1 - f, k_i = f + i M for
    i < I, k_I = e - 1; the block itself for a one-block segment."""
    n = e - 1 - f
    if n < 1:
        return [f]
    return [f + i * m for i in range(max(1, (n + m // 2) // m))] + [e - 1]


def digital_line(c0, c1, n, j):
    """d_b = c_i + floor((2 (c_{i+1} - c_i)(b - k_i) + n_i) / (2 n_i)); Python's // floors."""
    return c0 + (2 * (c1 - c0) * j + n) // (2 * n)


def line_sum(ref, k0, n, last, c0, c1):
    """sum of rows[b, d_b] over the interval's blocks (block k0 + n too when it is the segment's last interval)."""
    blocks = range(n + (1 if last else 0))
    return sum(float(ref.rows[k0 + j, ref.lag_index(digital_line(c0, c1, n, j))]) for j in blocks)


def bend(lam, m, d1, d2, na, nb):
    """((lambda * g) * M) / (n_a n_b), g = |D2 n_a - D1 n_b|, every operation rounded on its own."""
    return ((np.float64(lam) * np.float64(abs(d2 * na - d1 * nb))) * np.float64(m)) / np.float64(na * nb)


def check_fit(ref, m, radius, lam, block_offsets, block_jump, smooth_offsets, knot, segments):
    """Problems with a smooth fit of an exact (integer-level) problem, by the definition in csrc/ffs_drift_smooth.h and
    not by its model: ``segments`` = [(first_block, end_block, [(knot block, knot lag)], fit_total, line_score,
    bend_total)].  Returns (problems, multi-knot segments seen, segments whose fit left the path).
      - the segments are the maximal jump-free runs, the knot blocks the header's;
      - knot lags within ``radius`` of the path and inside the lag set; between knots the digital line;
      - line_score == sum of rows[b, smooth_offset_b]; bend_total == the header's bends summed in knot order;
      - fit_total >= the value of the path's own knots (u = 0 everywhere is always a candidate; evaluated in the
        Viterbi pass's order of operations, and fp64 addition and subtraction are monotone, so the maximum the pass
        keeps can never be below it), and <= line_score - bend_total up to rounding;
      - knot_blocks = 1 with radius = 0 returns the path.
    A one-block segment "is returned as it is": its offset is checked, its three sums are not defined by the header."""
    assert ref.exact
    bad, n_fit, n_off = [], 0, 0
    path = [int(x) for x in block_offsets]
    smooth = [int(x) for x in smooth_offsets]
    if [(g[0], g[1]) for g in segments] != segments_of(block_jump):
        return [("segments", [(g[0], g[1]) for g in segments])], 0, 0
    for f, e, knots, fit_total, line_score, bend_total in segments:
        ks = knots_of(f, e, m)
        if [b for b in range(f, e) if knot[b]] != ks or [b for b, _ in knots] != ks:
            bad.append(("knot blocks", f, e, knots, ks))
            continue
        if len(ks) == 1:  # "a one-block segment is returned as it is"
            if smooth[f] != path[f]:
                bad.append(("one-block segment moved", f, smooth[f], path[f]))
            continue
        n_fit += 1
        cs = [c for _, c in knots]
        ns = [ks[i + 1] - ks[i] for i in range(len(ks) - 1)]
        if any(abs(c - path[b]) > radius or not ref.lo <= c <= ref.hi for b, c in zip(ks, cs)):
            bad.append(("knot lag beyond the radius or outside the lag set", f, e, knots, [path[b] for b in ks]))
            continue
        want = []
        for i, n in enumerate(ns):
            want += [digital_line(cs[i], cs[i + 1], n, j) for j in range(n + (1 if i == len(ns) - 1 else 0))]
        if smooth[f:e] != want:
            bad.append(("smooth offsets off the digital line", f, e, smooth[f:e], want))
            continue
        n_off += smooth[f:e] != path[f:e]
        line = sum(float(ref.rows[b, ref.lag_index(smooth[b])]) for b in range(f, e))
        if line_score != line:
            bad.append(("line_score", f, e, line_score, line))
        bends = np.float64(0.0)
        for i in range(1, len(ns)):
            bends = bends + bend(lam, m, cs[i] - cs[i - 1], cs[i + 1] - cs[i], ns[i - 1], ns[i])
        if float(bend_total) != float(bends):
            bad.append(("bend_total", f, e, bend_total, float(bends)))
        # the path's own knots (u = 0 everywhere) are always a candidate: its value in the Viterbi pass's order
        ps = [path[b] for b in ks]
        v = np.float64(line_sum(ref, ks[0], ns[0], len(ns) == 1, ps[0], ps[1]))
        for i in range(1, len(ns)):
            v = (v - bend(lam, m, ps[i] - ps[i - 1], ps[i + 1] - ps[i], ns[i - 1], ns[i])) + \
                np.float64(line_sum(ref, ks[i], ns[i], i == len(ns) - 1, ps[i], ps[i + 1]))
        if not fit_total >= float(v):
            bad.append(("fit_total below the unsmoothed path's own knots", f, e, fit_total, float(v)))
        mag = sum(abs(float(ref.rows[b, ref.lag_index(smooth[b])])) for b in range(f, e)) + float(bends)
        if not fit_total <= line - float(bends) + 4.0 * EPS * len(ns) * mag:  # 2 I operations, each within eps of mag
            bad.append(("fit_total above its own line score minus bends", f, e, fit_total, line, float(bends)))
    if (m, radius) == (1, 0) and smooth != path:
        bad.append(("knot_blocks = 1, radius = 0 left the path", smooth, path))
    return bad, n_fit, n_off


def drifting_bits(rng, R, S, shift, every, break_at=None, break_by=0, flip=0.04, run=40.0):
    """Problems for the tests (not part of the reference): two-level bits, a reference of random runs and a subtitle
    whose sample i follows it at shift + i // every (a negative ``every`` drifts downwards: Python's floor), plus
    ``break_by`` from sample ``break_at`` on, a fraction ``flip`` of its samples inverted; both levels present in
    both.  Optimal paths then hold real moves and, with a break, real jumps."""
    seg = np.maximum(1, rng.geometric(1.0 / run, size=R // 4 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    i = np.arange(S)
    idx = i + int(shift) + i // int(every)
    if break_at is not None:
        idx = idx + np.where(i >= int(break_at), int(break_by), 0)
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < flip
    if S >= 2:
        sb[0], sb[1] = True, False
    rb[0], rb[1] = True, False
    return rb, sb
