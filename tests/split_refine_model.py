"""TEST INFRASTRUCTURE ONLY -- numpy model of sample-exact break refinement (csrc/ffs_split_refine.h,
ffsubsync_amd.split_refine): the contract the device is held to, bit for bit.

Per break j at c_j = f_j K between the offsets o_a (block f_j - 1) and o_b (block f_j), in the window [L, U]:
  A(t) = split_model's fp64 score of the counts of subtitle samples [L, t) at lag o_a, B(t) of [t, U) at lag o_b
  N(t) = n0 * z0 + n1 * z1 over [L, t), z_x = s~_x * rbar + beta * |s~_x|, rbar = ((R - P1) r~_0 + P1 r~_1) / R
  F = A - N, G = N + B; t2 = first argmax of G(t) + max_{t' <= t} F(t'), t1 = first argmax of F on [L, t2]
  beta None: t1 = t2 = first argmax of A + B
numpy rounds every elementwise product and sum on its own, so every value is the device's.  The records are
``_native.BREAK_REFINE_DTYPE`` arrays.
"""
import numpy as np

import split_model as sm
from ffsubsync_amd import _native

CLIPPED, AT_EDGE, UNMATCHED = 1, 2, 4


def _mix(c, ov, n11, n1x, nx1):
    c00, c01, c10, c11 = c
    n10 = n1x - n11
    n01 = nx1 - n11
    n00 = ov - n11 - n10 - n01
    f = lambda x: np.asarray(x).astype(np.float64)
    return ((f(n00) * c00 + f(n01) * c01) + f(n10) * c10) + f(n11) * c11


def breaks_of(block_offsets):
    """Blocks f with o_f != o_{f-1}."""
    o = np.asarray(block_offsets, dtype=np.int64)
    return [int(b) for b in np.flatnonzero(o[1:] != o[:-1]) + 1]


def windows(cuts, S, radius):
    """[(L, U, clipped)] of the cuts c_1 < ... < c_n."""
    out = []
    n = len(cuts)
    for j, c in enumerate(cuts):
        clipped = False
        lo, hi = c - radius, c + radius
        if j == 0:
            lo = max(lo, 0)
        else:
            mid = (cuts[j - 1] + c) // 2
            if mid > lo:
                lo, clipped = mid, True
        if j + 1 == n:
            hi = min(hi, S)
        else:
            mid = (c + cuts[j + 1]) // 2
            if mid < hi:
                hi, clipped = mid, True
        out.append((lo, hi, clipped))
    return out


def _prefix_counts(r, s, lo, hi, lag):
    """(ov, n11, n1x, nx1) over [lo, t) for t = lo .. hi, int64 arrays of hi - lo + 1."""
    R = r.size
    i = np.arange(lo, hi, dtype=np.int64)
    pres = (i + lag >= 0) & (i + lag < R)
    rv = np.zeros(i.size, bool)
    rv[pres] = r[i[pres] + lag]
    sv = s[lo:hi]
    cs = lambda x: np.concatenate([[0], np.cumsum(x.astype(np.int64))])
    return cs(pres), cs(sv & rv), cs(sv & pres), cs(rv)


def constants(rb, ref_levels, sub_levels, beta):
    """(c00, c01, c10, c11), z0, z1 of a pair (z = 0 for a single cut)."""
    r = np.asarray(rb) != 0
    s0, s1 = sm._pm1(sub_levels[0]), sm._pm1(sub_levels[1])
    r0, r1 = sm._pm1(ref_levels[0]), sm._pm1(ref_levels[1])
    c = (s0 * r0, s0 * r1, s1 * r0, s1 * r1)
    R = r.size
    p1 = int(r.sum())
    rbar = (np.float64(R - p1) * r0 + np.float64(p1) * r1) / np.float64(R)
    bz = np.float64(0.0 if beta is None else beta)
    return c, s0 * rbar + bz * np.abs(s0), s1 * rbar + bz * np.abs(s1)


def curves(rb, sb, ref_levels, sub_levels, lo, hi, oa, ob, beta):
    """(A, B, N) over t = lo .. hi."""
    r, s = np.asarray(rb) != 0, np.asarray(sb) != 0
    c, z0, z1 = constants(r, ref_levels, sub_levels, beta)
    pa = _prefix_counts(r, s, lo, hi, oa)
    pb = _prefix_counts(r, s, lo, hi, ob)
    A = _mix(c, *pa)
    B = _mix(c, *[x[-1] - x for x in pb])
    n1 = np.concatenate([[0], np.cumsum(s[lo:hi].astype(np.int64))])
    n0 = np.arange(hi - lo + 1, dtype=np.int64) - n1
    N = n0.astype(np.float64) * z0 + n1.astype(np.float64) * z1
    return A, B, N


def cut(A, B, N, single):
    """(i1, i2, objective) as window indices (t - L)."""
    if single:
        h = A + B
        i = int(np.argmax(h))
        return i, i, h[i]
    F = A - N
    G = N + B
    before = np.concatenate([[-np.inf], np.maximum.accumulate(F)[:-1]])
    idx = np.maximum.accumulate(np.where(F > before, np.arange(F.size), 0))  # first maximiser of F[:t + 1]
    H = G + F[idx]
    i2 = int(np.argmax(H))
    return int(idx[i2]), i2, H[i2]


def refine(rb, sb, ref_levels, sub_levels, block_offsets, block_samples, radius, beta):
    """BREAK_REFINE_DTYPE records of one pair's breaks (beta None = a single cut)."""
    S = np.asarray(sb).size
    k = int(block_samples)
    o = np.asarray(block_offsets, dtype=np.int64)
    fb = breaks_of(o)
    cuts = [b * k for b in fb]
    recs = np.zeros(len(fb), dtype=_native.BREAK_REFINE_DTYPE)
    for j, (b, c, (lo, hi, clipped)) in enumerate(zip(fb, cuts, windows(cuts, S, int(radius)))):
        oa, ob = int(o[b - 1]), int(o[b])
        A, B, N = curves(rb, sb, ref_levels, sub_levels, lo, hi, oa, ob, beta)
        i1, i2, obj = cut(A, B, N, beta is None)
        t1, t2 = lo + i1, lo + i2
        flags = (CLIPPED if clipped else 0) | (AT_EDGE if (t1 == lo and lo > 0) or (t2 == hi and hi < S) else 0) \
            | (UNMATCHED if t1 < t2 else 0)
        rec = recs[j]
        rec["block"], rec["cut"], rec["lo"], rec["hi"], rec["t1"], rec["t2"] = b, c, lo, hi, t1, t2
        rec["offset_prev"], rec["offset_next"] = oa, ob
        rec["coarse_score"] = A[c - lo] + B[c - lo]
        rec["refined_score"] = obj
        rec["flags"] = flags
    return recs


def brute(rb, sb, ref_levels, sub_levels, lo, hi, oa, ob, beta):
    """(t1, t2, objective) by direct counting at every t and an O(n^2) search over every t1 <= t2: the largest
    objective, the smallest t2 that reaches it, then the smallest maximiser of F on [L, t2] (the contract's tie rules)."""
    r, s = np.asarray(rb) != 0, np.asarray(sb) != 0
    c, z0, z1 = constants(r, ref_levels, sub_levels, beta)
    R = r.size

    def score(x0, x1, lag):
        ov = n11 = n1x = nx1 = 0
        for i in range(x0, x1):
            if 0 <= i + lag < R:
                ov += 1
                n1x += int(s[i])
                nx1 += int(r[i + lag])
                n11 += int(s[i] and r[i + lag])
        return _mix(c, ov, n11, n1x, nx1)[()]

    n = hi - lo + 1
    A = [score(lo, lo + i, oa) for i in range(n)]
    B = [score(lo + i, hi, ob) for i in range(n)]
    if beta is None:
        best = None
        for i in range(n):
            v = A[i] + B[i]
            if best is None or v > best[2]:
                best = (lo + i, lo + i, v)
        return best
    N = []
    for i in range(n):
        n1 = int(s[lo:lo + i].sum())
        N.append(np.float64(i - n1) * z0 + np.float64(n1) * z1)
    vals = {}
    for i2 in range(n):
        g = N[i2] + B[i2]
        for i1 in range(i2 + 1):
            vals[(i1, i2)] = g + (A[i1] - N[i1])
    top = max(vals.values())
    i2 = min(j for (_, j), v in vals.items() if v == top)
    F = [A[i] - N[i] for i in range(i2 + 1)]
    i1 = F.index(max(F))
    return lo + i1, lo + i2, vals[(i1, i2)]


def sub_cues(sub01):
    """(start, end) sample arrays of the runs of ones of a subtitle vector: the workload's cues."""
    s = np.concatenate([[0], (np.asarray(sub01) != 0).astype(np.int8), [0]])
    d = np.diff(s)
    return np.flatnonzero(d == 1).astype(np.int64), np.flatnonzero(d == -1).astype(np.int64)


def cue_errors(problem, cue_start, cue_offset, cue_unmatched, offset_tol=2):
    """Counts of a cue mapping against a workloads/splits.py problem's truth, by each cue's start sample: a start inside
    a removal's interval [lo, hi) belongs nowhere (a cut cue); any other start belongs to the piece after the events
    with hi <= start.  wrong = matched cues outside cut stretches mapped to an offset more than ``offset_tol`` from
    their piece's; found = cut cues marked unmatched; false = other cues marked unmatched."""
    start = np.asarray(cue_start, dtype=np.int64)
    lo = np.array([b[0] for b in problem.breaks], dtype=np.int64)
    hi = np.array([b[1] for b in problem.breaks], dtype=np.int64)
    in_cut = ((start[:, None] >= lo[None, :]) & (start[:, None] < hi[None, :])).any(axis=1) if lo.size else \
        np.zeros(start.size, bool)
    piece = (start[:, None] >= hi[None, :]).sum(axis=1) if lo.size else np.zeros(start.size, np.int64)
    want = np.asarray(problem.offsets, dtype=np.int64)[piece]
    um = np.asarray(cue_unmatched, dtype=bool)
    wrong = ~in_cut & ~um & (np.abs(np.asarray(cue_offset, dtype=np.int64) - want) > offset_tol)
    return dict(cues=int(start.size), cut_cues=int(in_cut.sum()), wrong=int(wrong.sum()), found=int((in_cut & um).sum()),
                false=int((~in_cut & um).sum()))
