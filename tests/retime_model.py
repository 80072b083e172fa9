"""TEST INFRASTRUCTURE ONLY -- numpy model of the joint cue retiming (csrc/ffs_cue_retime.h, ffsubsync_amd.cue_retime):
the contract the device is held to, bit for bit.

Per pair, cues (start, end, lag) in table order = chain order.  Live / skipped cues, the window and the counts at
d = lag + delta are cue_model's; the node score is the INTEGER agreement
  A_k(delta) = ov - 2 n1x - 2 nx1 + 4 n11        (the pair's levels do not enter)          u_k = 64 A_k
Link from live cue k-1 (shift d') to live cue k (shift d): w = penalty_q |d - d'|, capped at jump_q when jump_q >= 0;
g_k = (a_k + lag_k) - (a_{k-1} + lag_{k-1}) from the clamped starts; with keep_order and g_k >= 0 only d' <= d + g_k is
admissible.  V_1 = u_1, V_k(d) = u_k(d) + max over admissible d' of (V_{k-1}(d') - w(d', d)); the backpointer is the
maximising d', delta_K = argmax V_K; every tie goes to the option order on the candidate: smallest |.|, then + over -.

``retime`` is the plain O(K D^2) maximisation straight from these lines, in Python ints.  ``retime_paths`` is a second,
faster evaluation of the same recurrence for the calibration (prefix / suffix / sliding-window maxima in numpy, many
(penalty_q, jump_q) settings at once); tests/test_retime_model_host.py holds it to ``retime``.
"""
import numpy as np

import cue_model as cm

EMPTY, INVALID, MOVED, JUMP, UNORDERED, ORDER_TIGHT, AT_EDGE = 1, 2, 4, 8, 16, 32, 64
KEEP_ORDER = 1
MAX_RADIUS, MAX_CONTEXT, MAX_LAG = 1024, cm.MAX_CONTEXT, cm.MAX_LAG
Q, NO_JUMP, MAX_PENALTY_Q, MAX_JUMP_Q = 64, -1, 1 << 20, 1 << 40

DTYPE = np.dtype(
    [("start", "<i8"), ("end", "<i8"), ("lag", "<i8"), ("delta", "<i4"), ("flags", "<i4"), ("own", "<i4"), ("at", "<i4"),
     ("best", "<i4"), ("best_delta", "<i4"), ("link", "<i8"), ("reserved", "<i4", (2,))]
)
SUMMARY = np.dtype(
    [("total", "<i8"), ("own_total", "<i8"), ("best_total", "<i8"), ("n_live", "<i4"), ("n_moved", "<i4"),
     ("n_jumps", "<i4"), ("reserved", "<i4")]
)
assert DTYPE.itemsize == 64 and SUMMARY.itemsize == 40


def rank(d):
    """Place of a shift in the option order: 0, +1, -1, +2, -2, ..."""
    return 2 * abs(d) - (1 if d > 0 else 0)


def check_args(radius, context, penalty_q, jump_q):
    if not 0 <= radius <= MAX_RADIUS or not 0 <= context <= MAX_CONTEXT:
        raise ValueError("radius or context out of range")
    if not 0 <= penalty_q <= MAX_PENALTY_Q or not (jump_q == NO_JUMP or 0 <= jump_q <= MAX_JUMP_Q):
        raise ValueError("penalty_q or jump_q out of range")


def profiles(pair, cues, radius, context):
    """(flags, pos, A): per cue its skip flags (0 = live), a + lag, and the int64 row A(delta), delta = -rho..rho (zeros
    for a skipped cue)."""
    start, end, lag = (np.asarray(x, dtype=np.int64) for x in cues)
    n = start.size
    flags, pos, A = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, 2 * radius + 1), np.int64)
    delta = np.arange(-radius, radius + 1, dtype=np.int64)
    for k in range(n):
        a, e = min(max(int(start[k]), 0), pair.S), min(max(int(end[k]), 0), pair.S)
        flags[k] = (EMPTY if e <= a else 0) | (INVALID if abs(int(lag[k])) > MAX_LAG else 0)
        if flags[k]:
            continue
        pos[k] = a + int(lag[k])
        L, U = max(0, a - context), min(pair.S, e + context)
        ov, n11, n1x, nx1 = pair.counts(L, U, int(lag[k]) + delta)
        A[k] = ov - 2 * n1x - 2 * nx1 + 4 * n11
    return flags, pos, A


def _records(cues, flags, pos, A, path, radius, penalty_q, jump_q, keep_order, total):
    """The records and the summary of a path over the live cues (``path``: one shift per live cue)."""
    start, end, lag = (np.asarray(x, dtype=np.int64) for x in cues)
    recs, summ = np.zeros(start.size, DTYPE), np.zeros((), SUMMARY)
    recs["start"], recs["end"], recs["lag"], recs["flags"] = start, end, lag, flags
    live = np.flatnonzero(flags == 0)
    if live.size == 0:
        return recs, summ
    deltas = np.arange(-radius, radius + 1)
    for j, k in enumerate(live):
        d, row = int(path[j]), A[k]
        fl, link = 0, 0
        if j:
            dp, g = int(path[j - 1]), int(pos[k] - pos[live[j - 1]])
            link = penalty_q * abs(d - dp)
            if jump_q >= 0 and link > jump_q:
                link, fl = jump_q, fl | JUMP
            if keep_order and g < 0:
                fl |= UNORDERED
            if keep_order and g >= 0 and dp == d + g:
                fl |= ORDER_TIGHT
        if d != 0:
            fl |= MOVED
        if radius > 0 and abs(d) == radius:
            fl |= AT_EDGE
        ib = cm.first_in_option_order(row, deltas)
        recs[k]["delta"], recs[k]["flags"], recs[k]["link"] = d, fl, link
        recs[k]["own"], recs[k]["at"], recs[k]["best"], recs[k]["best_delta"] = row[radius], row[d + radius], row[ib], deltas[ib]
    lv = recs[live]
    summ["total"] = total
    summ["own_total"], summ["best_total"] = Q * int(lv["own"].astype(np.int64).sum()), Q * int(lv["best"].astype(np.int64).sum())
    summ["n_live"], summ["n_moved"] = live.size, int(((lv["flags"] & MOVED) != 0).sum())
    summ["n_jumps"] = int(((lv["flags"] & JUMP) != 0).sum())
    return recs, summ


def retime(r, s, cues, radius, context, penalty_q, jump_q, keep_order=True):
    """(DTYPE records, SUMMARY record) of one pair of 0/1 vectors: the plain maximisation."""
    radius, context, penalty_q, jump_q = int(radius), int(context), int(penalty_q), int(jump_q)
    check_args(radius, context, penalty_q, jump_q)
    pair = cm.Pair(r, s)
    flags, pos, A = profiles(pair, cues, radius, context)
    live = np.flatnonzero(flags == 0)
    shifts = list(range(-radius, radius + 1))
    V, back = None, []
    for j, k in enumerate(live):
        u = [Q * int(x) for x in A[k]]
        if j == 0:
            V = u
            continue
        g = int(pos[k] - pos[live[j - 1]])
        newV, bp = [], []
        for i, d in enumerate(shifts):
            best = None
            for ip, dp in enumerate(shifts):
                if keep_order and g >= 0 and dp > d + g:
                    continue
                w = penalty_q * abs(d - dp)
                if jump_q >= 0:
                    w = min(w, jump_q)
                cand = (V[ip] - w, -rank(dp), dp)
                if best is None or cand[:2] > best[:2]:
                    best = cand
            newV.append(u[i] + best[0])
            bp.append(best[2])
        V = newV
        back.append(bp)
    path, total = [], 0
    if live.size:
        total, _, d = max((V[i], -rank(d), d) for i, d in enumerate(shifts))
        path = [d]
        for bp in reversed(back):
            d = bp[d + radius]
            path.append(d)
        path.reverse()
    return _records(cues, flags, pos, A, path, radius, penalty_q, jump_q, bool(keep_order), total)


# ---- the same recurrence, faster: for the calibration -------------------------------------------------------------------
def _shift_right(x, n, fill):
    """x[..., i + n] at place i (``fill`` past the end)."""
    out = np.full_like(x, fill)
    if n < x.shape[-1]:
        out[..., :x.shape[-1] - n] = x[..., n:]
    return out


def retime_paths(flags, pos, A, radius, settings, keep_order=True):
    """The paths and totals of many (penalty_q, jump_q) ``settings`` over one pair's profiles (``profiles``' output):
    (paths [setting][live cue], totals [setting]).  A candidate is one int64 key, (value << 12) | (4095 - rank), so the
    maximum of keys is the lexicographic maximum of (value, option order); values stay far below 2^50 here."""
    live = np.flatnonzero(flags == 0)
    n_set, D = len(settings), 2 * radius + 1
    if live.size == 0:
        return np.zeros((n_set, 0), np.int64), np.zeros(n_set, np.int64)
    d = np.arange(-radius, radius + 1, dtype=np.int64)
    tag = 4095 - (2 * np.abs(d) - (d > 0))
    pq = np.array([s[0] for s in settings], dtype=np.int64)[:, None]
    jq = np.array([s[1] for s in settings], dtype=np.int64)[:, None]
    capped = jq >= 0
    low = np.int64(-(1 << 62))
    V = np.broadcast_to(Q * A[live[0]], (n_set, D)).copy()
    back = np.zeros((live.size, n_set, D), np.int16)
    for j in range(1, live.size):
        k = live[j]
        g = int(pos[k] - pos[live[j - 1]])
        geff = min(g, 2 * radius) if keep_order and g >= 0 else 2 * radius
        left = np.maximum.accumulate(((V + pq * d) << 12) | tag, axis=1) - ((pq * d) << 12)
        best = left
        x = ((V - pq * d) << 12) | tag
        if geff >= 1:
            jw = geff.bit_length() - 1
            m = x
            for lvl in range(jw):  # m[i] = max x[i .. i + 2^jw - 1]
                m = np.maximum(m, _shift_right(m, 1 << lvl, low))
            right = np.maximum(_shift_right(m, 1, low), _shift_right(m, geff - (1 << jw) + 1, low))
            best = np.maximum(best, np.where(right > low // 2, right + ((pq * d) << 12), low))
        pre = np.maximum.accumulate((V << 12) | tag, axis=1)
        reach = np.minimum(np.arange(D) + geff, D - 1)
        best = np.where(capped, np.maximum(best, pre[:, reach] - (jq << 12)), best)
        rk = 4095 - (best & 4095)  # the winner's place in the option order: odd = +, even = -
        mag = (rk + 1) >> 1
        back[j] = np.where(rk & 1, mag, -mag).astype(np.int16)
        V = Q * A[k] + (best >> 12)
    key = (V << 12) | tag
    last = key.argmax(axis=1)
    totals = V[np.arange(n_set), last]
    paths = np.zeros((n_set, live.size), np.int64)
    cur = d[last]
    paths[:, -1] = cur
    for j in range(live.size - 1, 0, -1):
        cur = back[j, np.arange(n_set), cur + radius].astype(np.int64)
        paths[:, j - 1] = cur
    return paths, totals


def retime_fast(r, s, cues, radius, context, penalty_q, jump_q, keep_order=True):
    """``retime`` through ``retime_paths``: the same records and summary."""
    check_args(int(radius), int(context), int(penalty_q), int(jump_q))
    flags, pos, A = profiles(cm.Pair(r, s), cues, int(radius), int(context))
    paths, totals = retime_paths(flags, pos, A, int(radius), [(int(penalty_q), int(jump_q))], keep_order)
    return _records(cues, flags, pos, A, paths[0], int(radius), int(penalty_q), int(jump_q), bool(keep_order), int(totals[0]))
