"""Numpy model of the subtitle-to-video matching (ffsubsync_amd.match): the matrix and the assignment the device path is
pinned against.

The matrix, per (reference, track) pair:
  - the track rasterised at each framerate ratio (oracle.raster_oracle.rasterize: amplitude min(1/ratio, 1));
  - every candidate's scores over the lag window through ``quality_model.scores``; its best (score, lag) with the largest
    lag on ties (np.argmax's first k, aligners.py:45-48); a candidate whose lag lies beyond the window is dropped
    (MaxScoreAligner's filter); the winner is the FIRST maximum over the ratios; no candidate left: ratio_index -1;
  - ``quality_model.report`` / ``psr_margin`` of the winner.

``scores_sparse`` is the same function as ``quality_model.scores`` with n11 taken from the run boundaries by two running
sums instead of an FFT (exact integers either way; tests/test_match_host.py holds the two against each other): it makes
matrices over hour-long vectors affordable for a test.

The assignment: a pair is trusted when it has a winner, its curve is neither empty nor flat, psr >= min_psr and
margin >= min_margin.  Per subtitle the trusted reference with the largest psr (ties: smaller index); ``exclusive``: trusted
pairs by descending psr, assigned while both sides are free.
"""
import numpy as np

import quality_model as qm
from oracle import raster_oracle as ro
from oracle import runs_model as rm

MIN_PSR, MIN_MARGIN = 5.0, 3.0


def counts_sparse(ref01, sub01, lags):
    """``quality_model.counts`` with n11 from the boundary lists: h(d) = sum over boundary pairs q - p = d of
    db[p] drho[q], g(d+1) = g(d) - h(d), n11(d+1) = n11(d) + g(d+1), started from a direct n11 / g at the first lag."""
    r = (np.asarray(ref01) != 0).astype(np.int64)
    s = (np.asarray(sub01) != 0).astype(np.int64)
    R, S = r.size, s.size
    lags = np.asarray(lags, dtype=np.int64)
    i0 = np.maximum(0, -lags)
    i1 = np.minimum(S, R - lags)
    ov = np.maximum(0, i1 - i0)
    has = ov > 0
    n11 = np.zeros(lags.size, dtype=np.int64)
    if lags.size:
        assert np.all(np.diff(lags) == 1)
        d_lo, d_hi = int(lags[0]), int(lags[-1])
        P = np.flatnonzero(np.diff(np.concatenate([[0], s, [0]])))
        Q = np.flatnonzero(np.diff(np.concatenate([[0], r, [0]])))
        sp = np.where(np.arange(P.size) & 1, -1, 1)
        sq = np.where(np.arange(Q.size) & 1, -1, 1)
        cr = np.concatenate([[0], np.cumsum(r)])
        x = P + d_lo
        n11_0 = -int((sp * cr[np.clip(x, 0, R)]).sum())
        xm = x - 1
        inside = (xm >= 0) & (xm < R)
        g_0 = -int((sp * np.where(inside, r[np.clip(xm, 0, R - 1)], 0)).sum())
        a = np.searchsorted(Q, x, side="left")
        b = np.searchsorted(Q, P + d_hi, side="right")
        cnt = np.maximum(b - a, 0)
        pi = np.repeat(np.arange(P.size), cnt)
        qi = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
        h = np.zeros(lags.size, dtype=np.int64)
        np.add.at(h, Q[qi] - P[pi] - d_lo, sp[pi] * sq[qi])
        g = g_0 - np.concatenate([[0], np.cumsum(h[:-1])])
        n11 = n11_0 + np.concatenate([[0], np.cumsum(g[1:])])
        assert np.all(n11[~has] == 0) and np.all(n11 >= 0)
    cs = np.concatenate([[0], np.cumsum(s)])
    cr = np.concatenate([[0], np.cumsum(r)])
    a, b = np.clip(i0, 0, S), np.clip(i1, 0, S)
    n1x = np.where(has, cs[b] - cs[a], 0)
    nx1 = np.where(has, cr[np.clip(b + lags, 0, R)] - cr[np.clip(a + lags, 0, R)], 0)
    return n11, n1x, nx1, ov


def scores_sparse(ref01, sub01, ref_levels, sub_levels, max_offset_samples):
    """``quality_model.scores`` over ``counts_sparse``."""
    ref01, sub01 = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    lags = qm.lag_set(ref01.size, sub01.size, max_offset_samples)
    n11, n1x, nx1, ov = counts_sparse(ref01, sub01, lags)
    f = lambda v: v.astype(np.float64)
    sc = rm.two_level_scores(f(n11), f(n1x), f(nx1), f(ov), qm._pm1(sub_levels[0]), qm._pm1(sub_levels[1]),
                             qm._pm1(ref_levels[0]), qm._pm1(ref_levels[1]))
    return lags, np.where(ov > 0, sc, 0.0)


def candidates(track, ratios, sample_rate=100):
    """[(0/1 samples, (lo, hi))] of a (start_us, end_us, is_metadata) track at every ratio."""
    start_us, end_us, meta = track
    meta = np.zeros(len(start_us), np.uint8) if meta is None else meta
    out = []
    for ratio in ratios:
        v = ro.rasterize(start_us, end_us, meta, ratio, sample_rate)
        out.append((v != 0, (0.0, min(1.0 / ratio, 1.0))))
    return out


def pair_entry(ref01, ref_levels, cands, w, top_k=3, exclusion_samples=300, scores=qm.scores):
    """dict(ratio_index, offset, score, psr, margin, flags, report) of one pair (ratio_index -1: no winner)."""
    best = None
    for k, (sub01, lv) in enumerate(cands):
        lags, sc = scores(ref01, sub01, ref_levels, lv, w)
        if lags.size == 0:
            continue
        top = sc.max()
        lag = int(lags[np.flatnonzero(sc == top)[-1]])
        if w is not None and abs(lag) > w:
            continue
        if best is None or top > best[0]:
            best = (float(top), lag, k, lags, sc)
    if best is None:
        return dict(ratio_index=-1, offset=0, score=0.0, psr=float("nan"), margin=float("nan"), flags=0, report=None)
    top, lag, k, lags, sc = best
    mean, std, flags = qm.moments(sc)
    rep = dict(peaks=qm.peaks(lags, sc, top_k, exclusion_samples), mean=mean, std=std, n_lags=int(lags.size), flags=flags)
    psr, margin = qm.psr_margin(rep)
    if rep["std"] == 0 or not rep["peaks"]:
        flags |= qm.FLAT
    assert rep["peaks"][0] == (top, lag)
    return dict(ratio_index=k, offset=lag, score=top, psr=psr, margin=margin, flags=flags, report=rep)


def matrix(refs01, tracks, w, ratios, top_k=3, exclusion_samples=300, ref_levels=None, scores=qm.scores, pairs=None):
    """The [N, M] arrays of ``ffsubsync_amd.match.MatchMatrix`` as a dict, plus ``reports`` (N x M nested lists)."""
    n, m = len(refs01), len(tracks)
    cands = [candidates(t, ratios) for t in tracks]
    out = dict(ratio_index=np.full((n, m), -1, np.int64), offset=np.zeros((n, m), np.int64), score=np.zeros((n, m)),
               psr=np.full((n, m), np.nan), margin=np.full((n, m), np.nan), flags=np.zeros((n, m), np.int32),
               reports=[[None] * m for _ in range(n)])
    todo = [(i, j) for i in range(n) for j in range(m)] if pairs is None else [(int(i), int(j)) for i, j in pairs]
    for i, j in todo:
        lv = (0.0, 1.0) if ref_levels is None else ref_levels[i]
        e = pair_entry(np.asarray(refs01[i]) != 0, lv, cands[j], w, top_k, exclusion_samples, scores)
        for key in ("ratio_index", "offset", "score", "psr", "margin", "flags"):
            out[key][i, j] = e[key]
        out["reports"][i][j] = e["report"]
    return out


def trusted(m, min_psr=MIN_PSR, min_margin=MIN_MARGIN):
    """[N, M] bool of a matrix dict (or any object with the same fields as attributes)."""
    get = (lambda k: m[k]) if isinstance(m, dict) else (lambda k: getattr(m, k))
    n, mm = get("ratio_index").shape
    ok = np.zeros((n, mm), bool)
    for i in range(n):
        for j in range(mm):
            if get("ratio_index")[i, j] < 0 or get("flags")[i, j] & (qm.FLAT | qm.EMPTY_WINDOW):
                continue
            psr, margin = float(get("psr")[i, j]), float(get("margin")[i, j])
            ok[i, j] = psr >= min_psr and margin >= min_margin
    return ok


def assign(m, min_psr=MIN_PSR, min_margin=MIN_MARGIN, exclusive=False):
    """dict(reference=[i or None per subtitle], runner_up_psr, ambiguous, subtitles=[[j, ...] per video])."""
    ok = trusted(m, min_psr, min_margin)
    psr = m["psr"] if isinstance(m, dict) else m.psr
    n, mm = ok.shape
    reference = [None] * mm
    if exclusive:
        cand = sorted(((-float(psr[i, j]), i, j) for i in range(n) for j in range(mm) if ok[i, j]))
        used = set()
        for _, i, j in cand:
            if i not in used and reference[j] is None:
                reference[j] = i
                used.add(i)
    else:
        for j in range(mm):
            for i in range(n):
                if ok[i, j] and (reference[j] is None or psr[i, j] > psr[reference[j], j]):
                    reference[j] = i
    runner = [float("nan")] * mm
    ambiguous = [False] * mm
    subtitles = [[] for _ in range(n)]
    for j, i in enumerate(reference):
        if i is not None:
            subtitles[i].append(j)
        others = [float(psr[k, j]) for k in range(n) if ok[k, j] and k != i]
        if others:
            runner[j] = max(others)
            ambiguous[j] = True
    return dict(reference=reference, runner_up_psr=runner, ambiguous=ambiguous, subtitles=subtitles)
