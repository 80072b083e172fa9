"""Numpy model of the alignment quality report (csrc/ffs_quality.h, ffsubsync_amd.quality): the contract the device is
pinned against.

Per pair: a two-level reference (0/1 samples + levels), ONE two-level subtitle vector, the lag window W (or None).
  - lag set: exactly the entries of the reference's masked `convolve` array its argmax reads (aligners.py:31-48 through
    oracle.aligners_oracle.mask_extreme_offsets, Python slice semantics included); convolve index k is lag N-1-S-k
  - score of lag d: n11 by fp64 FFT of the 0/1 vectors rounded to integers, ov / n1x / nx1 from cumulative sums,
    through oracle.runs_model.two_level_scores; exactly 0.0 where the overlap is empty
  - peaks: greedy, largest lag on ties, each at least E from every earlier one
  - moments: two passes; all scores equal -> mean = that score, std = 0 (FLAT)
"""
import numpy as np

from oracle import aligners_oracle as orc
from oracle import runs_model as rm

FLAT = 1
EMPTY_WINDOW = 2


def _pm1(level):
    return 2.0 * float(level) - 1.0


def lag_set(R, S, max_offset_samples):
    """The lags of the reference's window, ascending (int64)."""
    n = orc.fft_length(R, S)
    masked = orc.mask_extreme_offsets(np.zeros(n), S, max_offset_samples)
    k = np.flatnonzero(np.isfinite(masked))
    return np.sort(n - 1 - S - k).astype(np.int64)


def counts(ref01, sub01, lags):
    """(n11, n1x, nx1, ov) at every lag: n11 = sum_i s[i] r[i+d] by an fp64 FFT, rounded (exact at these sizes)."""
    r = np.asarray(ref01).astype(np.float64)
    s = np.asarray(sub01).astype(np.float64)
    R, S = r.size, s.size
    nfft = 1 << int(np.ceil(np.log2(R + S)))
    conv = np.fft.irfft(np.fft.rfft(r, nfft) * np.fft.rfft(s[::-1], nfft), nfft)[: R + S - 1]  # conv[d + S - 1] = n11(d)
    lags = np.asarray(lags, dtype=np.int64)
    i0 = np.maximum(0, -lags)
    i1 = np.minimum(S, R - lags)
    ov = np.maximum(0, i1 - i0)
    has = ov > 0
    raw = np.zeros(lags.size)
    raw[has] = conv[lags[has] + S - 1]
    n11 = np.rint(raw).astype(np.int64)
    assert np.all(np.abs(raw - n11) < 0.25), float(np.abs(raw - n11).max())
    cs = np.concatenate([[0], np.cumsum(np.asarray(sub01).astype(np.int64))])
    cr = np.concatenate([[0], np.cumsum(np.asarray(ref01).astype(np.int64))])
    a, b = np.clip(i0, 0, S), np.clip(i1, 0, S)
    n1x = np.where(has, cs[b] - cs[a], 0)
    nx1 = np.where(has, cr[np.clip(b + lags, 0, R)] - cr[np.clip(a + lags, 0, R)], 0)
    return n11, n1x, nx1, ov


def scores(ref01, sub01, ref_levels, sub_levels, max_offset_samples):
    """(lags, scores) over the lag set."""
    ref01, sub01 = np.asarray(ref01) != 0, np.asarray(sub01) != 0
    lags = lag_set(ref01.size, sub01.size, max_offset_samples)
    n11, n1x, nx1, ov = counts(ref01, sub01, lags)
    f = lambda x: x.astype(np.float64)
    sc = rm.two_level_scores(f(n11), f(n1x), f(nx1), f(ov), _pm1(sub_levels[0]), _pm1(sub_levels[1]),
                             _pm1(ref_levels[0]), _pm1(ref_levels[1]))
    sc = np.where(ov > 0, sc, 0.0)
    return lags, sc


def peaks(lags, sc, top_k, exclusion_samples):
    """Greedy peaks: [(score, lag)], the maximum first, ties to the largest lag."""
    out = []
    ok = np.ones(lags.size, bool)
    for _ in range(top_k):
        if not ok.any():
            break
        best = sc[ok].max()
        i = int(np.flatnonzero(ok & (sc == best))[-1])
        out.append((float(sc[i]), int(lags[i])))
        ok &= np.abs(lags - lags[i]) >= exclusion_samples
    return out


def moments(sc):
    """(mean, std, flags) of the scores: two passes, population std; all equal -> (that score, 0.0, FLAT)."""
    if sc.size == 0:
        return 0.0, 0.0, FLAT | EMPTY_WINDOW
    if sc.min() == sc.max():
        return float(sc[0]), 0.0, FLAT
    mean = float(sc.sum()) / sc.size
    return mean, float(np.sqrt(float(((sc - mean) ** 2).sum()) / sc.size)), 0


def report(ref01, sub01, ref_levels, sub_levels, max_offset_samples, top_k=3, exclusion_samples=300):
    """dict(peaks=[(score, lag)], mean, std, n_lags, flags) of one pair."""
    lags, sc = scores(ref01, sub01, ref_levels, sub_levels, max_offset_samples)
    mean, std, flags = moments(sc)
    return dict(peaks=peaks(lags, sc, top_k, exclusion_samples), mean=mean, std=std, n_lags=int(lags.size), flags=flags)


def psr_margin(rep):
    """Host-side statistics: psr = (peak1 - mean) / std, margin = (peak1 - peak2) / std (+inf with one peak);
    both 0 when std == 0."""
    if rep["std"] == 0 or not rep["peaks"]:
        return 0.0, 0.0
    p1 = rep["peaks"][0][0]
    psr = (p1 - rep["mean"]) / rep["std"]
    margin = (p1 - rep["peaks"][1][0]) / rep["std"] if len(rep["peaks"]) > 1 else float("inf")
    return psr, margin
