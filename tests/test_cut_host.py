"""Host side of the lag-range split (ffsubsync_amd/cut_align.py): the numpy model tests/cut_model.py against brute force,
against tests/split_model.py at [-W+1, W] and against the whole-vector correlation at P = inf; host validation; the
workloads/cuts.py ground truth; cue mapping over unmatched stretches.  No GPU needed."""
import numpy as np
import pytest

import cut_model as cm
import split_model as sm


def _problem(seed, R=None, S=None):
    rng = np.random.RandomState(seed)
    R = int(rng.randint(300, 2500)) if R is None else R
    S = int(rng.randint(300, 2500)) if S is None else S
    r = (np.repeat(rng.rand(R // 7 + 2) < 0.45, 7)[:R]).astype(np.uint8)
    sh = int(rng.randint(-S // 2, R // 2))
    idx = np.arange(S) + sh
    s = np.zeros(S, np.uint8)
    ok = (idx >= 0) & (idx < R)
    s[ok] = r[idx[ok]]
    s ^= (rng.rand(S) < 0.1).astype(np.uint8)
    r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
    s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (-0.5, 1.25)][(seed // 3) % 3]
    return r, s, r_lv, s_lv


@pytest.mark.parametrize("seed", range(12))
def test_model_equals_brute_force(seed):
    """Run-based block counts and the streamed DP against direct sums per (block, lag) and the split model's DP."""
    r, s, r_lv, s_lv = _problem(seed)
    rng = np.random.RandomState(100 + seed)
    k = 256
    lo = int(rng.randint(-s.size - 300, r.size))
    hi = lo + int(rng.randint(0, 700))
    m = cm.brute_scores(r, s, r_lv, s_lv, k, lo, hi)
    for b in range(m.shape[0]):
        assert m[b].tobytes() == cm.row_scores(r, s, r_lv, s_lv, k, lo, hi, b).tobytes()
    for p in (0.0, 3.0, 40.0, np.inf):
        o, total = sm.dp(m, p)
        offs, scores, tot = cm.solve(r, s, r_lv, s_lv, k, lo, hi, p)
        assert np.array_equal(offs, o + lo) and tot == total
        assert scores.tobytes() == m[np.arange(m.shape[0]), o].tobytes()


@pytest.mark.parametrize("seed", range(8))
def test_model_equals_split_model_at_symmetric_ranges(seed):
    r, s, r_lv, s_lv = _problem(50 + seed)
    w = [1, 7, 300, 1200][seed % 4]
    for p in (0.0, 25.0, 1e9):
        a = sm.solve(r, s, r_lv, s_lv, 256, w, p)
        b = cm.solve(r, s, r_lv, s_lv, 256, -w + 1, w, p)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
        assert cm.pieces(b[0], b[1], 256, s.size) == a[3]


@pytest.mark.parametrize("seed", range(8))
def test_infinite_penalty_full_range_is_the_correlation_argmax(seed):
    """One piece at the largest lag maximising the whole-vector score over [-(S-1), R-1] (direct sums; samples outside
    the reference absent)."""
    r, s, r_lv, s_lv = _problem(80 + seed, R=int(600 + 97 * seed), S=int(500 + 61 * seed))
    lo, hi = cm.full_range(r.size, s.size)
    offs, _, _ = cm.solve(r, s, r_lv, s_lv, 256, lo, hi, np.inf)
    assert np.all(offs == offs[0])
    c = np.array([(2 * s_lv[0] - 1, 2 * s_lv[1] - 1)[x] for x in s])
    rv = np.array([(2 * r_lv[0] - 1, 2 * r_lv[1] - 1)[x] for x in r])
    score = np.array([np.dot(c[max(0, -d):min(s.size, r.size - d)], rv[max(0, -d) + d:min(s.size, r.size - d) + d])
                      for d in range(lo, hi + 1)])
    best = np.flatnonzero(score >= score.max() - 1e-9 * max(1.0, abs(score.max())))
    assert offs[0] == lo + best[-1] or offs[0] in lo + best


def test_host_validation():
    from ffsubsync_amd import cut_align as ca

    for k in (300, 128, 65536, 1024.5):
        with pytest.raises(ValueError):
            ca.validate_args(k, 1.0)
    for p in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            ca.validate_args(1024, p)
    ca.validate_args(1024, float("inf"))
    for r in ((5, 4), (0, 2 ** 31), (-(2 ** 31), 0), (1.5, 3), 7, (1, 2, 3)):
        with pytest.raises(ValueError):
            ca.validate_range(r)
    assert ca.validate_range((-(2 ** 31 - 1), -(2 ** 31 - 1))) == (-(2 ** 31 - 1), -(2 ** 31 - 1))
    assert ca.full_range(100, 40) == (-39, 99)
    track = (np.array([0], np.int64), np.array([10000], np.int64), np.zeros(1, np.uint8))
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        ca.cut_sync([(np.zeros(0), track)])
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        ca.cut_sync([(np.ones(50), empty)])
    with pytest.raises(ValueError):
        ca.cut_sync([(np.ones(50), track)], lag_range=(3, 2))
    with pytest.raises(ValueError):
        ca.cut_sync([(np.ones(50), track)], radius_samples=0)


@pytest.mark.parametrize("seed", range(8))
def test_workload_ground_truth(seed):
    from workloads import cuts

    pr = cuts.make_problem(seed)
    assert pr.direction == ("up" if seed % 2 == 0 else "down")
    n = len(pr.scenes)
    total = sum(l for _, l in pr.scenes)
    assert cuts.MIN_SCENES <= n <= cuts.MAX_SCENES and 60000 <= total <= 300000
    assert abs(pr.d0) <= 6000
    prev_end = 0
    for pos, length in pr.scenes:
        assert 1500 <= length <= 36000
        assert 12000 <= pos - prev_end <= 48000
        prev_end = pos + (length if pr.direction == "down" else 0)
    assert prev_end <= pr.sub.size - 12000
    base = pr.ref.size - (total if pr.direction == "up" else -total)  # the video before the scenes were applied
    assert abs(base - 7200 * 100) <= 2
    samples = cuts.cue_samples(pr.track, pr.ratio)
    assert samples.size == pr.cue_offset.size == pr.cue_unmatched.size
    last = pr.d0 + (total if pr.direction == "up" else -total)
    for x, off, um in zip(samples, pr.cue_offset, pr.cue_unmatched):
        t = pr.true_offset(int(x))
        assert (t is None) == um and (um or t == off)
    assert pr.true_offset(pr.sub.size - 1) == last
    if pr.direction == "up":
        assert not pr.cue_unmatched.any() and np.all(np.diff(pr.cue_offset) >= 0)
    else:
        assert pr.cue_unmatched.sum() > 0
        assert np.all(np.diff(pr.cue_offset[~pr.cue_unmatched]) <= 0)
    # the data agree with the truth: most matched subtitle speech meets reference speech at its true offset
    hit = tot = 0
    for a, e, off, um in zip(pr.cue_start, pr.cue_end, pr.cue_offset, pr.cue_unmatched):
        if um or e <= a or a + off < 0 or e + off > pr.ref.size:
            continue
        hit += int(pr.ref[a + off:e + off].sum())
        tot += int(e - a)
    assert hit >= 0.8 * tot


def test_cue_mapping_over_unmatched_stretches():
    """map_cues_refined with offsets 30 to 50 minutes away and a cut stretch: cues before t1 keep the earlier piece,
    cues in [t1, t2) are unmatched (piece -2, shifted by the earlier piece), cues from t2 on take the later piece."""
    from ffsubsync_amd import split_refine as sr
    from ffsubsync_amd.split_align import Piece

    pieces = [Piece(0, 10, 0, 10240, 180000, 0.0), Piece(10, 20, 10240, 20480, 150000, 0.0),
              Piece(20, 30, 20480, 30000, 300000, 0.0)]
    mk = lambda t1, t2, a, b: sr.RefinedBreak(0, 0, 0, 0, t1, t2, a, b, 0.0, 0.0, 0)
    breaks = [mk(9000, 12000, 180000, 150000), mk(21000, 21000, 150000, 300000)]
    starts = np.array([0, 8999, 9000, 11999, 12000, 20999, 21000, 29999], np.int64) * 10000
    s, e, which, um = sr.map_cues_refined(starts, starts + 20000, 1.0, pieces, breaks)
    assert which.tolist() == [0, 0, -2, -2, 1, 1, 2, 2]
    assert um.tolist() == [False, False, True, True, False, False, False, False]
    shift = np.array([180000, 180000, 180000, 180000, 150000, 150000, 300000, 300000]) * 10000
    assert np.array_equal(s, starts + shift) and np.array_equal(e, starts + 20000 + shift)
