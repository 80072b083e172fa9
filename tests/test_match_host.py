"""Subtitle-to-video matching on the host (ffsubsync_amd.match, tests/match_model.py): the assignment on hand-written
matrices, the model matrix on synthetic seeds, argument validation.  No GPU."""
import numpy as np
import pytest

import match_model as mm
import quality_model as qm
from ffsubsync_amd import _native, match, quality
from ffsubsync_amd.constants import candidate_ratios
from workloads import synth

RATIOS = list(candidate_ratios())


def _matrix(psr, margin=None, ratio_index=None, flags=None):
    psr = np.asarray(psr, dtype=np.float64)
    m = match.empty_matrix(psr.shape[0], psr.shape[1], RATIOS)
    m.psr[...] = psr
    m.margin[...] = 10.0 if margin is None else np.asarray(margin, dtype=np.float64)
    m.ratio_index[...] = 0 if ratio_index is None else np.asarray(ratio_index)
    m.flags[...] = 0 if flags is None else np.asarray(flags)
    return m


def _nan_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def spec_track(spec):
    """The subtitle track of a synth pair as interval records (its ratio-1.0 candidate's samples, 10 ms each)."""
    j = spec.ratios.index(1.0)
    start = spec.cand_starts[j].astype(np.int64) * 10000
    end = spec.cand_ends[j].astype(np.int64) * 10000
    keep = end > start
    return start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)


def test_assign_picks_the_largest_trusted_psr_per_subtitle():
    m = _matrix([[9.0, 2.0, 7.0],
                 [6.0, 8.0, 7.0],
                 [1.0, 3.0, 4.9]])
    a = match.assign(m)
    assert a.reference == [0, 1, 0]  # column 2: a tie at 7.0 goes to the smaller reference index
    assert a.ambiguous.tolist() == [True, False, True]
    assert _nan_equal(a.runner_up_psr, [6.0, np.nan, 7.0])
    assert _nan_equal(a.psr, [9.0, 8.0, 7.0])
    assert a.subtitles == [[0, 2], [1], []]  # several subtitles may share a video


def test_assign_exclusive_takes_pairs_by_descending_psr_while_both_sides_are_free():
    m = _matrix([[9.0, 8.5, 7.0],
                 [6.0, 8.0, 7.0],
                 [1.0, 3.0, 4.9]])
    a = match.assign(m, exclusive=True)
    # (0,0)=9 first; (0,1)=8.5 loses video 0; (1,1)=8; subtitle 2 finds videos 0 and 1 taken and video 2 untrusted
    assert a.reference == [0, 1, None]
    assert a.subtitles == [[0], [1], []]
    assert a.ambiguous.tolist() == [True, True, True]  # the other trusted references are still reported
    assert _nan_equal(a.runner_up_psr, [6.0, 8.5, 7.0])
    tie = match.assign(_matrix([[7.0, 7.0], [7.0, 7.0]]), exclusive=True)
    assert tie.reference == [0, 1]  # ties: smaller reference, then smaller subtitle index


def test_assign_never_trusts_an_untrusted_best_or_a_pair_without_a_ratio():
    psr = [[20.0, 6.0], [5.5, 30.0]]
    margin = [[1.0, 10.0], [10.0, 10.0]]  # (0,0): the largest psr, but its runner-up is too close
    ratio_index = [[0, 0], [0, -1]]  # (1,1): no ratio landed inside the window
    a = match.assign(_matrix(psr, margin, ratio_index))
    assert a.reference == [1, 0] and not a.ambiguous.any()
    flags = [[_native.QUALITY_FLAT, 0], [0, _native.QUALITY_EMPTY_WINDOW]]
    a = match.assign(_matrix([[9.0, 9.0], [9.0, 9.0]], flags=flags))
    assert a.reference == [1, 0]
    a = match.assign(_matrix([[np.nan, 4.0]], [[np.nan, 9.0]], [[-1, 0]]))
    assert a.reference == [None, None] and a.subtitles == [[]] and np.isnan(a.runner_up_psr).all()
    # thresholds are arguments
    assert match.assign(_matrix([[np.nan, 4.0]], [[np.nan, 9.0]], [[-1, 0]]), min_psr=3.5).reference == [None, 0]


def test_assign_on_empty_inputs():
    for n, m_ in ((0, 0), (0, 3), (2, 0)):
        a = match.assign(match.empty_matrix(n, m_, RATIOS))
        assert a.reference == [None] * m_ and a.subtitles == [[] for _ in range(n)]
        assert a.ambiguous.shape == (m_,) and a.runner_up_psr.shape == (m_,)


def test_trusted_is_quality_assess_and_assign_equals_the_model():
    rng = np.random.RandomState(5)
    for trial in range(40):
        n, m_ = int(rng.randint(1, 6)), int(rng.randint(1, 7))
        psr = np.round(rng.uniform(2.0, 9.0, (n, m_)), 1)  # one decimal: ties happen
        margin = np.round(rng.uniform(1.0, 6.0, (n, m_)), 1)
        margin[rng.rand(n, m_) < 0.1] = np.inf
        ridx = np.where(rng.rand(n, m_) < 0.1, -1, rng.randint(0, 7, (n, m_)))
        flags = np.where(rng.rand(n, m_) < 0.1, rng.randint(1, 4, (n, m_)), 0)
        mat = _matrix(psr, margin, ridx, flags)
        ok = mat.trusted()
        for i in range(n):
            for j in range(m_):
                q = quality.AlignmentQuality([], 0.0, 1.0, 1, float(psr[i, j]), float(margin[i, j]), int(flags[i, j]))
                assert ok[i, j] == (ridx[i, j] >= 0 and not quality.assess(q)), (trial, i, j)
        assert np.array_equal(ok, mm.trusted(mat))
        for exclusive in (False, True):
            got, want = match.assign(mat, exclusive=exclusive), mm.assign(mat, exclusive=exclusive)
            assert got.reference == want["reference"], (trial, exclusive)
            assert got.subtitles == want["subtitles"] and got.ambiguous.tolist() == want["ambiguous"]
            assert _nan_equal(got.runner_up_psr, want["runner_up_psr"])


def test_derive_equals_from_record():
    recs = np.zeros(4, _native.QUALITY_RESULT_DTYPE)
    recs["peak_score"][:, 0] = [10.0, 10.0, 10.0, 0.0]
    recs["peak_score"][:, 1] = [4.0, 0.0, 4.0, 0.0]
    recs["n_peaks"] = [2, 1, 2, 0]
    recs["mean"] = [1.0, 1.0, 10.0, 0.0]
    recs["std"] = [2.0, 2.0, 0.0, 0.0]
    recs["flags"] = [0, 0, _native.QUALITY_FLAT, _native.QUALITY_FLAT | _native.QUALITY_EMPTY_WINDOW]
    psr, margin, flags = match.derive(recs)
    for k, r in enumerate(recs):
        q = quality.from_record(r)
        assert (psr[k], margin[k], flags[k]) == (q.psr, q.margin, q.flags), k


def test_model_matrix_separates_matched_from_wrong_pairs():
    """Six synthetic 10-minute seeds, every subtitle against every reference at +-60 s: the diagonal is trusted with the
    spec's true ratio, nothing else is; the boundary-list form of the model's counts equals the FFT form."""
    specs = [synth.make_pair_spec(seed, duration_s=600.0) for seed in range(6)]
    refs = [synth.rasterize(sp.ref_len, sp.ref_starts, sp.ref_ends) for sp in specs]
    tracks = [spec_track(sp) for sp in specs]
    m = mm.matrix(refs, tracks, 6000, RATIOS)
    ok = mm.trusted(m)
    assert np.array_equal(ok, np.eye(6, dtype=bool)), (m["psr"], m["margin"])
    assert np.diag(m["ratio_index"]).tolist() == [sp.true_ratio_index for sp in specs]
    # (the track is rounded to 10 ms samples twice, in the spec and at the ratio: the lag may sit a sample or two off)
    assert np.abs(np.diag(m["offset"]) - np.array([sp.true_offset_samples for sp in specs])).max() <= 2
    assert (np.argmax(m["psr"], axis=0) == np.arange(6)).all() and (np.argmax(m["psr"], axis=1) == np.arange(6)).all()
    a = mm.assign(m)
    assert a["reference"] == list(range(6)) and not any(a["ambiguous"])
    fast = mm.matrix(refs, tracks, 6000, RATIOS, scores=mm.scores_sparse)
    for key in ("ratio_index", "offset", "score", "psr", "margin", "flags"):
        assert fast[key].tobytes() == m[key].tobytes(), key


def test_sparse_counts_equal_the_fft_counts_on_edge_windows():
    rng = np.random.RandomState(11)
    for trial in range(24):
        R, S = int(rng.randint(1, 400)), int(rng.randint(1, 400))
        r, s = rng.rand(R) < rng.uniform(0, 1), rng.rand(S) < rng.uniform(0, 1)
        w = [None, 1, 5, 50, 1000][trial % 5]
        lags = qm.lag_set(R, S, w)
        if lags.size == 0:
            continue
        for got, want in zip(mm.counts_sparse(r, s, lags), qm.counts(r, s, lags)):
            assert np.array_equal(got, want), (trial, R, S, w)


def test_argument_errors_raise_before_any_device_work():
    spec = synth.make_pair_spec(0, duration_s=120.0)
    ref = synth.rasterize(spec.ref_len, spec.ref_starts, spec.ref_ends).astype(float)
    track = spec_track(spec)
    with pytest.raises(ValueError, match="unknown algorithm"):
        match.match_quality([ref], [track], algorithm="fft")
    for kw in (dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0), dict(max_offset_seconds=0)):
        with pytest.raises(ValueError):
            match.match_quality([ref], [track], **kw)
    for pairs in ([(1, 0)], [(0, 1)], [(-1, 0)]):
        with pytest.raises(ValueError, match="pair index"):
            match.match_quality([ref], [track], pairs=pairs)
    with pytest.raises(ValueError, match="multi-level float reference"):
        match.match_quality([ref + 0.25 * np.arange(ref.size) % 3], [track])
    with pytest.raises(ValueError, match="empty speech data"):
        match.match_quality([np.zeros(0)], [track])
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), None)
    with pytest.raises(ValueError, match="empty speech data"):
        match.match_quality([ref], [empty])
    with pytest.raises(ValueError, match="ratio"):
        match.match_quality([ref], [track], ratios=[])
    none = match.match_quality([ref], [track], pairs=[])  # nothing requested: nothing runs
    assert none.shape == (1, 1) and int(none.ratio_index[0, 0]) == -1 and not none.trusted().any()
    assert _native.match_algorithm_code(" Bits ") == _native.FFS_MATCH_BITS
