"""Alignment quality report, host side: the numpy model (tests/quality_model.py) against the reference's own
correlation array, argument checks, the wording of assess, the separation the default thresholds rest on, and the
record layout."""
import math

import numpy as np
import pytest

import golden_cases
import quality_model as qm
from oracle import aligners_oracle as orc


def _check_against_reference(ref, sub, w):
    """Model scores == the reference's masked convolve entries (within fp64 FFT noise); peak 1 == orc.fft_align."""
    ref = np.asarray(ref, dtype=float)
    sub = np.asarray(sub, dtype=float)
    r_lv = (float(ref.min()), float(ref.max())) if ref.min() != ref.max() else (0.0, float(ref.max()) or 1.0)
    s_lv = (float(sub.min()), float(sub.max())) if sub.min() != sub.max() else (0.0, float(sub.max()) or 1.0)
    rb, sb = ref == r_lv[1], sub == s_lv[1]
    lags, sc = qm.scores(rb, sb, r_lv, s_lv, w)
    conv, n_sub = orc.convolve_full(ref, sub)
    masked = orc.mask_extreme_offsets(conv, n_sub, w)
    k = np.flatnonzero(np.isfinite(masked))
    want_lags = len(masked) - 1 - n_sub - k
    order = np.argsort(want_lags)
    assert np.array_equal(lags, want_lags[order])
    want = masked[k][order]
    if lags.size == 0:
        return
    assert np.all(np.abs(sc - want) <= 1e-6 * max(1.0, float(np.abs(want).max()))), float(np.abs(sc - want).max())
    rep = qm.report(rb, sb, r_lv, s_lv, w, 2, 5)
    o_score, o_off = orc.fft_align(ref, sub, w)
    p_score, p_off = rep["peaks"][0]
    assert abs(p_score - o_score) <= 1e-6 * max(1.0, abs(o_score))
    # the reference's argmax runs on FFT noise: an exact tie may fall either way
    assert p_off == o_off or sc[np.searchsorted(lags, o_off)] == p_score


def test_model_on_golden_cases():
    n = 0
    for case in golden_cases.build_cases(include_large=False).values():
        ref = orc.as_pm1(case["ref"]) * 0.5 + 0.5
        for cand in case["cands"]:
            sub = orc.as_pm1(cand) * 0.5 + 0.5
            if len(ref) == 0 or len(sub) == 0 or np.unique(ref).size > 2 or np.unique(sub).size > 2:
                continue
            _check_against_reference(ref, sub, case["max_offset"])
            n += 1
    assert n >= 10


def _seeded_small(seed):
    rng = np.random.RandomState(500 + seed)
    R, S = int(rng.randint(1, 3000)), int(rng.randint(1, 3000))
    w = [None, 1, 2, 50, 700, R + S, 3 * (R + S)][seed % 7]
    r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
    s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (-0.5, 1.25)][(seed // 3) % 3]
    rb = rng.rand(R) < 0.4
    sb = rng.rand(S) < 0.4
    rb[0] = True
    sb[0] = True
    return np.where(rb, r_lv[1], r_lv[0]), np.where(sb, s_lv[1], s_lv[0]), w


@pytest.mark.parametrize("seed", range(32))
def test_model_on_seeded_small_cases(seed):
    ref, sub, w = _seeded_small(seed)
    _check_against_reference(ref, sub, w)


def test_negative_slice_window():
    """R = 1, S = 9: N = 16, W = 8 masks every entry; W = 11 on R = 10, S = 5 keeps only the last one (d = -5)."""
    assert qm.lag_set(1, 9, 8).size == 0
    assert qm.lag_set(10, 5, 11).tolist() == [-5]
    ref, sub = np.array([1.0, 0, 1, 1, 0, 0, 1, 0, 1, 1]), np.array([0.0, 1, 1, 0, 1])
    _check_against_reference(ref, sub, 11)


def test_lag_count_matches_the_model():
    from ffsubsync_amd import quality

    for R, S, w in [(1000, 800, 50), (10, 5, 11), (1, 9, 8), (300, 3000, None), (5000, 5000, 1), (20, 30, 10 ** 6)]:
        assert quality.n_lags(R, S, w) == qm.lag_set(R, S, w).size


def test_peaks_and_moments_rules():
    lags = np.arange(-5, 6)
    sc = np.array([1.0, 3, 3, 0, 5, 5, 2, 0, 4, 4, 1])
    assert qm.peaks(lags, sc, 8, 1)[:3] == [(5.0, 0), (5.0, -1), (4.0, 4)]  # ties to the largest lag
    assert qm.peaks(lags, sc, 8, 3) == [(5.0, 0), (4.0, 4), (3.0, -3)]
    assert qm.peaks(lags, sc, 8, 100) == [(5.0, 0)]
    assert qm.moments(np.full(7, 2.5)) == (2.5, 0.0, qm.FLAT)
    m, s, f = qm.moments(sc)
    assert f == 0 and m == pytest.approx(sc.mean()) and s == pytest.approx(sc.std())


def test_validate_args_rejections():
    from ffsubsync_amd import quality

    quality.validate_args(None, 1, 1)
    quality.validate_args(6000, 8, 10 ** 9)
    for args in [(0, 3, 300), (-1, 3, 300), (1.5, 3, 300), (6000, 0, 300), (6000, 9, 300), (6000, 2.5, 300),
                 (6000, 3, 0), (6000, 3, -4), (6000, 3, 0.5)]:
        with pytest.raises(ValueError):
            quality.validate_args(*args)


def _q(psr, margin, flags=0, peaks=((10.0, 3), (5.0, 900))):
    from ffsubsync_amd import quality

    return quality.AlignmentQuality(list(peaks), 1.0, 1.0, 100, psr, margin, flags)


def test_assess_wording():
    from ffsubsync_amd import _native, quality

    assert quality.assess(_q(7.5, 4.0)) == []
    assert quality.assess(_q(2.14, 4.0)) == ["psr 2.1 < 5.0"]
    assert quality.assess(_q(2.14, 0.26)) == ["psr 2.1 < 5.0", "margin 0.3 < 3.0"]
    assert quality.assess(_q(6.0, math.inf, peaks=((10.0, 3),))) == []
    assert quality.assess(_q(6.0, 2.0), min_psr=6.5, min_margin=1.0) == ["psr 6.0 < 6.5"]
    assert quality.assess(_q(0.0, 0.0, _native.QUALITY_FLAT)) == ["flat correlation (std 0)"]
    assert quality.assess(_q(0.0, 0.0, _native.QUALITY_FLAT | _native.QUALITY_EMPTY_WINDOW, ())) == ["empty lag window"]


def test_from_record_derives_psr_and_margin():
    from ffsubsync_amd import _native, quality

    rec = np.zeros(1, _native.QUALITY_RESULT_DTYPE)[0]
    rec["peak_score"][:2] = (50.0, 20.0)
    rec["peak_offset"][:2] = (-7, 400)
    rec["mean"], rec["std"], rec["n_lags"], rec["n_peaks"] = 2.0, 6.0, 12000, 2
    q = quality.from_record(rec)
    assert q.peaks == [(50.0, -7), (20.0, 400)] and q.psr == 8.0 and q.margin == 5.0 and q.flags == 0
    rec["n_peaks"] = 1
    assert quality.from_record(rec).margin == math.inf
    rec["std"] = 0.0
    q = quality.from_record(rec)
    assert q.psr == 0.0 and q.margin == 0.0 and q.flat


def test_defaults_separate_matched_from_wrong_pairs():
    """10 min, +-60 s, E = 300, the true-ratio candidate: every matched seed passes, every wrong one (the subtitle of
    seed i against the reference of seed i+1) fails, on 16 + 16 seeds."""
    from ffsubsync_amd import quality
    from workloads import synth

    bad = []
    for seed in range(16):
        sp, sp2 = synth.make_pair_spec(seed, duration_s=600.0), synth.make_pair_spec(seed + 1, duration_s=600.0)
        ref, cands = synth.pair_arrays(sp)
        ref2, _ = synth.pair_arrays(sp2)
        j = sp.true_ratio_index
        for kind, r in (("matched", ref), ("wrong", ref2)):
            rep = qm.report(r, cands[j], (0.0, 1.0), (0.0, sp.cand_amp[j]), 6000, quality.DEFAULT_TOP_K,
                            quality.DEFAULT_EXCLUSION_SAMPLES)
            psr, margin = qm.psr_margin(rep)
            trusted = psr >= quality.DEFAULT_MIN_PSR and margin >= quality.DEFAULT_MIN_MARGIN
            if trusted != (kind == "matched"):
                bad.append((seed, kind, psr, margin))
    assert not bad, bad


def test_record_dtype_matches_the_struct():
    from ffsubsync_amd import _native

    assert _native.QUALITY_RESULT_DTYPE.itemsize == 160 == _native.QUALITY_RESULT_BYTES
    off = _native.QUALITY_RESULT_DTYPE.fields
    assert [off[k][1] for k in ("peak_score", "peak_offset", "mean", "std", "n_lags", "n_peaks", "flags")] == \
        [0, 64, 128, 136, 144, 152, 156]
