"""Host side of the ratio sweep: the grid arithmetic, the argument errors, the export and record against
the header, the defaults against the committed calibration, and -- on the CPU model alone -- that an exhaustive sweep
recovers ratios that the seven-ratio solve cannot."""
import json
import math
import os
import re

import numpy as np
import pytest

import sweep_cases as cases
import sweep_model as sm
from ffsubsync_amd import _native, quality, ratio_sweep
from ffsubsync_amd.constants import candidate_ratios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_arithmetic():
    for d, lo, hi, tol in [(59988, 0.9, 1.1, 40.0), (719990, 0.9, 1.1, 40.0), (359911, 0.92, 1.08, 10.0), (1000, 0.95, 1.05, 1.0),
                           (100, 1.0, 1.0, 60.0), (30000, 0.9, 0.9 + 3 * 4 * 10.0 / 30000, 10.0)]:
        g = ratio_sweep.sweep_grid(d, lo, hi, tol)
        step = 4.0 * tol / d
        assert g.dtype == np.float64 and g[0] == lo and g[-1] <= hi < lo + step * g.size  # the last point, and no more fit
        assert all(g[i] == lo + step * float(i) for i in range(g.size))  # one multiply, one add, each rounded on its own
        assert np.array_equal(g, sm.grid(d, lo, hi, tol)[0])
    assert ratio_sweep.sweep_grid(59988).size == 75 and ratio_sweep.sweep_grid(719990).size == 900
    assert ratio_sweep.sweep_grid(100, 1.0, 1.0).tolist() == [1.0]
    # the tolerance's meaning: half a step of ratio error times half the duration
    assert (4.0 * 40.0 / 719990) / 2 * (719990 / 2) == pytest.approx(40.0)
    assert ratio_sweep.default_exclusion_steps() == math.ceil(quality.DEFAULT_EXCLUSION_SAMPLES / (2 * ratio_sweep.DEFAULT_TOLERANCE))
    assert ratio_sweep.default_exclusion_steps(25.0) == sm.default_exclusion_steps(25.0) == 6
    assert ratio_sweep.default_exclusion_steps(1e6) == 1


def test_track_duration_is_the_raster_length_at_ratio_one():
    for seed, dur in [(1, 600.0), (2, 300.0), (9, 77.7)]:
        p = cases.problem("free", seed, dur)
        d = ratio_sweep.track_duration_samples(p.track)
        assert d == sm.duration_samples(p.track) == int(_native.raster_lengths(np.array([p.track[1].max()]), np.array([1.0]), 100)[0])


def test_fine_stage_and_pick_equal_the_model():
    fr, owner = ratio_sweep.fine_ratios([1.0, 0.9003, 1.0999], 1e-3, 0.9, 1.1)
    m_fr, m_owner = sm.fine_ratios([1.0, 0.9003, 1.0999], 1e-3, 0.9, 1.1)
    assert np.array_equal(fr, m_fr) and np.array_equal(owner, m_owner) and list(fr[-7:]) == candidate_ratios() == sm.SEVEN
    rng = np.random.RandomState(3)
    for _ in range(50):
        recs = np.zeros(fr.size, _native.CAND_RESULT_DTYPE)
        recs["score"] = rng.randint(0, 4, fr.size).astype(np.float64)  # ties everywhere
        recs["score"][rng.rand(fr.size) < 0.1] = -np.inf
        recs["flags"][rng.rand(fr.size) < 0.1] = _native.FLAG_EMPTY_WINDOW
        assert ratio_sweep.pick(fr, owner, [1.0, 0.9003, 1.0999], recs) == sm.pick(fr, owner, [1.0, 0.9003, 1.0999], recs["score"], recs["flags"])
    recs["score"] = -np.inf
    assert ratio_sweep.pick(fr, owner, [1.0, 0.9003, 1.0999], recs) == -1


def test_argument_errors_come_before_any_native_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native call")

    monkeypatch.setattr(_native, "load", boom)
    monkeypatch.setattr(_native, "require_gpu", boom)
    for bad in [dict(lo=math.nan), dict(hi=math.inf), dict(lo=1.1, hi=0.9), dict(lo=0.0), dict(lo=-1.0), dict(tolerance_samples=0.5),
                dict(tolerance_samples=math.nan), dict(tolerance_samples="x"), dict(lo=None)]:
        with pytest.raises(ValueError):
            ratio_sweep.sweep_grid(60000, **bad)
    for d in (0, -5, 1.5):
        with pytest.raises(ValueError, match="duration_samples"):
            ratio_sweep.sweep_grid(d)
    with pytest.raises(ValueError, match="2\\^20"):
        ratio_sweep.sweep_grid(10 ** 9, 0.9, 1.1, 1.0)
    assert ratio_sweep.sweep_grid(4 * (1 << 20) // 2, 1.0, 1.5, 1.0).size <= ratio_sweep.MAX_GRID
    track = (np.array([0, 2_000_000]), np.array([1_000_000, 3_000_000]), np.zeros(2, np.uint8))
    ref = np.zeros(500)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    for fn in (ratio_sweep.ratio_profile_batch, ratio_sweep.sweep_sync):
        for kwargs in [dict(lo=1.1, hi=0.9), dict(lo=math.nan), dict(tolerance_samples=0), dict(max_offset_seconds=0),
                       dict(max_offset_seconds=math.nan), dict(sample_rate=0), dict(sample_rate=99.5), dict(budget_bytes=0)]:
            with pytest.raises(ValueError):
                fn([(ref, track)], **kwargs)
        with pytest.raises(ValueError, match="cannot align empty speech data"):
            fn([(ref, empty)])
        with pytest.raises(ValueError, match="cannot align empty speech data"):
            fn([(np.zeros(0), track)])
        with pytest.raises(ValueError):
            fn([(ref, track[:2])])
    for kwargs in [dict(top_k=0), dict(top_k=9), dict(top_k=2.5), dict(exclusion_steps=0), dict(exclusion_steps=1.5)]:
        with pytest.raises(ValueError):
            ratio_sweep.sweep_sync([(ref, track)], **kwargs)
        with pytest.raises(ValueError):
            ratio_sweep.sweep_peaks(None, np.array([0, 1]), **kwargs)


def test_export_and_record_against_the_header():
    text = open(os.path.join(ROOT, "include", "ffsubsync_amd.h")).read()
    assert "ffs_sweep_peaks" in _native.EXPORTED_SYMBOLS
    decl = re.search(r"int ffs_sweep_peaks\(([^;]*)\);", text).group(1)
    assert [a.strip().rsplit(" ", 1)[0].replace("const ", "") for a in decl.replace("\n", " ").split(",")] == [
        "ffs_cand_result*", "int64_t*", "int", "int", "int64_t", "ffs_sweep_profile*", "void*"]
    assert "plan" not in decl  # stateless: not one of the side plans' batch exports
    body = re.search(r"typedef struct ffs_sweep_profile \{(.*?)\} ffs_sweep_profile;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int64_t|int32_t)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?", name)
            fields.append((m.group(1), {"double": "<f8", "int64_t": "<i8", "int32_t": "<i4"}[ctype], int(m.group(2) or 1)))
    dt = _native.SWEEP_PROFILE_DTYPE
    assert [(n, dt.fields[n][0].base.str, int(np.prod(dt.fields[n][0].shape or (1,)))) for n in dt.names] == fields
    assert int(re.search(r"sizeof\(ffs_sweep_profile\) == (\d+)", text).group(1)) == dt.itemsize == _native.SWEEP_PROFILE_BYTES
    assert dt.itemsize % 8 == 0 and all(dt.fields[n][1] % dt.fields[n][0].base.itemsize == 0 for n in dt.names)
    for name, value in [("FLAT", _native.SWEEP_FLAT), ("EMPTY", _native.SWEEP_EMPTY), ("AMBIGUOUS", _native.SWEEP_AMBIGUOUS)]:
        assert int(re.search(r"#define FFS_SWEEP_%s (\d+)" % name, text).group(1)) == value == getattr(sm, name)
    assert (sm.FLAG_EMPTY_WINDOW, sm.FLAG_AMBIGUOUS) == (_native.FLAG_EMPTY_WINDOW, _native.FLAG_AMBIGUOUS)
    assert _native.SWEEP_MAX_PEAKS == sm.MAX_PEAKS == ratio_sweep.MAX_TOP_K == 8
    assert hasattr(_native.load(), "ffs_sweep_peaks")


def test_defaults_are_what_the_calibration_rules_pick():
    cal = json.load(open(os.path.join(ROOT, "profiles", "ratio_sweep_calibration.json")))
    assert "CPU model only" in cal["what"] and "synthetic" in cal["what"]
    passing = [int(t) for t, v in cal["per_tolerance"].items() if v["worst_kept"] >= cal["keep_at_least"] == 0.9]
    assert sorted(int(t) for t in cal["per_tolerance"]) == [10, 15, 25, 40, 60]
    assert ratio_sweep.DEFAULT_TOLERANCE == max(passing) == cal["rules"]["default_tolerance"]
    good = [f for f in cal["files"] if f["kind"] in ("free", "seven")]
    bad = [f for f in cal["files"] if f["kind"] == "wrong"]
    for key, default, fallback in [("psr", ratio_sweep.DEFAULT_MIN_PSR, quality.DEFAULT_MIN_PSR),
                                   ("margin", ratio_sweep.DEFAULT_MIN_MARGIN, quality.DEFAULT_MIN_MARGIN)]:
        lo_good, hi_bad = min(f[key] for f in good), max(f[key] for f in bad)
        want = round((lo_good + hi_bad) / 2, 2) if lo_good > hi_bad else fallback
        assert default == want == cal["rules"]["min_" + key]
        assert cal["rules"][key + "_separates"] == (lo_good > hi_bad)


def test_assess_wording():
    prof = lambda psr, margin, flags=0: ratio_sweep.SweepProfile([(1.0, 0, 1.0)], 0.0, 1.0, 10, 0, psr, margin, flags)
    assert ratio_sweep.assess(prof(9.0, 9.0)) == []
    assert ratio_sweep.assess(prof(1.0, 0.5), min_psr=5.0, min_margin=3.0) == ["psr 1.0 < 5.0", "margin 0.5 < 3.0"]
    assert ratio_sweep.assess(prof(9.0, 9.0), at_edge=True) == ["best ratio at the edge of [lo, hi]"]
    assert ratio_sweep.assess(prof(0.0, 0.0, _native.SWEEP_FLAT)) == ["flat ratio profile (std 0)"]
    assert ratio_sweep.assess(prof(0.0, 0.0, _native.SWEEP_FLAT | _native.SWEEP_EMPTY)) == ["empty ratio profile"]
    rec = np.zeros(1, _native.SWEEP_PROFILE_DTYPE)[0]
    rec["peak_score"][:2], rec["peak_offset"][:2], rec["peak_index"][:2] = [9.0, 5.0], [12, -3], [2, 0]
    rec["mean"], rec["std"], rec["n_points"], rec["n_peaks"] = 3.0, 2.0, 4, 2
    p = ratio_sweep.profile_from_record(rec, np.array([0.9, 1.0, 1.1, 1.2]))
    assert p.peaks == [(9.0, 12, 1.1), (5.0, -3, 0.9)] and (p.psr, p.margin, p.flags) == (3.0, 2.0, 0)


@pytest.mark.parametrize("seed", cases.FREE_SEEDS)
def test_the_model_recovers_an_unknown_ratio_that_the_seven_cannot(seed):
    """The reference's own aligner, swept: the coarse maximum is the grid point nearest the true ratio, the fine stage
    lands within step / 16 of it, and the best of the seven framerate ratios scores less than half of that."""
    p = cases.problem("free", seed)
    res = cases.model_sweep("free", seed)
    assert min(abs(p.true_ratio - r) for r in sm.SEVEN) >= 2e-3
    grid = res["grid"]
    assert res["report"]["peaks"][0][2] == int(np.argmin(np.abs(grid - p.true_ratio)))
    assert abs(res["ratio"] - p.true_ratio) <= res["step"] / 16 * (1 + 1e-9)
    assert abs(res["offset"] - p.true_offset_samples) <= 5
    seven = (orc_score for orc_score in res["fine"][1][-7:])
    assert max(seven) < 0.5 * res["score"]
    psr, margin = sm.psr_margin(res["report"])
    assert psr >= ratio_sweep.DEFAULT_MIN_PSR and margin >= ratio_sweep.DEFAULT_MIN_MARGIN
