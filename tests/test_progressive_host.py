"""Host side of the progressive alignment (ffsubsync_amd.progressive): the stop rule on hand-made histories, every
ValueError before any native call, the header's record against ``_native``'s dtype, the shipped defaults against the
calibration table.  No device."""
import json
import math
import os
import re

import numpy as np
import pytest

import progressive_model as pm
from ffsubsync_amd import _native, progressive, quality
from ffsubsync_amd.progressive import ProgressState, ProgressiveSolve, StopRule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _st(cand=2, offset=100, psr=8.0, margin=4.0, ratio_margin=1.0, ref_len=1000, flags=0, other=9.0):
    q = quality.AlignmentQuality([(10.0, offset)], 0.0, 1.0, 12000, psr, margin, flags)
    return ProgressState(ref_len, cand, offset, 10.0, q, ratio_margin, other)


def test_settled_with_each_clause_failing_alone():
    rule = StopRule(min_psr=5.0, min_margin=3.0, min_ratio_margin=0.5, stable_updates=3, offset_tolerance=2, min_seconds=5.0)
    good = [_st(), _st(offset=102), _st(offset=101)]
    assert rule.settled(good) and not rule.settled(good[:2]) and not rule.settled([])
    assert not StopRule(stable_updates=None).settled(good * 4)
    for bad in (_st(cand=1), _st(offset=98), _st(psr=4.9), _st(margin=2.9), _st(ratio_margin=0.4), _st(ref_len=499),
                _st(flags=_native.QUALITY_FLAT)):
        for at in range(3):
            assert not rule.settled(good[:at] + [bad] + good[at + 1:]), (bad, at)
        assert rule.settled([bad] + good)  # older than the last three: not looked at
    one = _st(ratio_margin=math.nan, other=math.nan, margin=math.inf)  # one candidate, one peak
    assert rule.settled([one] * 3)
    assert StopRule(stable_updates=1, min_seconds=0).settled([_st(ref_len=0)])
    assert rule.settled(good) == pm.settled(
        [dict(best_cand=s.best_cand, offset=s.offset, score=10.0, mean=2.0, std=1.0, runner_up=6.0, other_best=9.0,
              ref_len=s.ref_len, flags=0) for s in good], 5.0, 3.0, 0.5, 3, 2, 500)


def test_stop_rule_arguments():
    for kw in (dict(stable_updates=0), dict(stable_updates=2.5), dict(min_psr=math.nan), dict(min_margin="3"),
               dict(offset_tolerance=-1), dict(offset_tolerance=1.5), dict(sample_rate=0), dict(min_seconds=math.nan)):
        with pytest.raises(ValueError):
            StopRule(**kw)


TRACK = (np.array([0, 2_000_000]), np.array([1_000_000, 3_000_000]), np.zeros(2, np.uint8))


def test_every_constructor_error_is_a_valueerror_before_any_native_call(monkeypatch):
    monkeypatch.setattr(_native, "require_gpu", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("reached the library"))
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    for args, kw in [(([],), {}), (([TRACK[:2]],), {}), (([(TRACK[0], TRACK[1][:1], TRACK[2])],), {}),
                     (([TRACK],), dict(max_offset_seconds=None)), (([TRACK],), dict(max_offset_seconds=math.inf)),
                     (([TRACK],), dict(max_offset_seconds=0.001)), (([TRACK],), dict(max_offset_seconds=1400)),
                     (([TRACK],), dict(ratios=[])), (([TRACK],), dict(ratios=[1.0] * 9)), (([TRACK],), dict(ratios=[0.0])),
                     (([TRACK],), dict(ratios=[math.nan])), (([TRACK],), dict(sample_rate=0)),
                     (([TRACK],), dict(max_reference_seconds=0)), (([TRACK],), dict(max_reference_seconds=math.inf)),
                     (([TRACK],), dict(max_reference_seconds=2.0 ** 30)), (([TRACK],), dict(top_k=0)),
                     (([TRACK],), dict(top_k=9)), (([TRACK],), dict(exclusion_samples=0)),
                     (([TRACK],), dict(ref_levels=(0.0, math.inf)))]:
        with pytest.raises(ValueError):
            ProgressiveSolve(*args, **kw)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        ProgressiveSolve([empty])
    with pytest.raises(ValueError):
        progressive.progressive_sync([(iter([]), TRACK, 1)])
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        progressive.progressive_sync([(iter([]), empty)])


def test_every_append_error_is_a_valueerror_before_any_native_call():
    import torch

    class NoCalls:
        def __getattr__(self, name):
            pytest.fail("reached the plan: %s" % name)

    s = object.__new__(ProgressiveSolve)
    s.plan, s.torch, s.n_files, s.consumed, s.max_ref = NoCalls(), torch, 2, [0, 90], 100
    words = torch.zeros(4, dtype=torch.int32)
    for chunks in ({2: np.zeros(3)}, {-1: np.zeros(3)}, {"a": np.zeros(3)}, {0: np.array([0, 2])}, {1: np.zeros(11)},
                   {0: (words, 0, 5)}, {0: (words, 0)}, {0: torch.zeros(3)}, {0: np.zeros(5), 1: np.array([3])}):
        with pytest.raises(ValueError):
            s.append(chunks)
    for dtype, name in ((np.float64, "F64"), (np.float32, "F32")):
        with pytest.raises(ValueError, match="multi-level float reference \\(FFS_DTYPE_%s\\) is not supported" % name) as err:
            s.append({0: np.array([0.0, 0.4, 1.0], dtype)})
        assert "needs a two-level reference" in str(err.value)
    assert s.consumed == [0, 90] and s.append({}) == {}
    s.plan = None
    for call in (lambda: s.append({0: np.zeros(3)}), lambda: s.reference(0)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_exports_and_record_against_the_header():
    text = open(os.path.join(ROOT, "include", "ffsubsync_amd.h")).read()
    names = ["ffs_prog_plan_create", "ffs_prog_plan_destroy", "ffs_prog_plan_workspace_bytes", "ffs_prog_open",
             "ffs_prog_append", "ffs_prog_reference", "ffs_prog_close"]
    lib = _native.load()
    for name in names:
        assert name in _native.EXPORTED_SYMBOLS and (name + "(") in text and hasattr(lib, name)
        assert not name.endswith("_batch")  # not one of the side plans' batch exports
    body = re.search(r"typedef struct ffs_prog_state \{(.*?)\} ffs_prog_state;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, decl in re.findall(r"(double|int64_t|int32_t)\s+([^;]+);", body):
        for name in decl.split(","):
            fields.append((name.strip(), {"double": "<f8", "int64_t": "<i8", "int32_t": "<i4"}[ctype]))
    dt = _native.PROG_STATE_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields
    assert int(re.search(r"sizeof\(ffs_prog_state\) == (\d+)", text).group(1)) == dt.itemsize == _native.PROG_STATE_BYTES
    assert all(dt.fields[n][1] % dt.fields[n][0].itemsize == 0 for n in dt.names)
    kern = open(os.path.join(ROOT, "ffsubsync_amd", "csrc", "ffs_progressive.h")).read()
    piece = int(re.search(r"constexpr int PROG_PIECE = (\d+);", kern).group(1))
    assert _native.PROG_PIECE_SAMPLES == 32 * piece
    assert _native.PROG_MAX_CAND == int(re.search(r"constexpr int PROG_MAX_CAND = (\d+);", kern).group(1)) == 8
    from ffsubsync_amd import split_align

    assert _native.PROG_MAX_LAGS == split_align.MAX_LAGS


def test_defaults_are_what_the_calibration_rules_pick():
    cal = json.load(open(os.path.join(ROOT, "profiles", "progressive_calibration.json")))
    assert "CPU" in cal["model"] and "synthetic" in cal["model"]
    assert cal["seeds"] >= 32 and cal["durations"] == [600.0, 3600.0] and (cal["chunk"], cal["W"], cal["E"]) == (10000, 6000, 300)
    assert cal["k_grid"] == [2, 3, 4, 6] and cal["m_grid"] == [0, 0.05, 0.1, 0.2, 0.4, 0.8]
    assert {(c["k"], c["m"]) for c in cal["cells"]} == {(k, m) for k in cal["k_grid"] for m in cal["m_grid"]}
    for dur in cal["durations"]:
        for kind in ("matched", "wrong"):
            assert sum(f["duration"] == dur and f["kind"] == kind for f in cal["files"]) == cal["seeds"]
    rule = StopRule()
    assert (rule.min_psr, rule.min_margin) == (quality.DEFAULT_MIN_PSR, quality.DEFAULT_MIN_MARGIN) == (cal["min_psr"], cal["min_margin"])
    assert rule.offset_tolerance == cal["offset_tolerance"] == 2 and rule.min_seconds == 0
    clean = [c for c in cal["cells"] if c["wrong_stops"] == 0]
    if not clean:
        assert rule.stable_updates is None and cal["shipped"]["stable_updates"] is None
        return
    best = min(clean, key=lambda c: (c["mean_consumed"], c["k"], c["m"]))
    larger = [m for m in cal["m_grid"] if m > best["m"]]
    want = (best["k"] + 1, larger[0] if larger else best["m"])
    assert (rule.stable_updates, rule.min_ratio_margin) == want == (cal["shipped"]["stable_updates"], cal["shipped"]["min_ratio_margin"])
    assert (progressive.DEFAULT_STABLE_UPDATES, progressive.DEFAULT_MIN_RATIO_MARGIN) == want
