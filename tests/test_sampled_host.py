"""Host side of the sampled alignment (ffsubsync_amd.sampled): every ValueError before any native call, the new exports
against the header and ``_native``, the shipped default rule against the calibration table.  No device."""
import json
import math
import os
import re

import numpy as np
import pytest

from ffsubsync_amd import _native, quality, sampled
from ffsubsync_amd.progressive import StopRule
from ffsubsync_amd.sampled import SampledSolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK = (np.array([0, 2_000_000]), np.array([1_000_000, 3_000_000]), np.zeros(2, np.uint8))
NAMES = ["ffs_prog_open_sampled", "ffs_prog_append_at", "ffs_prog_known", "ffs_prog_plan_sampled_bytes"]


def test_exports_against_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "ffsubsync_amd.h")).read()
    lib = _native.load()
    for name in NAMES:
        assert name in _native.EXPORTED_SYMBOLS and (name + "(") in text and hasattr(lib, name)
        assert name.startswith("ffs_prog_") and not name.endswith("_batch")
    assert int(re.search(r"#define FFS_PROG_MAX_INTERVALS (\d+)", text).group(1)) == _native.PROG_MAX_INTERVALS == 256
    assert sampled.MAX_INTERVALS == 256
    # the argument lists, by count: open_sampled = open + ref_total, append_at = append + position
    def n_args(name):
        return re.search(r"\b%s\(([^;]*?)\);" % name, text, re.S).group(1).count(",") + 1

    assert n_args("ffs_prog_open_sampled") == n_args("ffs_prog_open") + 1 == len(lib.ffs_prog_open_sampled.argtypes)
    assert n_args("ffs_prog_append_at") == n_args("ffs_prog_append") + 1 == len(lib.ffs_prog_append_at.argtypes)
    assert n_args("ffs_prog_known") == 5 == len(lib.ffs_prog_known.argtypes)
    kern = open(os.path.join(ROOT, "ffsubsync_amd", "csrc", "ffs_sampled.h")).read()
    for k in ("k_samp_ingest", "k_samp_counts", "k_samp_peaks"):
        assert "void __launch_bounds__" in kern and k in kern
    assert "ffs_sampled.h" in open(os.path.join(ROOT, "ffsubsync_amd", "csrc", "Makefile")).read()


def test_every_constructor_and_sync_error_is_a_valueerror_before_any_native_call(monkeypatch):
    monkeypatch.setattr(_native, "require_gpu", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_native, "load", lambda: pytest.fail("reached the library"))
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    for args, kw in [(([], []), {}), (([TRACK], []), {}), (([TRACK], [10.0, 20.0]), {}), (([TRACK], [0.0]), {}),
                     (([TRACK], [math.nan]), {}), (([TRACK], [math.inf]), {}), (([TRACK], ["10"]), {}),
                     (([TRACK], [2.0 ** 30]), {}), (([TRACK[:2]], [10.0]), {}),
                     (([TRACK], [10.0]), dict(max_offset_seconds=None)), (([TRACK], [10.0]), dict(max_offset_seconds=1400)),
                     (([TRACK], [10.0]), dict(ratios=[])), (([TRACK], [10.0]), dict(ratios=[1.0] * 9)),
                     (([TRACK], [10.0]), dict(sample_rate=0)), (([TRACK], [10.0]), dict(top_k=0)),
                     (([TRACK], [10.0]), dict(exclusion_samples=0)), (([TRACK], [10.0]), dict(ref_levels=(0.0, math.inf)))]:
        with pytest.raises(ValueError):
            SampledSolve(*args, **kw)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        SampledSolve([empty], [10.0])
    read = lambda start, seconds: np.zeros(int(seconds * 100), bool)
    overlap = lambda total, seg: [(0, 10), (5, 20)]
    outside = lambda total, seg: [(0, total + 1)]
    for problems, kw in [([(read, TRACK)], {}), ([(None, TRACK, 10.0)], {}), ([(read, TRACK, 0.0)], {}),
                         ([(read, TRACK, math.nan)], {}), ([(read, TRACK, 10.0)], dict(segment_seconds=0)),
                         ([(read, TRACK, 10.0)], dict(segment_seconds=math.nan)), ([(read, TRACK, 10.0)], dict(order="spread")),
                         ([(read, TRACK, 10.0)], dict(order=overlap)), ([(read, TRACK, 10.0)], dict(order=outside)),
                         ([(read, TRACK, 10.0)], dict(rule="never")), ([(read, TRACK, 10.0)], dict(sample_rate=0)),
                         ([(read, TRACK, 10.0)], dict(max_offset_seconds=math.inf)), ([(read, TRACK[:2], 10.0)], {})]:
        with pytest.raises(ValueError):
            sampled.sampled_sync(problems, **kw)
    many = lambda total, seg: [(2 * k, 2 * k + 1) for k in range(257)]
    with pytest.raises(ValueError, match="256 known intervals"):
        sampled.sampled_sync([(read, TRACK, 10.0)], order=many)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        sampled.sampled_sync([(read, empty, 10.0)])


def test_every_append_at_error_is_a_valueerror_before_any_native_call():
    import torch

    class NoCalls:
        def __getattr__(self, name):
            pytest.fail("reached the plan: %s" % name)

    s = object.__new__(SampledSolve)
    s.plan, s.torch, s.n_files, s.consumed, s.max_ref = NoCalls(), torch, 2, [0, 10], 100
    s.totals, s._known = [100, 50], [[], [(10, 20)]]
    words = torch.zeros(4, dtype=torch.int32)
    for chunks in ({2: (0, np.zeros(3))}, {-1: (0, np.zeros(3))}, {"a": (0, np.zeros(3))}, {0: np.zeros(3)},
                   {0: (0, np.zeros(3), 1)}, {0: (0, np.array([0, 2]))}, {0: (-1, np.zeros(3))}, {0: (98, np.zeros(3))},
                   {0: (1.5, np.zeros(3))}, {1: (48, np.zeros(3))}, {1: (19, np.zeros(1))}, {1: (5, np.zeros(6))},
                   {1: (0, np.zeros(50))}, {0: (0, (words, 0, 5))}, {0: (0, (words, 0))}, {0: (0, torch.zeros(3))},
                   {0: (0, np.zeros(5)), 1: (12, np.zeros(1))}):
        with pytest.raises(ValueError):
            s.append_at(chunks)
    for dtype, name in ((np.float64, "F64"), (np.float32, "F32")):
        with pytest.raises(ValueError, match="multi-level float reference \\(FFS_DTYPE_%s\\) is not supported" % name) as err:
            s.append_at({0: (0, np.array([0.0, 0.5, 1.0], dtype))})
        assert "SampledSolve.append_at needs a two-level reference" in str(err.value)
    with pytest.raises(ValueError, match="append_at"):
        s.append({0: np.zeros(3)})
    assert s.consumed == [0, 10] and s._known == [[], [(10, 20)]] and s.append_at({}) == {}
    # the interval limit: 256 one-sample intervals, the 257th refused, one that joins two accepted by the check
    s._known[0] = [(2 * k, 2 * k + 1) for k in range(50)]
    s.totals[0] = 1000
    s._known[0] += [(200 + 2 * k, 201 + 2 * k) for k in range(206)]
    assert len(s._known[0]) == 256
    with pytest.raises(ValueError, match="more than 256 known intervals"):
        s.append_at({0: (900, np.zeros(1))})
    assert s._check_interval(0, 1, 1) == 1 and s._check_interval(0, 99, 1) == 99
    s.plan = None
    for call in (lambda: s.append_at({0: (0, np.zeros(3))}), lambda: s.reference(0), lambda: s.known(0)):
        with pytest.raises(ValueError, match="closed"):
            call()


def test_the_default_rule_is_what_the_calibration_rules_pick():
    cal = json.load(open(os.path.join(ROOT, "profiles", "sampled_calibration.json")))
    assert "CPU" in cal["model"] and "synthetic" in cal["model"]
    assert cal["seeds"] == 40 and cal["durations"] == [600.0, 3600.0] and (cal["segment"], cal["W"], cal["E"]) == (6000, 6000, 300)
    pro = json.load(open(os.path.join(ROOT, "profiles", "progressive_calibration.json")))
    assert cal["k_grid"] == pro["k_grid"] and cal["m_grid"] == pro["m_grid"]  # the same grid
    assert (cal["min_psr"], cal["min_margin"], cal["offset_tolerance"]) == (pro["min_psr"], pro["min_margin"], pro["offset_tolerance"])
    assert {(c["k"], c["m"]) for c in cal["cells"]} == {(k, m) for k in cal["k_grid"] for m in cal["m_grid"]}
    assert all("prefix_mean_consumed" in c and "prefix_wrong_stops" in c for c in cal["cells"])  # the prefix schedule beside it
    for dur in cal["durations"]:
        for kind in ("matched", "wrong"):
            assert sum(f["duration"] == dur and f["kind"] == kind for f in cal["files"]) == cal["seeds"]
    rule = sampled.DEFAULT_SAMPLED_RULE
    assert isinstance(rule, StopRule)
    assert (rule.min_psr, rule.min_margin) == (quality.DEFAULT_MIN_PSR, quality.DEFAULT_MIN_MARGIN) == (cal["min_psr"], cal["min_margin"])
    assert rule.offset_tolerance == cal["offset_tolerance"] == 2 and rule.min_seconds == 0
    clean = [c for c in cal["cells"] if c["wrong_stops"] == 0]
    if not clean:
        assert rule.stable_updates is None and cal["shipped"]["stable_updates"] is None
        assert sampled.DEFAULT_SAMPLED_STABLE_UPDATES is None and not rule.settled([])
        return
    best = min(clean, key=lambda c: (c["mean_consumed"], c["k"], c["m"]))
    larger = [m for m in cal["m_grid"] if m > best["m"]]
    want = (best["k"] + 1, larger[0] if larger else best["m"])
    assert (rule.stable_updates, rule.min_ratio_margin) == want == (cal["shipped"]["stable_updates"], cal["shipped"]["min_ratio_margin"])
    assert (sampled.DEFAULT_SAMPLED_STABLE_UPDATES, sampled.DEFAULT_SAMPLED_MIN_RATIO_MARGIN) == want
