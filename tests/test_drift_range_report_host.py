"""The segment path report over a lag range on the CPU: the numpy model (tests/drift_range_report_model.py) against the
independent reference (tests/report_reference.py) on every pair of every range group and every added group, against
tests/drift_report_model.py at symmetric windows, its run grouping against the per-block statement, the host's work-item
tables under the sanitizers, and ``checked_cut_drift_sync``'s decision logic.  No GPU."""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import drift_path_cases as cases
import drift_range_model as drgm
import drift_range_report_cases as dc
import drift_range_report_model as m
import drift_report_model as drm
import piecewise_reference as pw
import report_cases as rc
import report_reference as rr
from test_gpu_split_optimum import RANGE_GROUPS, WINDOW_GROUPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference(pr, k):
    return pw.Reference(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"])


def _group(name, k, pairs, settings, first_call):
    """Every pair at every setting: the path of drift_range_model, the model's records against the reference's."""
    bad, facts, checked = [], rr.Facts(), 0
    for i, pr in enumerate(pairs):
        ref = _reference(pr, k)
        for si, setting in enumerate(settings):
            top_k, excl = rc.peak_args(first_call + si, max(p["hi"] - p["lo"] + 1 for p in pairs))
            offs, _, jump, _ = drgm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], *setting)
            recs, _ = m.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, pr["lo"], pr["hi"], offs, jump, top_k, excl)
            want = rr.segment_records(ref, offs, jump, top_k, excl)
            probs = rr.compare(ref, want, recs, len(recs), top_k, "segment", facts, (name, i))
            checked += 1
            if probs:
                bad.append((name, i, setting, (top_k, excl), probs[:3]))
    return dict(bad=bad, facts=facts, checked=checked, pairs=pairs, settings=settings)


@functools.lru_cache(maxsize=None)
def _range_group(gi):
    return _group("range K=%d" % RANGE_GROUPS[gi][0], RANGE_GROUPS[gi][0], rc.range_pairs(gi), rc.SEGMENT_SETTINGS,
                  gi * len(rc.SEGMENT_SETTINGS))


@functools.lru_cache(maxsize=None)
def _extra_group(name):
    k, pairs, settings = dc.extra_groups()[name]
    return _group(name, k, pairs, settings, dc.EXTRA_NAMES.index(name) * 2 + 1)


@pytest.mark.parametrize("gi", range(len(RANGE_GROUPS)))
def test_model_equals_the_reference_on_the_range_groups(gi):
    g = _range_group(gi)
    assert g["checked"] == len(RANGE_GROUPS[gi][2]) * len(rc.SEGMENT_SETTINGS)  # every pair (the F pair too), every setting
    assert not g["bad"], g["bad"][:5]


@pytest.mark.parametrize("name", dc.EXTRA_NAMES)
def test_model_equals_the_reference_on_the_added_groups(name):
    g = _extra_group(name)
    assert g["checked"] == len(g["pairs"]) * len(g["settings"])
    assert not g["bad"], g["bad"][:5]


def test_the_lists_reach_what_the_device_test_asserts():
    """Counted on the reference's own records: the device test's coverage conditions do not depend on device output."""
    facts = rr.Facts()
    for g in [_range_group(gi) for gi in range(len(RANGE_GROUPS))] + [_extra_group(name) for name in dc.EXTRA_NAMES]:
        facts.merge(g["facts"])
    assert dc.conditions_hold(facts), facts.counts()
    assert _extra_group("rounds")["facts"].many >= 1 and _extra_group("long")["facts"].first_1024 >= 1
    assert _extra_group("single")["facts"].single_shift >= 1 and _extra_group("wide")["facts"].flat_second_chunk >= 1
    assert _extra_group("edge288")["facts"].nan_inside + _extra_group("edge800")["facts"].nan_inside >= 1
    assert _range_group(0)["facts"].no_overlap >= 2  # (910, 1400) at R = 900
    assert facts.worst <= facts.worst_tol and facts.worst_tol > 0  # an F pair went through the tolerance path


@pytest.mark.parametrize("gi", range(len(WINDOW_GROUPS)))
def test_symmetric_windows_equal_the_windowed_model(gi):
    """At [-W+1, W], given the windowed solve's path, the records are drift_report_model's byte for byte."""
    k, w, _, _ = WINDOW_GROUPS[gi]
    for i, pr in enumerate(cases.window_pairs(gi)):
        for si in (0, 2):
            setting = rc.SEGMENT_SETTINGS[si]
            top_k, excl = rc.peak_args(gi + si, 2 * w)
            (offs, _, jump, _), want, _ = drm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, w, *setting, top_k, excl)
            got, _ = m.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], k, -w + 1, w, offs, jump, top_k, excl)
            assert got.tobytes() == want.tobytes(), (gi, i, setting)


def test_run_sums_equal_block_sums_on_a_path_that_steps_every_block():
    """The four integer sums of a run of equal-offset blocks are the sums of its blocks': the per-block sample ranges of
    consecutive blocks at one lag concatenate.  A path that steps every block, one that never does, and mixed ones,
    at ranges that cut the reference off on either side."""
    rng = np.random.RandomState(5)
    k = 256
    for S, R, lo, hi in ((256 * 9 + 33, 2000, -700, 900), (256 * 6 + 1, 3000, -2000, 2500), (256 * 4, 500, -300, 1200)):
        rb, sb = rng.rand(R) < 0.4, rng.rand(S) < 0.5
        bits = m.Bits(rb, sb)
        B = (S + k - 1) // k
        for path in (lo + 300 + 7 * np.arange(B), np.full(B, (lo + hi) // 2), lo + 100 + 5 * (np.arange(B) // 3),
                     hi - 40 - 3 * (np.arange(B) % 2)):
            assert path.min() >= lo and path.max() <= hi
            a = m.path_sums(bits, k, lo, hi, 0, B, path)
            b = m.path_sums(bits, k, lo, hi, 0, B, path, by_block=True)
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            assert len(m.runs_of(path, 0, B)) <= len(m.runs_of(path, 0, B, by_block=True)) == B
        stepping = lo + 300 + 7 * np.arange(B)
        assert len(m.runs_of(stepping, 0, B)) == B


def test_the_scheduler_tables_hold_under_the_sanitizers(tmp_path):
    """tests/drift_range_sched_check.cpp (its own main; csrc/ffs_drift_range_sched.h alone, no HIP) built with the host
    compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run as a program of its own."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "sched_check")
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []  # (clang's default)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    "-o", exe, os.path.join(ROOT, "tests", "drift_range_sched_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stdout.startswith("ok: "), out.stdout


# ---- host decision logic ---------------------------------------------------------------------------------------------

def _seg(psr=20.0, gain_prev=math.nan, gain_next=math.nan, drift_gain=0.0, lo=0, hi=0, flags=0, first_block=0):
    from ffsubsync_amd.drift_report import SegmentQuality

    return SegmentQuality(first_block, first_block + 4, first_block * 1024, (first_block + 4) * 1024, lo, hi, lo, hi, 1.0,
                          math.nan, math.nan, 0.5, lo, [(1.0, 0)], 0.0, 0.05, 1000, psr, math.inf, gain_prev, gain_next,
                          drift_gain, flags)


def test_the_decision_follows_the_module_defaults():
    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_range_report as drr

    psr, gain, dg = drr.DEFAULT_MIN_SEGMENT_PSR, drr.DEFAULT_MIN_GAIN, drr.DEFAULT_MIN_DRIFT_GAIN
    ok, reasons = drr.decide_drift([_seg(psr=psr)])
    assert ok and reasons == []
    ok, reasons = drr.decide_drift([_seg(psr=psr - 0.01)])
    assert not ok and reasons == ["segment 0: psr %.1f < %.1f" % (psr - 0.01, psr)]
    ok, reasons = drr.decide_drift([_seg(flags=_native.QUALITY_FLAT)])
    assert not ok and "flat" in reasons[0]
    two = [_seg(gain_next=gain), _seg(gain_prev=gain, first_block=4)]
    assert drr.decide_drift(two) == (True, [])
    two[1] = _seg(gain_prev=gain - 0.01, first_block=4)
    ok, reasons = drr.decide_drift(two)
    assert not ok and reasons[0].startswith("jump 0 (block 4)")
    two[1] = _seg(gain_prev=math.nan, first_block=4)  # the neighbour's path does not fit the range
    assert not drr.decide_drift(two)[0]
    assert drr.decide_drift([_seg(lo=5, hi=9, drift_gain=dg)]) == (True, [])
    ok, reasons = drr.decide_drift([_seg(lo=5, hi=9, drift_gain=dg - 0.01)])
    assert not ok and "drift gain" in reasons[0]
    assert drr.decide_drift([_seg(lo=5, hi=5, drift_gain=-3.0)])[0]  # no step taken: nothing to prove
    # explicit thresholds override the defaults
    assert drr.decide_drift([_seg(psr=3.0)], min_segment_psr=2.0)[0]
    assert not drr.decide_drift([_seg(psr=30.0)], min_segment_psr=31.0)[0]


def test_validate_refuses_before_any_native_call():
    from ffsubsync_amd import drift_range_report as drr

    for kw in (dict(block_samples=100), dict(split_penalty=-1.0), dict(max_step=8), dict(step_cost=math.nan),
               dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0)):
        args = dict(block_samples=1024, split_penalty=8192.0, max_step=2, step_cost=64.0, top_k=3, exclusion_samples=300)
        args.update(kw)
        with pytest.raises(ValueError):
            drr.validate_args(**args)
    for kw in (dict(min_segment_psr=math.nan), dict(min_gain="8"), dict(min_drift_gain=None), dict(min_gain=True)):
        args = dict(min_segment_psr=9.0, min_gain=8.0, min_drift_gain=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            drr.validate_thresholds(**args)
    with pytest.raises(ValueError):
        drr.checked_cut_drift_sync([], min_segment_psr=math.nan)
    with pytest.raises(ValueError):
        drr.checked_cut_drift_sync([], lag_range=(5, 4))
    with pytest.raises(ValueError):
        drr.checked_cut_drift_sync([], min_coverage=2.0)


def test_the_binding_counts_the_report_workspace_as_the_header_states():
    from ffsubsync_amd import _native

    class P:
        pairs_in_flight, max_blocks, max_lags, max_samples = 1, 704, 1439999, 720000
    lpad = -(-(1439999 + 1) // 64) * 64
    assert _native.DriftRangePlan.report_bytes(P) == 8 * lpad * 12 + 2 * (-(-22500 // 512) + 704) * 32
    assert 138.0e6 < _native.DriftRangePlan.report_bytes(P) < 138.5e6  # the 2 h full-range figure of DESIGN 3.17
