"""The Python layer of the joint cue retiming (ffsubsync_amd.cue_retime) without a GPU: apply_retime, every
Python-side refusal by its message, the workspace rule, the workload's truth, and the calibrated defaults against
profiles/cue_retime_calibration.json on four seeds of workloads/cue_stretches.py."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "profiles"))

import retime_model as rm  # noqa: E402
from ffsubsync_amd import _native  # noqa: E402
from ffsubsync_amd import cue_retime as ct  # noqa: E402

CALIBRATION = os.path.join(os.path.dirname(HERE), "profiles", "cue_retime_calibration.json")


def test_constants_and_layouts_match_the_model():
    assert _native.CUE_RETIME_DTYPE.itemsize == rm.DTYPE.itemsize == 64
    assert _native.RETIME_SUMMARY_DTYPE.itemsize == rm.SUMMARY.itemsize == 40
    assert [(n, _native.CUE_RETIME_DTYPE.fields[n][1]) for n in rm.DTYPE.names] == [(n, rm.DTYPE.fields[n][1]) for n in rm.DTYPE.names]
    assert [(n, _native.RETIME_SUMMARY_DTYPE.fields[n][1]) for n in rm.SUMMARY.names] == [(n, rm.SUMMARY.fields[n][1]) for n in rm.SUMMARY.names]
    assert (_native.RETIME_EMPTY, _native.RETIME_INVALID, _native.RETIME_MOVED, _native.RETIME_JUMP, _native.RETIME_UNORDERED,
            _native.RETIME_ORDER_TIGHT, _native.RETIME_AT_EDGE) == (rm.EMPTY, rm.INVALID, rm.MOVED, rm.JUMP, rm.UNORDERED,
                                                                    rm.ORDER_TIGHT, rm.AT_EDGE)
    assert (_native.RETIME_MAX_RADIUS, _native.RETIME_Q, _native.RETIME_NO_JUMP, _native.RETIME_KEEP_ORDER) == (
        rm.MAX_RADIUS, rm.Q, rm.NO_JUMP, rm.KEEP_ORDER)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ffsubsync_amd.h")).read()
    for text in ("#define FFS_RETIME_MAX_RADIUS 1024", "#define FFS_RETIME_Q 64", "#define FFS_RETIME_NO_JUMP (-1)",
                 "#define FFS_RETIME_WORK_CAP (256ll << 20)", "#define FFS_RETIME_KEEP_ORDER 1",
                 "THE PAIR'S LEVELS DO NOT ENTER THE RETIME"):
        assert text in header
    assert "ffs_cue_retime_batch" in _native.EXPORTED_SYMBOLS and _native.RETIME_WORK_CAP == 256 << 20


def test_apply_retime_moves_every_live_cue():
    recs = np.zeros(4, rm.DTYPE)
    recs["delta"] = [0, -120, 7, 0]
    recs["flags"] = [0, rm.MOVED, rm.MOVED | rm.JUMP, rm.EMPTY]
    start = np.arange(4, dtype=np.int64) * 5_000_000
    end = start + 2_000_000
    new_s, new_e = ct.apply_retime(start, end, recs, 100)
    assert np.array_equal(new_s - start, [0, -1_200_000, 70_000, 0]) and np.array_equal(new_e - end, new_s - start)
    assert new_s is not start and start[1] == 5_000_000  # copies
    cues = [ct.from_record(x) for x in recs]
    assert [c.moved for c in cues] == [False, True, True, False] and cues[2].jump and cues[3].skipped and not cues[0].at_edge
    again = ct.apply_retime(start, end, cues, 100)
    assert np.array_equal(again[0], new_s) and np.array_equal(again[1], new_e)
    with pytest.raises(ValueError, match="one record per cue"):
        ct.apply_retime(start, end, recs[:3], 100)
    summ = np.zeros((), rm.SUMMARY)
    summ["total"], summ["n_jumps"] = -5, 2
    assert ct.summary_from_record(summ) == ct.RetimeSummary(-5, 0, 0, 0, 0, 2)


def _fake_batch(n=2, dtype=None, ref_dtype=None, n_cand=1, hi=1.0, lens=None):
    dtype = _native.FFS_DTYPE_U1 if dtype is None else dtype
    return SimpleNamespace(n_pairs=n, n_cand=n_cand, dtype=dtype, ref_dtype=ref_dtype,
                           lens=np.full((n, 2), 100, np.int64) if lens is None else lens, lo=np.zeros((n, 2)),
                           hi=np.full((n, 2), hi))


def test_python_side_refusals_name_the_problem():
    z = np.zeros(3, np.int64)
    good = [(z, z, z), (z, z, z)]
    with pytest.raises(ValueError, match="multi-level float reference .FFS_DTYPE_F64. is not supported"):
        ct.retime_batch(_fake_batch(ref_dtype=_native.FFS_DTYPE_F64), good)
    with pytest.raises(ValueError, match="multi-level float reference .FFS_DTYPE_F32. is not supported"):
        ct.retime_batch(_fake_batch(dtype=_native.FFS_DTYPE_F32), good)
    with pytest.raises(ValueError, match="needs two-level vectors"):
        ct.retime_batch(_fake_batch(dtype=_native.FFS_DTYPE_RUNS), good)
    with pytest.raises(ValueError, match="two-level vectors need finite levels"):
        ct.retime_batch(_fake_batch(hi=np.inf), good)
    with pytest.raises(ValueError, match="one candidate per pair"):
        ct.retime_batch(_fake_batch(n_cand=7), good)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        ct.retime_batch(_fake_batch(lens=np.array([[100, 100], [100, 0]])), good)
    with pytest.raises(ValueError, match="pair 1: 3 starts, 2 ends and 3 lags"):
        ct.retime_batch(_fake_batch(), [(z, z, z), (z, z[:2], z)])
    with pytest.raises(ValueError, match="1 cue tables for 2 pairs"):
        ct.retime_batch(_fake_batch(), good[:1])
    big = np.zeros(30000, np.int64)
    with pytest.raises(ValueError, match="pair 1: 30000 cues x 2049 shifts x 6 bytes exceed the retime workspace cap"):
        ct.retime_batch(_fake_batch(), [(z, z, z), (big, big, big)], radius=1024)
    for bad in (-1, 1025, 1.5):
        with pytest.raises(ValueError, match="radius=.*need an integer in .0, 1024."):
            ct.retime_batch(_fake_batch(), good, radius=bad)
    for bad in (-1, 65537, 0.5):
        with pytest.raises(ValueError, match="context_samples=.*need an integer in .0, 65536."):
            ct.retime_batch(_fake_batch(), good, context=bad)
    for bad in (-1, (1 << 20) + 1, 2.5):
        with pytest.raises(ValueError, match="penalty_q=.*need an integer in .0, 2.20."):
            ct.retime_batch(_fake_batch(), good, penalty_q=bad)
    for bad in (-2, (1 << 40) + 1, 0.5):
        with pytest.raises(ValueError, match="jump_q=.*need -1 .no cap. or an integer in .0, 2.40."):
            ct.retime_batch(_fake_batch(), good, jump_q=bad)
    track = (np.array([0, 2_000_000]), np.array([1_000_000, 3_000_000]), np.zeros(2, np.uint8))
    res = SimpleNamespace(ratio=1.0, cue_start_us=track[0], cue_end_us=track[1])
    with pytest.raises(ValueError, match="retime_sync needs two-level references: reference 0 is a multi-level float"):
        ct.retime_sync([(np.array([0.0, 0.4, 1.0, 0.6]), track)], [res])
    with pytest.raises(ValueError, match="problem 0: the reference has non-finite levels"):
        ct.retime_sync([(np.array([0.0, np.nan, 1.0]), track)], [res])
    with pytest.raises(ValueError, match="problem 0: 2 cues, 1 output times"):
        ct.retime_sync([(np.array([0.0, 1.0]), track)], [SimpleNamespace(ratio=1.0, cue_start_us=track[0][:1])])
    with pytest.raises(ValueError, match="1 results for 2 problems"):
        ct.retime_sync([(np.array([0.0, 1.0]), track)] * 2, [res])
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        ct.retime_sync([(np.array([0.0, 1.0]), (track[0][:0], track[1][:0], track[2][:0]))], [res])
    with pytest.raises(ValueError, match="radius="):
        ct.retime_sync([(np.array([0.0, 1.0]), track)], [res], radius=2000)


def test_workspace_rule():
    assert ct.workspace_bytes([3, 0, 5], 1, 1) == 256 and ct.workspace_bytes([3, 0, 5], 1, 3) == 256
    assert ct.workspace_bytes([100, 50, 7], 10, 2) == -(-150 * 21 * 6 // 256) * 256
    assert ct.workspace_bytes([100, 50, 700], 10, 2) == -(-700 * 21 * 6 // 256) * 256
    assert ct.workspace_bytes([], 10, 2) == 0 and ct.workspace_bytes([0, 0], 10, 2) == 0
    cell = 2049 * 6
    assert ct.workspace_bytes([9000] * 3, 1024, 3) == -(-18000 * cell // 256) * 256  # the cap cuts after two pairs
    assert ct.workspace_bytes([9000] * 3, 1024, 1) == -(-9000 * cell // 256) * 256


def test_the_workload_records_its_truth():
    from workloads import cue_stretches as ws

    pr = ws.make_stretch_problem(3, 1800.0)
    again = ws.make_stretch_problem(3, 1800.0)
    assert np.array_equal(pr.start_us, again.start_us) and np.array_equal(pr.displacement, again.displacement)
    assert np.all(np.diff(pr.start_us) >= 0)  # file order
    assert set(np.unique(pr.kind)) == {ws.UNTOUCHED, ws.STRETCH, ws.ISOLATED, ws.EXTRA}
    assert not pr.displacement[(pr.kind == ws.UNTOUCHED) | (pr.kind == ws.EXTRA)].any()
    for j in np.unique(pr.stretch[pr.stretch >= 0]):
        d = pr.displacement[pr.stretch == j]
        assert 3 <= d.size <= 12 and np.abs(d).max() - np.abs(d).min() <= 1 and 76 <= np.abs(d).min() <= 261  # 0.8-2.5 s at a ratio in [0.959, 1.043]
    assert (pr.stretch >= 0).sum() == (pr.kind == ws.STRETCH).sum()
    iso = np.abs(pr.displacement[pr.kind == ws.ISOLATED])
    assert iso.size == 16 and ((iso >= 76) & (iso <= 261)).all()


def test_defaults_reach_the_calibrated_figures_on_four_seeds():
    """The model at the defaults, on the first four 10-minute seeds, against the figures the calibration wrote for those
    seeds (the same model produced them: equality), and the rule's pick against the table."""
    import cue_retime_calibration as cal

    with open(CALIBRATION) as f:
        doc = json.load(f)
    assert "synthetic data only; nobody has measured real files" in doc["note"]
    chosen = doc["chosen"]
    assert (ct.DEFAULT_RADIUS, ct.DEFAULT_CONTEXT, ct.DEFAULT_PENALTY_Q, ct.DEFAULT_JUMP_Q) == (
        chosen["radius"], chosen["context"], chosen["penalty_q"], chosen["jump_q"])
    long = doc["table"]["7200"]
    base, pick = long["baseline"], long[chosen["key"]]
    assert pick["untouched_moved_share"] <= base["untouched_moved_share"]
    for k, cell in long.items():  # the rule: no allowed setting recovers more of the stretch class
        if k != "baseline" and cell["untouched_moved"] * base["n_untouched"] <= base["untouched_moved"] * cell["n_untouched"]:
            assert (cell["stretch_recovered"], cell["isolated_recovered"]) <= (pick["stretch_recovered"], pick["isolated_recovered"])
    assert len(long) == 1 + 2 * 3 * 5 * 4 and doc["seeds"] == 64
    for seed in range(4):
        want = doc["per_seed"]["600"]["%d" % seed]
        pr, table, sub = cal.problem(seed, 600.0)
        got = cal.retime_figures(pr, table, sub, ct.DEFAULT_RADIUS, ct.DEFAULT_CONTEXT,
                                 [(ct.DEFAULT_PENALTY_Q, ct.DEFAULT_JUMP_Q)])[0]
        assert got == want["retime"], (seed, got, want)
        assert cal.baseline_figures(pr, table, sub) == want["baseline"], seed
        assert got["order_violations"] == 0
