"""The Python layer of the per-cue evidence report (ffsubsync_amd.cue_report) without a GPU: cue_table on
the golden rasters' tracks, assess_cues / snap_cues on hand-made records, every Python-side refusal by its message, and
the calibrated defaults against profiles/cue_report_calibration.json on four seeds of workloads/cues.py."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cue_model as cm  # noqa: E402
from ffsubsync_amd import _native  # noqa: E402
from ffsubsync_amd import cue_report as cr  # noqa: E402
from ffsubsync_amd.split_align import Piece, _scaled_us, map_cues  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "raster_golden.npz"))
RATIOS = [float(r) for r in GOLD["ratios"]]
CALIBRATION = os.path.join(os.path.dirname(HERE), "profiles", "cue_report_calibration.json")


@pytest.mark.parametrize("name", ["a", "b"])
def test_cue_table_intervals_reproduce_the_golden_rasters(name):
    s, e, m = GOLD[name + "_start_us"], GOLD[name + "_end_us"], GOLD[name + "_meta"]
    assert int(GOLD[name + "_start_seconds"]) == 0
    for j, ratio in enumerate(RATIOS):
        want = (GOLD["%s_r%d" % (name, j)] != 0).astype(np.uint8)
        out = np.array([_scaled_us(u, ratio) for u in s], dtype=np.int64)
        a, b, lag = cr.cue_table(s, e, ratio, out, 100, m)
        assert a.size == s.size and not lag.any()
        got = np.zeros(want.size, np.uint8)
        for x, y in zip(a, b):
            assert 0 <= x <= y <= want.size
            got[x:y] = 1
        assert np.array_equal(got, want), (name, j)
        assert all(x == y == 0 for x, y, meta in zip(a, b, m) if meta)
        # without the metadata flags every cue contributes its own run, the flagged ones included
        a2, b2, _ = cr.cue_table(s, e, ratio, out, 100)
        assert np.array_equal(a2[m == 0], a[m == 0]) and np.array_equal(b2[m == 0], b[m == 0])


def test_cue_table_lags_are_the_pieces_offsets_and_a_polyline_shift_rounds_as_rint():
    s, e = GOLD["a_start_us"], GOLD["a_end_us"]
    ratio = RATIOS[1]
    n = _native.raster_length(e, ratio, 100)
    cut1, cut2 = (n // 3) // 1024 * 1024, (2 * n // 3) // 1024 * 1024
    pieces = [Piece(0, cut1 // 1024, 0, cut1, 1234, 0.0), Piece(cut1 // 1024, cut2 // 1024, cut1, cut2, -77, 0.0),
              Piece(cut2 // 1024, -(-n // 1024), cut2, n, 59999, 0.0)]
    cs, ce, which = map_cues(s, e, ratio, pieces, 100)
    _, _, lag = cr.cue_table(s, e, ratio, cs, 100)
    assert len(set(which.tolist())) == 3
    assert np.array_equal(lag, np.array([p.offset for p in pieces], dtype=np.int64)[which])
    scaled = np.array([_scaled_us(u, ratio) for u in s[:8]], dtype=np.int64)
    shift_us = np.array([1234567, 5000, 15000, -5000, -15000, 25000, 4999, -1234567])  # x.5 samples: half to even
    _, _, lag = cr.cue_table(s[:8], e[:8], ratio, scaled + shift_us, 100)
    assert lag.tolist() == [123, 0, 2, 0, -2, 2, 0, -123]
    assert lag.tolist() == np.rint(shift_us * 100 / 1e6).astype(np.int64).tolist()


def _rep(**kw):
    base = dict(start=100, end=300, lag=50, lo=0, hi=400, own=(400, 150, 200, 190), best=(400, 150, 200, 190),
                own_score=100.0, best_score=100.0, best_delta=0, n_best=1, cue_own_n11=190, cue_own_ov=200,
                cue_max_n11=195, cue_max_delta=0, flags=0)
    base.update(kw)
    return cr.CueReport(**base)


def test_assess_and_snap_on_hand_made_records():
    reps = [
        _rep(),  # ok
        _rep(flags=_native.CUE_EMPTY, cue_own_ov=0, cue_own_n11=0),  # empty
        _rep(flags=_native.CUE_INVALID),  # an invalid lag reads as empty
        _rep(flags=_native.CUE_SILENT, cue_max_n11=0, cue_own_n11=0, best_delta=9, best_score=500.0),  # silent wins
        _rep(best_delta=-120, best_score=100.0 + 0.2 * 400),  # shifted: gain = 0.2 (U - L) >= min_gain (U - L)
        _rep(best_delta=-120, best_score=100.0 + 0.2 * 400 - 1e-9, cue_own_n11=10),  # just under: uncovered instead
        _rep(best_delta=300, best_score=900.0, flags=_native.CUE_BEST_AT_EDGE),  # at the edge: not shifted; covered: ok
        _rep(best_delta=0, best_score=100.0, cue_own_n11=99),  # cover 0.495 < 0.5
        _rep(cue_own_n11=100),  # cover 0.5: ok
        _rep(best_delta=7, best_score=100.0 + 0.2 * 400 + 1.0),  # shifted
    ]
    verdicts = cr.assess_cues(reps, min_gain=0.2, min_cover=0.5)
    assert verdicts == ["ok", "empty", "empty", "silent", "shifted", "uncovered", "ok", "uncovered", "ok", "shifted"]
    assert reps[4].gain == 80.0 and reps[7].cover == 0.495 and reps[1].cover == 0.0
    start = np.arange(10, dtype=np.int64) * 5_000_000
    end = start + 2_000_000
    new_s, new_e = cr.snap_cues(start, end, reps, verdicts, 100)
    move = np.zeros(10, np.int64)
    move[4], move[9] = -1_200_000, 70_000
    assert np.array_equal(new_s, start + move) and np.array_equal(new_e, end + move)
    assert new_s is not start and start[4] == 20_000_000  # copies
    with pytest.raises(ValueError, match="one report and one verdict per cue"):
        cr.snap_cues(start, end, reps[:3], verdicts, 100)
    rec = np.zeros((), cm.DTYPE)
    rec["best"], rec["best_delta"], rec["flags"], rec["best_score"] = [4, 3, 2, 1], -5, 40, 2.5
    back = cr.from_record(rec)
    assert back.best == (4, 3, 2, 1) and back.best_delta == -5 and back.silent and back.at_edge and back.best_score == 2.5


def _fake_batch(n=2, dtype=None, ref_dtype=None, n_cand=1, hi=1.0, lens=None):
    dtype = _native.FFS_DTYPE_U1 if dtype is None else dtype
    return SimpleNamespace(n_pairs=n, n_cand=n_cand, dtype=dtype, ref_dtype=ref_dtype,
                           lens=np.full((n, 2), 100, np.int64) if lens is None else lens, lo=np.zeros((n, 2)),
                           hi=np.full((n, 2), hi))


def test_python_side_refusals_name_the_problem():
    z = np.zeros(3, np.int64)
    good = [(z, z, z), (z, z, z)]
    with pytest.raises(ValueError, match="multi-level float reference .FFS_DTYPE_F64. is not supported"):
        cr.cue_report_batch(_fake_batch(ref_dtype=_native.FFS_DTYPE_F64), good)
    with pytest.raises(ValueError, match="multi-level float reference .FFS_DTYPE_F32. is not supported"):
        cr.cue_report_batch(_fake_batch(dtype=_native.FFS_DTYPE_F32), good)
    with pytest.raises(ValueError, match="needs two-level vectors"):
        cr.cue_report_batch(_fake_batch(dtype=_native.FFS_DTYPE_RUNS), good)
    with pytest.raises(ValueError, match="two-level vectors need finite levels"):
        cr.cue_report_batch(_fake_batch(hi=np.inf), good)
    with pytest.raises(ValueError, match="one candidate per pair"):
        cr.cue_report_batch(_fake_batch(n_cand=7), good)
    with pytest.raises(ValueError, match="cannot align empty speech data"):
        cr.cue_report_batch(_fake_batch(lens=np.array([[100, 100], [100, 0]])), good)
    with pytest.raises(ValueError, match="pair 1: 3 starts, 2 ends and 3 lags: the three cue arrays need one length"):
        cr.cue_report_batch(_fake_batch(), [(z, z, z), (z, z[:2], z)])
    with pytest.raises(ValueError, match="1 cue tables for 2 pairs"):
        cr.cue_report_batch(_fake_batch(), good[:1])
    with pytest.raises(ValueError, match="a .start, end, lag. triple"):
        cr.cue_report_batch(_fake_batch(), [(z, z), (z, z, z)])
    for bad in (-1, 4097, 1.5):
        with pytest.raises(ValueError, match="radius_samples=.*need an integer in .0, 4096."):
            cr.cue_report_batch(_fake_batch(), good, radius_samples=bad)
    for bad in (-1, 65537, 0.5):
        with pytest.raises(ValueError, match="context_samples=.*need an integer in .0, 65536."):
            cr.cue_report_batch(_fake_batch(), good, context_samples=bad)
    with pytest.raises(ValueError, match="3 starts, 2 ends and 3 output starts"):
        cr.cue_table(z, z[:2], 1.0, z)
    track = (np.array([0, 2_000_000]), np.array([1_000_000, 3_000_000]), np.zeros(2, np.uint8))
    res = SimpleNamespace(ratio=1.0, cue_start_us=track[0], cue_end_us=track[1])
    with pytest.raises(ValueError, match="reference 0 is a multi-level float reference"):
        cr.cue_report_sync([(np.array([0.0, 0.4, 1.0, 0.6]), track)], [res])
    with pytest.raises(ValueError, match="problem 0: the reference has non-finite levels"):
        cr.cue_report_sync([(np.array([0.0, np.nan, 1.0]), track)], [res])
    with pytest.raises(ValueError, match="problem 0: 2 cues, 1 output times"):
        cr.cue_report_sync([(np.array([0.0, 1.0]), track)], [SimpleNamespace(ratio=1.0, cue_start_us=track[0][:1])])
    with pytest.raises(ValueError, match="1 results for 2 problems"):
        cr.cue_report_sync([(np.array([0.0, 1.0]), track)] * 2, [res])


def test_flat_cue_table_layout():
    table, first, count = cr.flat_cue_table([([1, 2], [3, 4], [5, 6]), ([], [], []), ([7], [8], [-9])], 3)
    assert table.dtype.itemsize == 24 and first.tolist() == [0, 2, 2] and count.tolist() == [2, 0, 1]
    assert table.view(np.int64).tolist() == [1, 3, 5, 2, 4, 6, 7, 8, -9]


def test_defaults_reach_the_calibrated_figures_on_four_seeds():
    """The verdicts of the model at the defaults, on the first four 10-minute seeds, against the figures the calibration
    wrote for those seeds (the same model produced them: no margin)."""
    from workloads import cues as wc

    with open(CALIBRATION) as f:
        doc = json.load(f)
    assert "synthetic data only; nobody has measured real files" in doc["note"]
    chosen = doc["chosen"]
    assert (cr.DEFAULT_RADIUS, cr.DEFAULT_CONTEXT, cr.DEFAULT_MIN_GAIN, cr.DEFAULT_MIN_COVER) == (
        chosen["radius"], chosen["context"], chosen["min_gain"], chosen["min_cover"])
    for seed in range(4):
        want = doc["per_seed"]["600"]["%d" % seed]
        pr = wc.make_cue_problem(seed, 600.0)
        res = wc.true_sync(pr)
        table = cr.cue_table(pr.start_us, pr.end_us, res.ratio, res.cue_start_us)
        recs = cm.cue_report(pr.ref, wc.host_subtitle_vector(pr), table, cr.DEFAULT_RADIUS, cr.DEFAULT_CONTEXT, (0.0, 1.0),
                             (0.0, min(1.0 / pr.ratio, 1.0)))
        verdicts = np.array(cr.assess_cues([cr.from_record(x) for x in recs]))
        err = np.abs(recs["best_delta"].astype(np.int64) + pr.displacement)
        moved, plain = pr.kind == wc.DISPLACED, pr.kind == wc.UNTOUCHED
        assert int(moved.sum()) == want["n_displaced"] and int(plain.sum()) == want["n_untouched"]
        found = int(((verdicts == "shifted") & (err <= doc["err_ok_samples"]) & moved).sum())
        false = int(((verdicts != "ok") & plain).sum())
        assert found >= want["displaced_found"], (seed, found, want)  # recall
        assert false <= want["untouched_flagged"], (seed, false, want)  # false positives
