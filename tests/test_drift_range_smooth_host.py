"""The smooth drift fit over a lag range on the CPU: the numpy model tests/drift_range_smooth_model.py (the contract of
csrc/ffs_drift_range_smooth.h) against drift_smooth_model at [-W+1, W], against direct counting and exhaustive
enumeration, its identities, the lag range's edge, the bound the device's band rows rest on, the Python layer's argument
checks and the ABI.  Every comparison is exact."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import drift_range_model as drg
import drift_range_smooth_model as drsm
import drift_report_model as drm
import drift_smooth_model as dsm
from drift_range_smooth_cases import SMALL, coverage, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_fit(got, want):
    return (np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3].tobytes() == want[3].tobytes()
            and np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][2], want[0][2])
            and np.array_equal(_bits(got[0][1]), _bits(want[0][1])) and _bits([got[0][3]])[0] == _bits([want[0][3]])[0])


def _windowed(seed):
    """A small problem for both models: the range is [-W+1, W]."""
    rng = np.random.RandomState(500 + seed)
    R, S = int(rng.randint(700, 6000)), int(rng.randint(700, 6000))
    k = int(rng.choice([256, 512]))
    w = int(rng.choice([40, 300, 1500]))
    seg = np.maximum(1, rng.geometric(1.0 / 40.0, size=R // 10 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    i = np.arange(S)
    idx = i + int(rng.randint(-w, w)) + i // int(rng.randint(100, 500)) + np.where(i < S // 2, 0, int(rng.randint(-w, w)))
    sb = np.zeros(S, bool)
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.05
    rb[0], rb[1], sb[0], sb[1] = True, False, True, False
    return dict(rb=rb, sb=sb, r_lv=[(0.0, 1.0), (-1.0, 2.5)][seed % 2], s_lv=[(0.0, 1.0), (0.0, 0.96), (-0.5, 1.25)][seed % 3],
                k=k, w=w, p=[0.0, 60.0, np.inf][seed % 3], s=seed % 8, q=[0.0, 1.0, 16.0][seed % 3],
                m=[1, 2, 3, 8, 256][seed % 5], r=[0, 1, 5, 16][seed % 4], lam=[0.0, 1.0, 64.0][(seed // 2) % 3])


@pytest.mark.parametrize("seed", range(12))
def test_symmetric_range_equals_the_windowed_model(seed):
    pr = _windowed(seed)
    args = (pr["p"], pr["s"], pr["q"], pr["m"], pr["r"], pr["lam"])
    want = dsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["w"], *args)
    got = drsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], -pr["w"] + 1, pr["w"], *args)
    assert _same_fit(got, want)


def test_symmetric_range_equals_the_windowed_model_on_a_two_hour_pair():
    """workloads/drift.py seed 3 at W = 6000 and drift_smooth's defaults; the drift path is the windowed model's (the two
    DPs are held equal by tests/test_drift_range_host.py), the fit runs on both counts objects."""
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    pr, w = drift.make_problem(3), 6000
    lv = ((0.0, 1.0), (0.0, pr.sub_hi))
    want = dsm.solve(pr.ref, pr.sub, *lv, 1024, w, da.DEFAULT_SPLIT_PENALTY, da.DEFAULT_MAX_STEP, da.DEFAULT_STEP_COST,
                     ds.DEFAULT_KNOT_BLOCKS, ds.DEFAULT_RADIUS, ds.DEFAULT_BEND_COST)
    got = drsm.solve(pr.ref, pr.sub, *lv, 1024, -w + 1, w, None, None, None, ds.DEFAULT_KNOT_BLOCKS, ds.DEFAULT_RADIUS,
                     ds.DEFAULT_BEND_COST, drift=want[0])
    assert _same_fit(got, want) and np.count_nonzero(want[1] != want[0][0]) > 100


def test_line_scores_equal_direct_counting():
    """Every line of the longest segment's first interval against brute_line_score; among the problems are ranges past
    both overlap edges and without any overlap, so lines with blocks of partial and of no overlap are met."""
    partial = empty = done = 0
    for i in (0, 3, 5, 9, 11, 15, 17, 21, 35):
        pr = SMALL[i]
        (off, _, jump, _), _, _, _ = model(i)
        f, e = max(drm.segments_of(jump), key=lambda s: s[1] - s[0])
        if e - f < 2:
            continue
        r, n = 2, e - 1 - f
        cnt = drsm.RangeCounts(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"])
        tab = dsm.line_table(cnt, off, f, n, True, r)
        for a, b in itertools.product(range(2 * r + 1), repeat=2):
            c0, c1 = int(off[f]) + a - r, int(off[e - 1]) + b - r
            if not (cnt.valid(c0) and cnt.valid(c1)):
                assert tab[a, b] == -np.inf
                continue
            lags = [int(x) for x in dsm.digital_line(c0, c1, n, np.arange(n + 1))]
            want = dsm.brute_line_score(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], range(f, e), lags)
            assert _bits([tab[a, b]])[0] == _bits([want])[0], (i, a, b)
            ov = [min((blk + 1) * pr["k"], pr["sb"].size, pr["rb"].size - d) - max(blk * pr["k"], -d)
                  for blk, d in zip(range(f, e), lags)]
            full = [min((blk + 1) * pr["k"], pr["sb"].size) - blk * pr["k"] for blk in range(f, e)]
            partial += any(0 < x < y for x, y in zip(ov, full))
            empty += all(x <= 0 for x in ov)
            if all(x <= 0 for x in ov):
                assert tab[a, b] == 0.0
        done += 1
    assert done >= 5 and partial >= 1 and empty >= 1, (done, partial, empty)


def test_viterbi_total_equals_exhaustive_enumeration_on_exact_tables():
    """0/1 levels make every line score an integer; with power-of-two intervals and an integer bend cost every sum is
    exact, so the fit's total must be the maximum over ALL knot lags."""
    rng = np.random.RandomState(21)
    done = 0
    for trial in range(6):
        k, m, r = 256, [2, 4][trial % 2], 1 + trial % 2
        blocks = [2 * m + 1, 3 * m + 1][trial % 2]
        rb = rng.rand(blocks * k + 600) < 0.5
        i = np.arange(blocks * k)
        sb = rb[i + 100 + i // (2 * k)]
        sb ^= rng.rand(sb.size) < 0.05
        lo, hi = [(-50, 400), (99, 103), (-1000, 3000)][trial % 3]
        off, _, jump, _ = drg.solve(rb, sb, (0.0, 1.0), (0.0, 1.0), k, lo, hi, np.inf, 2, 1.0)
        cnt = drsm.RangeCounts(rb, sb, (0.0, 1.0), (0.0, 1.0), k, lo, hi)
        lam = float([0.0, 4.0, 16.0][trial % 3])
        _, _, recs = drsm.fit(cnt, off, jump, m, r, lam)
        ks = dsm.knots_of(0, blocks, m)
        ns = np.diff(ks)
        tables = [dsm.line_table(cnt, off, ks[q], ns[q], q == len(ns) - 1, r) for q in range(len(ns))]
        bends = [dsm.bend_table(off, ks[q - 1], ns[q - 1], ns[q], m, r, lam) for q in range(1, len(ns))]
        assert len(recs) == 1 and recs[0]["fit_total"] == dsm.brute_force_total(tables, bends, r), trial
        done += len(ns) >= 2
    assert done >= 6


def test_no_steps_or_no_radius_return_the_path():
    """What holds whatever the data: at max_step = 0 every segment is flat, so without a radius the only line between
    its knots is the path itself, for any M; at R = 0 every knot sits on the path, and with M = 1 every block is a knot.
    (With a radius a free polyline may leave even a flat path, and with M > 1 a digital line between two knots on the
    path need not repeat the staircase between them.)"""
    flat = 0
    for i, pr in enumerate(SMALL):
        (off, _, jump, _), smooth, _, _ = model(i)
        cnt = drsm.RangeCounts(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"])
        if pr["s"] == 0:
            assert np.array_equal(drsm.fit(cnt, off, jump, pr["m"], 0, pr["lam"])[0], off), i
            flat += 1
        if i % 4 == 0:
            for m in (1, 3):
                sm_, knot, _ = drsm.fit(cnt, off, jump, m, 0, 8.0)
                ks = np.flatnonzero(knot)
                assert np.array_equal(sm_[ks], off[ks]), i
                if m == 1:
                    assert np.array_equal(sm_, off) and knot.all(), i
    assert flat >= 4


def test_a_one_lag_range_keeps_every_knot_and_no_fit_leaves_its_range():
    one_lag = 0
    for i, pr in enumerate(SMALL):
        (off, _, _, _), smooth, knot, recs = model(i)
        assert smooth.min() >= pr["lo"] and smooth.max() <= pr["hi"], i
        assert np.isfinite(recs["fit_total"]).all(), i
        if pr["hi"] == pr["lo"]:
            assert (smooth == pr["lo"]).all() and np.array_equal(smooth, off)
            one_lag += 1
    assert one_lag >= 1


def test_every_lag_a_line_visits_lies_in_its_intervals_band():
    """The bound of csrc/ffs_drift_range_smooth.h: each block's lags stay inside [min(o_k, o_{k+n}) - R,
    max(o_k, o_{k+n}) + R] of its interval, and that band has at most max_step * ceil(3M / 2) + 2R + 1 lags."""
    c = coverage()
    assert c["widest_step"] >= 1, c
    widest = 0
    for i, pr in enumerate(SMALL):
        (off, _, jump, _), _, _, _ = model(i)
        cnt = drsm.RangeCounts(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["k"], pr["lo"], pr["hi"])
        cnt.visited = []
        drsm.fit(cnt, off, jump, pr["m"], pr["r"], pr["lam"])
        band = {}
        for k0, n, last in drsm.intervals_of(jump, pr["m"]):
            lo, width = drsm.band_of(off, k0, n, pr["r"])
            assert width <= drsm.band_row(pr["s"], pr["m"], pr["r"]), (i, k0, n)
            assert n < (3 * pr["m"] + 1) // 2 or n == 1, (i, k0, n)  # no interval reaches ceil(3M / 2) blocks
            widest = max(widest, width)
            for b in range(k0, k0 + n + (1 if last else 0)):
                band[b] = (lo, lo + width - 1)
        for b, lags in cnt.visited:
            assert lags.min() >= band[b][0] and lags.max() <= band[b][1], (i, b)
    assert widest >= 7 * 13 + 33  # the 14-block ramp at max_step 7
    assert drsm.band_row(2, 16, 16) == 81 and drsm.band_row(7, 256, 16) == 2721


def test_the_set_holds_what_the_fit_has_to_get_right():
    c = coverage()
    assert c["one_block"] >= 1 and c["two_block"] >= 1 and c["last_shorter"] >= 1 and c["last_longer"] >= 1, c
    assert c["most_intervals"] > 64 and c["most_segments"] > 4 and c["widest_step"] >= 1 and c["knot_outside"] >= 1, c
    assert c["moved"] >= 20, c
    lens = {pr["hi"] - pr["lo"] + 1 for pr in SMALL}
    assert {1, 5, 63, 65, 2049} <= lens
    assert {pr["s"] for pr in SMALL} == set(range(8)) and {pr["q"] for pr in SMALL} == {0.0, 1.0, 16.0, 128.0}
    assert {pr["m"] for pr in SMALL} == {1, 2, 3, 8, 16, 256} and {pr["r"] for pr in SMALL} == {0, 1, 5, 16}
    assert {pr["lam"] for pr in SMALL} == {0.0, 1.0, 64.0, 1e6} and {pr["p"] for pr in SMALL} == {0.0, 60.0, np.inf}
    assert any(pr["lo"] > 0 for pr in SMALL) and any(pr["lo"] == -pr["hi"] + 1 for pr in SMALL)
    assert any(pr["lo"] >= pr["rb"].size or pr["hi"] <= -pr["sb"].size for pr in SMALL)  # no overlap at all
    assert any(pr["lo"] < -pr["sb"].size and pr["hi"] > pr["rb"].size for pr in SMALL)  # past both overlap edges


def test_argument_validation_of_the_python_layer():
    from ffsubsync_amd import drift_range_smooth as drs

    bad_kw = (dict(knot_blocks=0), dict(knot_blocks=257), dict(radius=17), dict(radius=-1), dict(bend_cost=-1.0),
              dict(bend_cost=float("nan")), dict(bend_cost=float("inf")), dict(max_step=8), dict(step_cost=-1.0),
              dict(block_samples=100), dict(split_penalty=-1.0))
    for kw in bad_kw:  # before any native call: no batch, no GPU needed to be refused
        with pytest.raises(ValueError):
            drs.smooth_align_range_batch(None, None, **kw)
        with pytest.raises(ValueError):
            drs.smooth_cut_sync([], **kw)
    with pytest.raises(ValueError):
        drs.smooth_cut_sync([], lag_range=(5, 4))
    assert issubclass(drs.SmoothCutSyncResult, drs.CutDriftSyncResult)
    from ffsubsync_amd import _native

    assert _native.range_band_row(2, 16, 16) == drsm.band_row(2, 16, 16) == 81
    assert _native.range_band_row(7, 256, 16) == drsm.band_row(7, 256, 16)


def test_the_new_symbol_is_declared_and_exported():
    from ffsubsync_amd import _native

    name = "ffs_align_drift_range_smooth_batch"
    text = open(os.path.join(ROOT, "include", "ffsubsync_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert name in _native.EXPORTED_SYMBOLS
    lib = ctypes.CDLL(_native.library_path())
    assert getattr(lib, name) is not None
    assert _native.load().ffs_version() >= 390
    assert hasattr(_native.DriftRangePlan, "smooth")
