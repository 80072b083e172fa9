"""Jump refinement of a drift path on the host (no GPU): the numpy model tests/drift_refine_model.py against a
brute-force search over every (t1, t2) and against direct counting along the path, its identity with
split_refine_model on piecewise-constant offsets, the refined cue mappings, and the C prototype against the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import drift_refine_model as drm
import split_refine_model as rm
import test_gpu_drift_refine as t_gpu  # its seeded problems are built on the host
from ffsubsync_amd import _native, drift_align, drift_refine, drift_smooth
from ffsubsync_amd.drift_smooth import SmoothResult, SmoothSegment
from ffsubsync_amd.split_refine import UNMATCHED_PIECE, RefinedBreak

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 256
LEVELS = [((0.3, 0.8), (-0.5, 1.25)), ((-1.0, 2.5), (0.0, 24.0 / 25.0)), ((0.25, 1.5), (0.125, 25.0 / 24.0))]


def _path(rng, n_b, jumps, base, spread):
    """Block offsets that move by -2 .. 2 per block inside a segment and jump at ``jumps``."""
    o = np.zeros(n_b, np.int64)
    o[0] = base
    for b in range(1, n_b):
        o[b] = o[b - 1] + (int(rng.randint(-spread, spread + 1)) if b in jumps else int(rng.randint(-2, 3)))
    jf = np.zeros(n_b, np.uint8)
    jf[list(jumps)] = 1
    return o, jf


def _problem(seed):
    """A tiny pair whose subtitle follows a drifting path with one or two jumps; every third seed sends part of a
    window's partners off an end of the reference, every seventh has lags with no overlap at all."""
    rng = np.random.RandomState(7000 + seed)
    S = int(rng.randint(3 * K + 1, 5 * K))
    R = S + int(rng.randint(-150, 200))
    n_b = -(-S // K)
    jumps = sorted(rng.choice(np.arange(1, n_b), size=int(rng.randint(1, 3)), replace=False).tolist())
    base = [int(rng.randint(-20, 21)), -jumps[0] * K + 25, R - jumps[0] * K - 30][seed % 3]
    if seed % 7 == 6:
        base = [R + 40, -S - R - 9][seed % 2]
    o, jf = _path(rng, n_b, jumps, base, 40)
    rb = rng.rand(R) < 0.45
    idx = np.arange(S) + np.repeat(o, K)[:S] + rng.randint(-25, 26)  # the true change is off the block grid
    sb = rng.rand(S) < 0.3
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.1
    r_lv, s_lv = LEVELS[seed % 3]
    return rb, sb, r_lv, s_lv, o, jf


N_TINY = 140  # seeds of one or two jumps each: more than 200 distinct windows


@pytest.mark.parametrize("beta", [None, 0.0, 0.25, 1.0])
def test_model_equals_brute_force_on_tiny_windows(beta):
    """At least 200 distinct seeded windows, every one at each of the four margins: K = 256, windows of at most 120
    samples, steps of -2 .. 2 per block, levels that are not 0/1."""
    windows, unmatched, off_low, off_high, no_overlap = set(), 0, 0, 0, 0
    for seed in range(N_TINY):
        rb, sb, r_lv, s_lv, o, jf = _problem(seed)
        recs = drm.refine(rb, sb, r_lv, s_lv, o, jf, K, int(np.random.RandomState(seed).randint(8, 61)), beta)
        assert list(recs["block"]) == drm.jumps_of(jf)
        for rec in recs:
            lo, hi, f = int(rec["lo"]), int(rec["hi"]), int(rec["block"])
            assert hi - lo <= 120
            t1, t2, v = drm.brute(rb, sb, r_lv, s_lv, lo, hi, o, K, f, beta)
            assert (int(rec["t1"]), int(rec["t2"])) == (t1, t2), (seed, rec, t1, t2)
            assert np.float64(rec["refined_score"]).tobytes() == np.float64(v).tobytes()
            assert (rec["offset_prev"], rec["offset_next"]) == (o[f - 1], o[f])
            la, lb = drm.sample_lags(o, K, f, lo, hi)
            x = np.arange(lo, hi)
            off_low += int(((x + la < 0) | (x + lb < 0)).any() and ((x + la >= 0) | (x + lb >= 0)).any())
            off_high += int(((x + la >= rb.size) | (x + lb >= rb.size)).any() and (x + la < rb.size).any())
            no_overlap += int(((x + la < 0) | (x + la >= rb.size)).all())
            unmatched += int(rec["t1"] < rec["t2"])
            windows.add((seed, f))
            if beta is None:
                assert rec["t1"] == rec["t2"] and not rec["flags"] & drm.UNMATCHED
    assert len(windows) >= 200, len(windows)  # distinct (pair, jump) windows, each searched at this margin
    assert off_low >= 3 and off_high >= 3 and no_overlap >= 3, (off_low, off_high, no_overlap)
    if beta:
        assert unmatched >= 1


def test_curves_count_every_sample_at_its_own_blocks_lag():
    """Windows that span several blocks on each side: A, B at every t equal direct counts with the lag looked up per
    sample (the tiny windows above never leave the two blocks next to the cut)."""
    for seed in range(4):
        rng = np.random.RandomState(90 + seed)
        S, R = 9 * K + 57, 9 * K - 100
        base, far = int(rng.randint(-30, 31)), int(rng.randint(-300, 301))
        o = np.array([base + d for d in (0, 1, 3, 2, 4)] + [far + d for d in (0, -2, -1, 1, 2)], np.int64)
        rb, sb = rng.rand(R) < 0.5, rng.rand(S) < 0.4
        r_lv, s_lv = LEVELS[seed % 3]
        lo, hi = 5 * K - 700, 5 * K + 650
        A, B, _ = drm.curves(rb, sb, r_lv, s_lv, lo, hi, o, K, 5, 0.25)
        c = drm.constants(rb, r_lv, s_lv, 0.25)[0]
        x = np.arange(lo, hi)
        for second, curve in ((False, A), (True, B)):
            lag = np.array([o[max(b, 5)] if second else o[min(b, 4)] for b in x // K])
            assert len(set(lag.tolist())) == 3  # the side's own blocks differ
            pres = (x + lag >= 0) & (x + lag < R)
            rv = np.zeros(x.size, bool)
            rv[pres] = rb[(x + lag)[pres]]
            for t in range(0, hi - lo + 1, 37):
                sl = slice(t, None) if second else slice(0, t)
                want = drm._mix(c, pres[sl].sum(), (sb[lo:hi][sl] & rv[sl]).sum(), (sb[lo:hi][sl] & pres[sl]).sum(),
                                rv[sl].sum())
                assert np.float64(curve[t]).tobytes() == np.float64(want).tobytes()


@pytest.mark.parametrize("beta", [None, 0.25])
def test_model_is_split_refine_on_piecewise_constant_offsets(beta):
    for seed in range(12):
        rng = np.random.RandomState(500 + seed)
        S = int(rng.randint(6 * K, 12 * K))
        R = S + int(rng.randint(-300, 300))
        n_b = -(-S // K)
        o = np.repeat(rng.randint(-400, 400, n_b), rng.randint(1, 4, n_b))[:n_b].astype(np.int64)
        jf = np.concatenate([[0], o[1:] != o[:-1]]).astype(np.uint8)
        jf[0] = seed % 2  # ignored
        rb, sb = rng.rand(R) < 0.5, rng.rand(S) < 0.4
        r_lv, s_lv = LEVELS[seed % 3]
        for radius in (40, 300, 5000):
            want = rm.refine(rb, sb, r_lv, s_lv, o, K, radius, beta)
            got = drm.refine(rb, sb, r_lv, s_lv, o, jf, K, radius, beta)
            assert len(want) >= 1 and want.tobytes() == got.tobytes()


def test_a_jump_with_equal_offsets_on_both_sides_is_still_a_jump():
    rng = np.random.RandomState(3)
    rb, sb = rng.rand(2000) < 0.5, rng.rand(6 * K) < 0.5
    o = np.array([5, 6, 7, 7, 8, 9], np.int64)
    jf = np.array([1, 0, 0, 1, 0, 0], np.uint8)
    recs = drm.refine(rb, sb, (0.0, 1.0), (0.0, 1.0), o, jf, K, 100, 0.25)
    assert drm.jumps_of(jf) == [3] and len(recs) == 1
    assert (recs[0]["block"], recs[0]["cut"], recs[0]["offset_prev"], recs[0]["offset_next"]) == (3, 768, 7, 7)
    assert (recs[0]["lo"], recs[0]["hi"]) == (668, 868)
    assert len(rm.refine(rb, sb, (0.0, 1.0), (0.0, 1.0), np.array([7] * 6), K, 100, 0.25)) == 0
    assert len(drm.refine(rb, sb, (0.0, 1.0), (0.0, 1.0), o, np.zeros(6, np.uint8), K, 100, 0.25)) == 0  # offsets move, no jump


def test_fuzz_set_covers_what_it_claims():
    """The cases the device test relies on are in the seeded set: the first and the last block, adjacent blocks (a
    window of half a block on one side), no jump, every block, partners off either end, lags beyond the reference, S on
    and off the block and word grids."""
    lens = np.array([pr["sb"].size for pr in t_gpu.FUZZ])
    assert (lens % t_gpu.K == 0).any() and (lens % 32 != 0).sum() >= 40
    assert all(pr["rb"].size != pr["sb"].size for pr in t_gpu.FUZZ)
    for kind in range(8):
        assert sum(pr["kind"] == kind for pr in t_gpu.FUZZ) == 8
    low = high = 0
    for pr in t_gpu.FUZZ:
        j, n_b, R = drm.jumps_of(pr["jf"]), pr["o"].size, pr["rb"].size
        assert len(set(np.diff(pr["o"].astype(np.int64))[[b - 1 for b in range(1, n_b) if b not in j]].tolist())
                   - {-2, -1, 0, 1, 2}) == 0
        if pr["kind"] == 0:
            assert j[0] == 1 and j[-1] == n_b - 1
        if pr["kind"] == 1:
            assert any(b - a == 1 for a, b in zip(j[:-1], j[1:]))
            w = drm.windows([b * t_gpu.K for b in j], pr["sb"].size, 5000)
            half = t_gpu.K // 2
            assert any(c - lo == half or hi - c == half for (lo, hi, _), c in zip(w, [b * t_gpu.K for b in j]))
        if pr["kind"] == 2:
            assert not j
        if pr["kind"] == 3:
            assert j == list(range(1, n_b))
        if pr["kind"] in (4, 5) and pr["radius"] >= 100:
            rec = t_gpu._model(pr)[0]
            x = np.arange(int(rec["lo"]), int(rec["hi"]))
            la, _ = drm.sample_lags(pr["o"], t_gpu.K, int(rec["block"]), int(rec["lo"]), int(rec["hi"]))
            low += int((x + la < 0).any() and (x + la >= 0).any())
            high += int((x + la >= R).any() and (x + la < R).any())
        if pr["kind"] == 6:
            assert np.abs(pr["o"].astype(np.int64)).min() > R
    assert low >= 3 and high >= 3, (low, high)


def _drift_result(o, jf, sub_len, k=K):
    o, jf = np.asarray(o, np.int32), np.asarray(jf, np.uint8)
    sc = np.zeros(o.size)
    return drift_align.DriftResult(drift_align.segments_from_blocks(o, sc, jf, k, sub_len), 0.0, o, sc, jf)


def _smooth_result(drift, k=K):
    """A SmoothResult over ``drift`` with knots at each segment's first and last block (its own offsets there)."""
    segs, knot = [], np.zeros(drift.block_offsets.size, np.uint8)
    for s in drift.segments:
        blocks = sorted({s.first_block, s.end_block - 1})
        knot[blocks] = 1
        segs.append(SmoothSegment(s.first_block, s.end_block, [(b, int(drift.block_offsets[b])) for b in blocks], 0.0,
                                  0.0, 0.0, []))
    return SmoothResult(drift, drift.block_offsets.copy(), knot, segs)


def _brk(t1, t2):
    return RefinedBreak(0, t1, 0, 0, t1, t2, 0, 0, 0.0, 0.0, 0)


def _cues(seed, sub_len):
    rng = np.random.RandomState(seed)
    s_us = np.sort(rng.randint(-30000, (sub_len + 300) * 10000, 300)).astype(np.int64)
    return s_us, s_us + rng.randint(1, 500000, 300)


O12 = [10, 11, 13, 13, 400, 402, 401, 401, 399, -80, -80, -82]
J12 = [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]


def test_map_cues_drift_refined_at_the_coarse_cuts_is_map_cues_drift():
    S = 12 * K - 40
    res = _drift_result(O12, J12, S)
    s_us, e_us = _cues(1, S)
    cuts = [_brk(4 * K, 4 * K), _brk(9 * K, 9 * K)]
    for ratio in (1.0, 24.0 / 25.0, 25.0 / 24.0):
        want = drift_align.map_cues_drift(s_us, e_us, ratio, res, K)
        got = drift_refine.map_cues_drift_refined(s_us, e_us, ratio, res, cuts, K)
        for a, b in zip(want, got[:3]):
            assert np.array_equal(a, b)
        assert not got[3].any()


def test_map_cues_smooth_refined_at_the_coarse_cuts_is_map_cues_smooth():
    S = 12 * K - 40
    res = _smooth_result(_drift_result(O12, J12, S))
    s_us, e_us = _cues(2, S)
    cuts = [_brk(4 * K, 4 * K), _brk(9 * K, 9 * K)]
    for ratio in (1.0, 24.0 / 25.0, 25.0 / 24.0):
        want = drift_smooth.map_cues_smooth(s_us, e_us, ratio, res, K)
        got = drift_refine.map_cues_smooth_refined(s_us, e_us, ratio, res, cuts, K)
        for a, b in zip(want, got[:3]):
            assert np.array_equal(a, b)
        assert not got[3].any()


def test_a_cue_between_t1_and_t2_is_unmatched_with_the_earlier_segments_shift():
    S = 12 * K - 40
    res = _drift_result(O12, J12, S)
    # jump 1 refined EARLIER than its block cut (t2 = 1000 < 1024), jump 2 LATER with an unmatched stretch [2350, 2400)
    breaks = [_brk(1000, 1000), _brk(2350, 2400)]
    starts = np.array([0, 999, 1000, 1023, 1024, 2303, 2304, 2349, 2350, 2399, 2400, 3000], np.int64)
    s_us, e_us = starts * 10000, starts * 10000 + 5000
    cs, ce, which, um = drift_refine.map_cues_drift_refined(s_us, e_us, 1.0, res, breaks, K)
    assert list(which) == [0, 0, 1, 1, 1, 1, 1, 1, UNMATCHED_PIECE, UNMATCHED_PIECE, 2, 2]
    assert list(um) == [False] * 8 + [True, True, False, False]
    # the lag of block clamp(x // K, first, end - 1) of the cue's segment: samples 1000 .. 1023 lie in block 3 and take
    # segment 1's first block (4); samples 2304 .. 2399 lie in block 9 and stay with segment 1's last block (8)
    want = np.array([10, 13, 400, 400, 400, 399, 399, 399, 399, 399, -80, -82]) * 10000
    assert np.array_equal(cs, s_us + want) and np.array_equal(ce, e_us + want)
    sm = _smooth_result(res)
    cs2, ce2, which2, um2 = drift_refine.map_cues_smooth_refined(s_us, e_us, 1.0, sm, breaks, K)
    assert list(which2) == list(which) and list(um2) == list(um)
    for i in (8, 9):  # unmatched: the earlier segment's polyline, continued
        shift = int(round(drift_smooth.polyline_shift(sm.segments[1], float(starts[i]), K) * 1e4))
        assert cs2[i] == s_us[i] + shift and ce2[i] == e_us[i] + shift


def test_refined_mappings_check_their_arguments():
    res = _drift_result(O12, J12, 12 * K)
    with pytest.raises(ValueError):
        drift_refine.map_cues_drift_refined([0], [1], 1.0, res, [_brk(5, 5)], K)
    with pytest.raises(ValueError):
        drift_refine.map_cues_smooth_refined([0], [1], 1.0, _smooth_result(res), [], K)


C_TYPES = {"ffs_split_plan*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_header_prototype_and_record_size_match_the_binding():
    text = open(os.path.join(ROOT, "include", "ffsubsync_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+ffs_drift_refine_batch\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m, "ffs_drift_refine_batch is not declared"
    want = []
    for arg in m.group(1).split(","):
        typ = re.sub(r"\s+", " ", arg.strip()).rsplit(" ", 1)[0].replace(" *", "*")
        want.append(C_TYPES.get(typ, ctypes.c_void_p if typ.endswith("*") else None))
    assert None not in want and len(want) == 18
    lib = _native.load()
    assert lib.ffs_drift_refine_batch.restype is ctypes.c_int
    assert list(lib.ffs_drift_refine_batch.argtypes) == want
    # the split call's prototype with block_jump_dev after block_offset_dev
    split = list(lib.ffs_split_refine_batch.argtypes)
    assert want[:12] + want[13:] == split
    assert "ffs_drift_refine_batch" in _native.EXPORTED_SYMBOLS
    size = re.search(r"sizeof\(ffs_break_refine\) == (\d+)", text)
    assert int(size.group(1)) == _native.BREAK_REFINE_BYTES == _native.BREAK_REFINE_DTYPE.itemsize == 88
    assert "sample-exact jumps of a drift solve" in text
