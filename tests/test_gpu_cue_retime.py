"""The joint cue retiming on the device (csrc/ffs_cue_retime.h via ffsubsync_amd.cue_retime): every record and summary
byte-identical to the numpy model tests/retime_model.py -- edge shapes, every option, chain lengths across the 64-lane
and sub-batch seams, the gaps at the windowed maximum's seams, ties, sub-batches (by pair count and by the workspace cap),
hostile layouts, the refusals of the C ABI, the tiny cases against the enumeration of every path, and retime_sync end to
end."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import layout_cases as lc  # noqa: E402
import retime_model as rm  # noqa: E402
import retime_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

LEVELS = [((0.0, 1.0), (0.0, 1.0)), ((0.25, 1.0), (0.0, 1.0 / 1.001)), ((-1.0, 2.5), (-0.5, 1.25))]
PENALTIES = (0, 1, 64, 1 << 20)
JUMPS = (-1, 0, 300, 1 << 40)


def speechy(rng, n, mean_run=40):
    seg = np.maximum(1, rng.geometric(1.0 / mean_run, size=n // 2 + 2))
    vals = (np.arange(seg.size) + rng.randint(2)) % 2
    return np.repeat(vals, seg)[:n].astype(np.uint8)


def _pair(rb, sb, levels=LEVELS[0]):
    (r0, r1), (s0, s1) = levels
    return dict(rb=np.asarray(rb, np.uint8), sb=np.asarray(sb, np.uint8), r_lv=(r0, r1), s_lv=(s0, s1))


def _device_batch(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    import torch

    def raster(bits, lv):
        packed = np.packbits(bits, bitorder="little")
        host = np.zeros((bits.size + 31) // 32 * 4, np.uint8)
        host[:packed.size] = packed
        return DeviceRaster(torch.from_numpy(host).cuda().view(torch.int32), lv[0], lv[1], bits.size)

    return batch.pack_pairs([(raster(p["rb"], p["r_lv"]), [raster(p["sb"], p["s_lv"])]) for p in problems])


def _model(problems, cues, radius, context, penalty_q, jump_q, keep_order):
    """(records of the flat table, summaries): the plain maximisation at small radii, its pinned fast evaluation
    (tests/test_retime_model_host.py) at the others.  The levels do not enter."""
    fn = rm.retime if radius <= 8 else rm.retime_fast
    out = [fn(p["rb"], p["sb"], c, radius, context, penalty_q, jump_q, keep_order) for p, c in zip(problems, cues)]
    return (np.concatenate([o[0] for o in out] + [np.zeros(0, rm.DTYPE)]),
            np.array([o[1] for o in out], dtype=rm.SUMMARY).reshape(-1))


def _assert_same(got, want, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize
    if got.tobytes() != want.tobytes():
        bad = [(k, f, got[k][f], want[k][f]) for k in range(min(len(got), len(want))) for f in want.dtype.names
               if np.asarray(got[k][f]).tobytes() != np.asarray(want[k][f]).tobytes()]
        raise AssertionError("%s: %d / %d records, first differences %r" % (what, len(got), len(want), bad[:6]))


def _check(db, problems, cues, radius, context, penalty_q, jump_q, keep_order, what=""):
    from ffsubsync_amd import cue_retime as ct

    got, slices, sums = ct.retime_batch(db, cues, radius, context, penalty_q, jump_q, keep_order, raw=True)
    want, want_sums = _model(problems, cues, radius, context, penalty_q, jump_q, keep_order)
    tag = "%s rho %d m %d q %d jump %d order %d" % (what, radius, context, penalty_q, jump_q, keep_order)
    _assert_same(got, want, tag)
    _assert_same(sums, want_sums, tag + " (summaries)")
    live = (got["flags"] & 3) == 0
    for sl, sm in zip(slices, sums):  # the invariants
        lv = got[sl][live[sl]]
        assert sm["own_total"] <= sm["total"] <= sm["best_total"]
        assert sm["total"] == 64 * int(lv["at"].astype(np.int64).sum()) - int(lv["link"].sum())
    return got, slices, sums


def _edge_cues(R, S, rng):
    """Cues at every edge of the contract: hostile rows between ordinary ones, partly sorted, with duplicates."""
    w = min(S, 32)
    rows = [
        (0, min(S, 9), 0), (max(S - 7, 0), S, 3), (-10, S + 10, -2), (min(20, S), min(5, S - 1), 1),  # end < start
        (S // 2, S // 2 + 1, 0), (S // 2, S // 2, 0), (w // 4, w // 2, 4), (max(w - 3, 0), w + 5, -1),
        (S // 3, S // 3 + 70, 5), (S // 3, S // 3 + 70, 5), (0, S, 0),  # duplicates; the whole vector
        (S // 4, S // 2, -S - R - 5), (S // 4, S // 2, R + 10),  # wholly before / behind the reference
        (S // 4, S // 2 + 1, R - S // 2), (0, S // 2 + 1, -S // 4 - 1), (S // 5, S // 2, R - S // 5 - 1),  # partly outside
        (3, 30, 2 ** 31 + 1), (3, 30, -2 ** 31 - 1), (3, 30, 2 ** 31), (3, 30, -2 ** 31), (5, 1, 2 ** 40),
        (-2 ** 62, 2 ** 62, 7), (2 ** 62, -2 ** 62, 7), (np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0),
    ]
    start = np.sort(rng.randint(-5, S + 5, 24))
    for a in start:  # an ordinary file: sorted starts, small lags, some overlap
        rows.append((int(a), int(a) + int(rng.randint(0, 90)), int(rng.randint(-4, 5))))
    order = np.concatenate([rng.permutation(12), np.arange(12, len(rows))])  # half of the hostile rows shuffled in front
    rows = [rows[i] for i in order]
    return tuple(np.array([r[k] for r in rows], dtype=np.int64) for k in range(3))


def _edge_problems():
    rng = np.random.RandomState(2424)
    sizes = [(31, 29), (33, 64), (1000, 777), (97, 2500), (3001, 2047)]
    probs = [_pair(speechy(rng, R), speechy(rng, S), LEVELS[i % len(LEVELS)]) for i, (R, S) in enumerate(sizes)]
    cues = [_edge_cues(R, S, rng) for R, S in sizes]
    empty = tuple(np.zeros(0, np.int64) for _ in range(3))
    probs.insert(2, _pair(speechy(rng, 500), speechy(rng, 300)))  # a pair with zero cues between pairs with many
    cues.insert(2, empty)
    probs.append(_pair(speechy(rng, 200), speechy(rng, 150)))  # a pair with only skipped cues
    cues.append((np.array([5, 9, 200, 3], np.int64), np.array([5, 2, 300, 30], np.int64), np.array([0, 1, 2, 2 ** 33], np.int64)))
    return probs, cues


EDGE = _edge_problems()
_batches = {}


def _edge_batch():
    if "edge" not in _batches:
        _batches["edge"] = _device_batch(EDGE[0])
    return _batches["edge"]


@pytest.mark.parametrize("context", [0, 1, 65536])
@pytest.mark.parametrize("radius", [0, 1, 31, 32, 33, 64, 1024])
def test_edge_shapes_equal_the_model(radius, context):
    probs, cues = EDGE
    n = [0, 1, 31, 32, 33, 64, 1024].index(radius) * 3 + [0, 1, 65536].index(context)
    pq, jq, keep = PENALTIES[n % 4], JUMPS[(n // 4 + n) % 4], n % 3 != 2
    got, slices, sums = _check(_edge_batch(), probs, cues, radius, context, pq, jq, keep)
    assert [s.stop - s.start for s in slices] == [c[0].size for c in cues] and slices[2].start == slices[2].stop
    assert not sums[2].tobytes().strip(b"\0") and not sums[6].tobytes().strip(b"\0")  # no live cue: all zeros
    assert (got["flags"] & rm.EMPTY).any() and (got["flags"] & rm.INVALID).any()
    assert ((got["flags"] & 3) == 0).sum() >= 100 and sums["n_live"].sum() == ((got["flags"] & 3) == 0).sum()


@pytest.mark.parametrize("jump_q", JUMPS)
@pytest.mark.parametrize("keep_order", [True, False])
def test_every_option(keep_order, jump_q):
    probs, cues = EDGE
    seen = 0
    for pq in PENALTIES:
        got, _, sums = _check(_edge_batch(), probs, cues, 33, 9, pq, jump_q, keep_order)
        seen |= int(np.bitwise_or.reduce(got["flags"]))
        assert bool(got["flags"].__and__(rm.UNORDERED).any()) == keep_order
        assert (sums["n_jumps"].sum() > 0) <= (jump_q >= 0)
    assert seen & rm.MOVED and seen & rm.AT_EDGE


def _file_cues(rng, S, K, spread=30):
    """K cues of a file in order: sorted starts, some overlapping, small lags."""
    start = np.sort(rng.randint(0, S - 40, K))
    return start.astype(np.int64), (start + rng.randint(5, spread, K)).astype(np.int64), rng.randint(-3, 4, K).astype(np.int64)


def test_chain_lengths_across_the_lane_and_wave_seams():
    rng = np.random.RandomState(99)
    counts = [1, 2, 63, 64, 65, 300, 17]
    probs = [_pair(speechy(rng, 1500, 12), speechy(rng, 1400, 12)) for _ in counts]
    cues = [_file_cues(rng, 1400, K) for K in counts]
    db = _device_batch(probs)
    got, slices, sums = _check(db, probs, cues, 40, 20, 16, 2000, True)
    assert sums["n_live"].tolist() == counts and sums["n_moved"].sum() > 0
    _check(db, probs, cues, 40, 20, 3, -1, False)


def test_gaps_at_the_windowed_maximum_seams():
    """One chain whose gap g takes 0, 1, powers of two and their neighbours, >= 2 rho and < 0: rho = 20, so the window
    (d, d + g] is a doubling level with two overlapping reads below 40 and the whole suffix from 40 on."""
    rng = np.random.RandomState(5)
    gaps = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 39, 40, 41, 100, -5, 1, 0, -60, 2, 64, 0, 0, 1, 19, 20, 21]
    r, s = speechy(rng, 1300, 6), speechy(rng, 1200, 6)
    start = 300 + np.concatenate([[0], np.cumsum(gaps)]).astype(np.int64)
    lag = np.zeros(start.size, np.int64)
    lag[5], start[5] = 3, start[5] - 3  # the gap is of start + lag
    cues = [(start, start + 25, lag)]
    probs = [_pair(r, s)]
    db = _device_batch(probs)
    tight = 0
    for pq, jq in ((0, -1), (1, -1), (7, 200), (64, 0), (64, 640), (1000, 1 << 40)):
        for context in (0, 30):
            got, _, _ = _check(db, probs, cues, 20, context, pq, jq, True)
            tight += int(((got["flags"] & rm.ORDER_TIGHT) != 0).sum())
            _check(db, probs, cues, 20, context, pq, jq, False)
    assert tight > 0  # the order constraint binds somewhere
    _check(db, probs, cues, 600, 10, 2, 900, True, "wide")  # every gap below 2 rho


LONG_N = 70000
# (start, end, lag): windows at context 0 of exactly 256 words from a word boundary, 257 words off one, 512 words from a
# boundary, a short cue, 513 words off a boundary (three slices), 907 words (four slices) and a cue whose partners run
# past the end of the reference; at context 65536 every window is the whole vector (2188 words, nine slices)
LONG_CUES = ((3200, 3200 + 8192, 30), (12005, 12005 + 8192, 45), (20480, 20480 + 16384, 5), (36900, 36950, -3),
             (37001, 37001 + 16384, -20), (40000, 69000, -45), (60000, 69990, 900))


def _long_problem():
    """One pair of 70 000 samples: the subtitle follows the reference at +37 up to sample 36 000 and at -25 behind it,
    5 % of its samples flipped."""
    if "long" not in _batches:
        rng = np.random.RandomState(313)
        r = speechy(rng, LONG_N, 150)
        i = np.arange(LONG_N)
        src = np.clip(i + np.where(i < 36000, 37, -25), 0, LONG_N - 1)
        s = r[src] ^ (rng.rand(LONG_N) < 0.05).astype(np.uint8)
        probs = [_pair(r, s, LEVELS[1])]
        cues = [tuple(np.array([c[k] for c in LONG_CUES], np.int64) for k in range(3))]
        _batches["long"] = (probs, cues, _device_batch(probs))
    return _batches["long"]


def _window_words(cue, context, S=LONG_N):
    lo, hi = max(cue[0] - context, 0), min(cue[1] + context, S)
    return lo >> 5, (hi + 31) >> 5


def test_the_long_cues_span_the_slice_seams():
    """(host data only) The shapes test_long_windows_are_staged_slice_by_slice relies on: CUE_SLICE = 256 window words."""
    words = [b - a for a, b in (_window_words(c, 0) for c in LONG_CUES)]
    assert words == [256, 257, 512, 2, 513, 907, 313]
    assert [c[0] % 32 == 0 for c in LONG_CUES[:5]] == [True, False, True, False, False]
    assert any(c[1] - c[0] > 3 * 8192 for c in LONG_CUES)  # a window of more than 3 x 8192 samples at any context
    assert all(_window_words(c, 65536) == (0, (LONG_N + 31) >> 5) for c in LONG_CUES)
    assert {np.sign(c[2]) for c in LONG_CUES} == {-1, 1} and LONG_CUES[6][1] + LONG_CUES[6][2] > LONG_N


@pytest.mark.parametrize("keep_order", [True, False])
@pytest.mark.parametrize("context", [0, 8192, 65536])
@pytest.mark.parametrize("radius", [33, 100, 1024])
def test_long_windows_are_staged_slice_by_slice(radius, context, keep_order):
    """k_retime_profile stages the reference 256 window words at a time: windows of exactly one slice, one word more, two
    slices, one word more, four and nine slices, from and off a word boundary, a short cue between them, lags of both
    signs and partners past the end of the reference -- the second and later iterations of the slice loop (the barrier
    between slices, the carried bit offset, the clamps far from word 0, the first staged word) under the byte-exact
    check against retime_model.retime_fast."""
    probs, cues, db = _long_problem()
    got, _, sums = _check(db, probs, cues, radius, context, 16, 2000 if keep_order else -1, keep_order, "long windows")
    assert max(int(e - s) for s, e in zip(got["start"], got["end"])) > 3 * 8192
    assert sums["n_live"].tolist() == sums["n_moved"].tolist() == [len(LONG_CUES)]  # every cue live and moved


def test_constant_profiles_and_ties():
    from ffsubsync_amd import cue_retime as ct

    rng = np.random.RandomState(77)
    s = speechy(rng, 900)
    ones = _pair(np.ones(1100, np.uint8), s, LEVELS[1])  # every shift scores the same: every choice is a tie
    ts = np.zeros(400, np.uint8)
    ts[200:210] = 1
    tr = np.zeros(400, np.uint8)
    tr[160:170] = 1
    tr[240:250] = 1  # runs at -40 and +40 of the cue, symmetric about it
    tie = _pair(tr, ts, LEVELS[2])
    probs = [ones, tie]
    inner = _file_cues(rng, 390, 40)  # every window and every partner inside both vectors: no edge enters the profile
    cues = [(inner[0] + 250, inner[1] + 250, inner[2]), (np.array([200, 200, 200]), np.array([210, 210, 210]), np.array([0, 0, 0]))]
    db = _device_batch(probs)
    for pq, jq, keep in ((0, -1, True), (0, 0, False), (5, 100, True), (1 << 20, -1, False)):
        got, slices, sums = _check(db, probs, cues, 70, 100, pq, jq, keep)
        assert not got["delta"][slices[0]].any() and not got["best_delta"][slices[0]].any() and sums["n_moved"][0] == 0
        assert got["best_delta"][slices[1]].tolist() == [40, 40, 40]
        assert got["delta"][slices[1]].tolist() == [40, 40, 40]  # + over -, on every cue of the chain
    got, slices, _ = ct.retime_batch(db, cues, 29, 100, 0, -1, raw=True)
    assert not got["delta"][slices[1]].any()  # the runs out of reach: a flat profile, the smallest |delta|


def _raw_call(plan, db, table, first, count, out, summ, radius=33, context=9, penalty_q=16, jump_q=500, flags=1,
              n_cues=None, cue_ptr=None, out_ptr=None, sum_ptr=None, n_pairs=None, arrays=None):
    """ffs_cue_retime_batch through ctypes with every argument open to abuse; returns the code."""
    import torch

    arrays = list(db.pair_arrays()) if arrays is None else arrays
    kinds = (np.uint64, np.int64, np.float64, np.float64) * 2
    bufs = [np.ascontiguousarray(a, dtype=t) for a, t in zip(arrays, kinds)]
    first, count = np.ascontiguousarray(first, np.int64), np.ascontiguousarray(count, np.int64)
    torch.cuda.synchronize()
    return plan.lib.ffs_cue_retime_batch(
        plan.handle, len(bufs[0]) if n_pairs is None else n_pairs, *[b.ctypes.data for b in bufs],
        table.data_ptr() if cue_ptr is None else cue_ptr, table.numel() // 24 if n_cues is None else n_cues,
        first.ctypes.data, count.ctypes.data, radius, context, penalty_q, jump_q, flags,
        out.data_ptr() if out_ptr is None else out_ptr, summ.data_ptr() if sum_ptr is None else sum_ptr,
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_sub_batches_and_repeats_give_identical_bytes():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import cue_report as cr
    from ffsubsync_amd import cue_retime as ct

    probs, cues = EDGE  # 7 pairs
    db = _edge_batch()
    table, first, count = cr.flat_cue_table(cues, len(probs))
    dev = db.data.device
    tdev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
    outs = []
    for pif in (1, 3, len(probs), 16):
        plan = _native.SplitPlan(pif, 1, 2, 1)
        try:
            before = plan.workspace_bytes
            out = torch.full((table.size * 64,), 0xEE, dtype=torch.uint8, device=dev)
            summ = torch.full((len(probs) * 40,), 0xEE, dtype=torch.uint8, device=dev)
            args = (*db.pair_arrays(), tdev, first, count, 33, 9, 16, 500, 1, out, summ)
            plan.cue_retime(*args)
            outs.append(out.cpu().numpy().tobytes() + summ.cpu().numpy().tobytes())
            grown = plan.workspace_bytes
            assert grown == before + _native.RETIME_DESC_BYTES * pif + ct.workspace_bytes(count, 33, pif)
            plan.cue_retime(*args)
            assert out.cpu().numpy().tobytes() + summ.cpu().numpy().tobytes() == outs[-1] and plan.workspace_bytes == grown
            plan.cue_retime(*db.pair_arrays(), tdev, first, count, 5, 9, 16, 500, 1, out, summ)  # a smaller call: no growth
            assert plan.workspace_bytes == grown
        finally:
            plan.close()
    assert outs[0] == outs[1] == outs[2] == outs[3]
    want, want_sums = _model(probs, cues, 33, 9, 16, 500, True)
    assert outs[0] == want.tobytes() + want_sums.tobytes()


def test_the_workspace_cap_cuts_sub_batches():
    """Three pairs of 9000 cues at the largest radius: two fit under the cap together, the third does not."""
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import cue_report as cr
    from ffsubsync_amd import cue_retime as ct

    rng = np.random.RandomState(8)
    probs = [_pair(speechy(rng, 2100, 9), speechy(rng, 2000, 9)) for _ in range(3)]
    cues = [_file_cues(rng, 2000, 9000) for _ in probs]
    db = _device_batch(probs)
    table, first, count = cr.flat_cue_table(cues, 3)
    cell = 2049 * 6
    assert 2 * 9000 * cell <= _native.RETIME_WORK_CAP < 3 * 9000 * cell
    tdev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    outs = []
    for pif in (3, 1):
        plan = _native.SplitPlan(pif, 1, 2, 1)
        try:
            out = torch.full((table.size * 64,), 0xEE, dtype=torch.uint8, device="cuda")
            summ = torch.full((3 * 40,), 0xEE, dtype=torch.uint8, device="cuda")
            before = plan.workspace_bytes
            plan.cue_retime(*db.pair_arrays(), tdev, first, count, 1024, 3, 2, 4000, 1, out, summ)
            outs.append((out.cpu().numpy(), summ.cpu().numpy()))
            assert plan.workspace_bytes - before - _native.RETIME_DESC_BYTES * pif == ct.workspace_bytes(count, 1024, pif) == -(
                -min(pif, 2) * 9000 * cell // 256) * 256
        finally:
            plan.close()
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    sums = outs[0][1].view(_native.RETIME_SUMMARY_DTYPE)
    recs = outs[0][0].view(_native.CUE_RETIME_DTYPE)
    assert sums["n_live"].tolist() == [9000] * 3
    for p in range(3):  # the invariants, and the first cues of the third pair (the second sub-batch) against the model
        lv = recs[p * 9000:(p + 1) * 9000]
        assert sums[p]["own_total"] <= sums[p]["total"] <= sums[p]["best_total"]
        assert sums[p]["total"] == 64 * int(lv["at"].astype(np.int64).sum()) - int(lv["link"].sum())
    flags, pos, A = rm.profiles(rm.cm.Pair(probs[2]["rb"], probs[2]["sb"]), tuple(c[:50] for c in cues[2]), 1024, 3)
    head = recs[2 * 9000:2 * 9000 + 50]
    assert np.array_equal(head["own"], A[:, 1024]) and np.array_equal(head["best"], A.max(axis=1))
    assert np.array_equal(head["at"], A[np.arange(50), head["delta"] + 1024])


@pytest.mark.parametrize("keep_order", [True, False])
@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_tiny_cases_reach_the_enumerated_optimum(radius, keep_order):
    from ffsubsync_amd import cue_retime as ct

    rng = np.random.RandomState(1000 + 10 * radius + keep_order)
    n_checked = 0
    for jump_q in (-1, 0, 90, 4000):
        probs, cues = [], []
        while len(probs) < 6:
            R, S = int(rng.randint(20, 81)), int(rng.randint(20, 81))
            K = int(rng.randint(1, 7))
            st = rng.randint(-3, S, K)
            if rng.rand() < 0.6:
                st = np.sort(st)
            c = (st.astype(np.int64), (st + rng.randint(0, 14, K)).astype(np.int64), rng.randint(-6, 7, K).astype(np.int64))
            if len(rr.live_cues(S, c)) > rr.MAX_LIVE:
                continue
            probs.append(_pair((rng.rand(R) < 0.5).astype(np.uint8), (rng.rand(S) < 0.5).astype(np.uint8)))
            cues.append(c)
        db = _device_batch(probs)
        for pq in (0, 1, 64, 1000):
            context = int(rng.randint(0, 6))
            got, slices, sums = ct.retime_batch(db, cues, radius, context, pq, jump_q, keep_order, raw=True)
            for p, c, sl, sm in zip(probs, cues, slices, sums):
                ref = rr.Reference(p["rb"], p["sb"], c, radius, context, pq, jump_q, keep_order)
                live = got[sl][(got[sl]["flags"] & 3) == 0]
                assert int(sm["total"]) == ref.optimum()
                assert ref.value([int(x) for x in live["delta"]]) == ref.optimum()  # admissible, and attains it
                n_checked += 1
    assert n_checked == 96


@pytest.mark.parametrize("layout", lc.LAYOUTS)
def test_hostile_layouts(layout):
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import cue_report as cr

    probs, cues = EDGE
    vectors = [v for p in probs for v in (p["rb"], p["sb"])]
    img = lc.build(vectors, lc.U1, layout).upload()
    lo = [x for p in probs for x in (p["r_lv"][0], p["s_lv"][0])]
    hi = [x for p in probs for x in (p["r_lv"][1], p["s_lv"][1])]
    db = img.device_batch((len(probs), 2), lo, hi, lc.U1)
    table, first, count = cr.flat_cue_table(cues, len(probs))
    raw = table.view(np.uint8).reshape(-1)
    can = lc.Canaries([raw.size, table.size * 64, len(probs) * 40], [8, 24, 40])
    can.tensor(0).copy_(torch.from_numpy(raw.copy()).cuda())
    plan = _native.SplitPlan(2, 1, 2, 1)
    try:
        plan.cue_retime(*db.pair_arrays(), can.tensor(0), first, count, 33, 40, 16, 700, 1, can.tensor(1), can.tensor(2))
        got = can.tensor(1).cpu().numpy().view(_native.CUE_RETIME_DTYPE)
        sums = can.tensor(2).cpu().numpy().view(_native.RETIME_SUMMARY_DTYPE)
    finally:
        plan.close()
    want, want_sums = _model(probs, cues, 33, 40, 16, 700, True)
    _assert_same(got, want, layout)
    _assert_same(sums, want_sums, layout)
    img.assert_inputs_untouched("cue retime")
    can.assert_canaries_intact("cue retime")
    assert can.tensor(0).cpu().numpy().tobytes() == raw.tobytes()


def test_refusals_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import cue_report as cr

    probs, cues = EDGE
    db = _edge_batch()
    n = len(probs)
    table, first, count = cr.flat_cue_table(cues, n)
    dev = db.data.device
    tdev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(dev)
    out = torch.full((table.size * 64 + 8,), 0xAB, dtype=torch.uint8, device=dev)
    summ = torch.full((n * 40 + 8,), 0xAB, dtype=torch.uint8, device=dev)
    plan = _native.SplitPlan(2, 1, 2, 1)
    E_INVALID, E_EMPTY = -1, -5

    def arrays(**change):
        a = [np.array(x) for x in db.pair_arrays()]
        for k, v in change.items():
            a[int(k[1:])][1] = v
        return a

    neg, past, before, big, huge = count.copy(), first.copy(), first.copy(), count.copy(), count.copy()
    neg[1] = -1
    past[n - 1] += 1
    before[0] = -1
    big[0] = table.size + 1
    huge[0] = 30000  # 30000 cues x 2049 shifts x 6 bytes > 256 MiB: refused by name, whatever the table holds
    cases = [
        ("radius -1", dict(radius=-1), E_INVALID), ("radius 1025", dict(radius=1025), E_INVALID),
        ("context -1", dict(context=-1), E_INVALID), ("context 65537", dict(context=65537), E_INVALID),
        ("penalty -1", dict(penalty_q=-1), E_INVALID), ("penalty 2^20 + 1", dict(penalty_q=(1 << 20) + 1), E_INVALID),
        ("jump -2", dict(jump_q=-2), E_INVALID), ("jump 2^40 + 1", dict(jump_q=(1 << 40) + 1), E_INVALID),
        ("flag 2", dict(flags=2), E_INVALID), ("flag 3", dict(flags=3), E_INVALID), ("flag -1", dict(flags=-1), E_INVALID),
        ("negative count", dict(count=neg), E_INVALID), ("range past the table", dict(first=past), E_INVALID),
        ("range before the table", dict(first=before), E_INVALID), ("count past the table", dict(count=big), E_INVALID),
        ("short table", dict(n_cues=table.size - 1), E_INVALID), ("negative table", dict(n_cues=-1), E_INVALID),
        ("null table", dict(cue_ptr=0), E_INVALID), ("misaligned table", dict(cue_ptr=tdev.data_ptr() + 4), E_INVALID),
        ("null output", dict(out_ptr=0), E_INVALID), ("misaligned output", dict(out_ptr=out.data_ptr() + 4), E_INVALID),
        ("null summaries", dict(sum_ptr=0), E_INVALID), ("misaligned summaries", dict(sum_ptr=summ.data_ptr() + 4), E_INVALID),
        ("over the cap", dict(count=huge, n_cues=1 << 20, radius=1024), E_INVALID),
        ("negative pairs", dict(n_pairs=-1), E_INVALID), ("empty reference", dict(arrays=arrays(a1=0)), E_EMPTY),
        ("empty subtitle", dict(arrays=arrays(a5=0)), E_EMPTY), ("null vector", dict(arrays=arrays(a0=0)), E_INVALID),
        ("misaligned vector", dict(arrays=arrays(a4=int(db.pair_arrays()[4][1]) + 2)), E_INVALID),
        ("non-finite level", dict(arrays=arrays(a3=np.inf)), E_INVALID), ("no pairs", dict(n_pairs=0), 0),
    ]
    try:
        for what, change, code in cases:
            kw = dict(first=first, count=count)
            kw.update(change)
            got = _raw_call(plan, db, tdev, kw.pop("first"), kw.pop("count"), out, summ, **kw)
            assert got == code, (what, got, code)
            if code:
                assert _native.load().ffs_last_error()
                if what == "over the cap":
                    assert b"pair 0" in _native.load().ffs_last_error() and b"workspace cap" in _native.load().ffs_last_error()
            torch.cuda.synchronize()
            assert bool((out == 0xAB).all()) and bool((summ == 0xAB).all()), what
        assert _raw_call(plan, db, tdev, first, count, out, summ) == 0  # the same call, unabused, retimes
        torch.cuda.synchronize()
        want, want_sums = _model(probs, cues, 33, 9, 16, 500, True)
        assert out[:table.size * 64].cpu().numpy().tobytes() == want.tobytes()
        assert summ[:n * 40].cpu().numpy().tobytes() == want_sums.tobytes()
        assert bool((out[table.size * 64:] == 0xAB).all()) and bool((summ[n * 40:] == 0xAB).all())
        # no cues at all: the summaries are still written (all zeros), table and records may be null
        assert _raw_call(plan, db, tdev, first, np.zeros(n, np.int64), out, summ, cue_ptr=0, out_ptr=0) == 0
        torch.cuda.synchronize()
        assert not summ[:n * 40].any() and bool((summ[n * 40:] == 0xAB).all())
        assert out[:table.size * 64].cpu().numpy().tobytes() == want.tobytes()
    finally:
        plan.close()


def test_retime_sync_end_to_end():
    from ffsubsync_amd import cue_report as cr
    from ffsubsync_amd import cue_retime as ct
    from workloads import cue_stretches as ws

    pr = ws.make_stretch_problem(1, 600.0)
    res = ws.true_sync(pr)
    got, slices, sums = ct.retime_sync([pr.problem], [res], raw=True)
    cues, summaries = ct.retime_sync([pr.problem], [res])
    table = cr.cue_table(pr.start_us, pr.end_us, res.ratio, res.cue_start_us)
    sub = ws.host_subtitle_vector(pr, res.ratio)
    want, want_sum = rm.retime_fast(pr.ref, sub, table, ct.DEFAULT_RADIUS, ct.DEFAULT_CONTEXT, ct.DEFAULT_PENALTY_Q,
                                    ct.DEFAULT_JUMP_Q, True)
    _assert_same(got[slices[0]], want, "seed 1")
    assert sums[0].tobytes() == want_sum.tobytes()
    assert [c.delta for c in cues[0]] == want["delta"].tolist() and summaries[0].total == int(want_sum["total"])
    planted = pr.kind == ws.STRETCH
    model_ok = np.abs(want["delta"] + pr.displacement) <= 10
    device_ok = np.abs(got["delta"].astype(np.int64) + pr.displacement) <= 10
    assert planted.sum() >= 3 and (model_ok & planted).sum() >= 1
    assert not (planted & model_ok & ~device_ok).any()  # every planted cue the model recovers is recovered
    new_s, new_e = ct.apply_retime(res.cue_start_us, res.cue_end_us, cues[0])
    assert np.array_equal(new_s - res.cue_start_us, want["delta"].astype(np.int64) * 10000)
    assert np.array_equal(new_e - new_s, res.cue_end_us - res.cue_start_us)
    live = np.flatnonzero((want["flags"] & 3) == 0)
    pos = np.clip(want["start"], 0, sub.size) + want["lag"]
    a, b = live[:-1], live[1:]
    assert not ((pos[b] >= pos[a]) & (pos[b] + want["delta"][b] < pos[a] + want["delta"][a])).any()  # no order violation
