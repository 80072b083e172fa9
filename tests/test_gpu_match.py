"""All-pairs quality report from boundary lists on the device (csrc/ffs_match.h via ffsubsync_amd.match): records against
``quality_batch`` byte for byte and against the numpy model, edge lists in both roles, shared vectors and batching,
refusals before any output, matching end to end on synthetic files, and the existing entry points left where they were."""
import json
import os

import numpy as np
import pytest

import match_model as mm
import quality_model as qm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALGORITHMS = ("runs", "bits", "auto")


# ---- helpers ------------------------------------------------------------------------------------------------------
def _block(v01, cap=None):
    """The ``ffs_runs_list`` block of a 0/1 host vector as int32 words, built on the host (oracle.runs_model.boundaries):
    header (n, ones, len, cap), cap entries (position, ones in front), e[n] = (INT32_MAX, ones).  A ``cap`` <= n gives
    a truncated list: the header keeps the true n, the block holds the first cap entries."""
    v01 = np.asarray(v01) != 0
    pos, before = mm.rm.boundaries(v01)
    n, ones = int(pos.size), int(v01.sum())
    cap = n + 1 if cap is None else int(cap)
    e = np.zeros((cap, 2), dtype=np.int32)
    k = min(n, cap)
    e[:k, 0], e[:k, 1] = pos[:k], before[:k]
    if n < cap:
        e[n] = (np.iinfo(np.int32).max, ones)
    return np.concatenate([np.array([n, ones, v01.size, cap], dtype=np.int32), e.ravel()])


class Lists:
    """Boundary lists of 0/1 host vectors in one device buffer: pointers and lengths."""

    def __init__(self, vectors, caps=None):
        import torch

        blocks = [_block(v, None if caps is None else caps[i]) for i, v in enumerate(vectors)]
        self.lens = np.array([len(v) for v in vectors], dtype=np.int64)
        size = np.array([(b.size + 15) // 16 * 16 for b in blocks], dtype=np.int64)  # 64-byte aligned blocks
        offs = np.concatenate([[0], np.cumsum(size)[:-1]])
        host = np.zeros(int(size.sum()), dtype=np.int32)
        for b, o in zip(blocks, offs):
            host[o:o + b.size] = b
        self.data = torch.from_numpy(host).cuda()
        self.ptr = np.uint64(self.data.data_ptr()) + (4 * offs).astype(np.uint64)


def _raster01(v01, levels=(0.0, 1.0)):
    """DeviceRaster of a 0/1 host vector with explicit levels (a constant vector has no two levels of its own)."""
    import torch

    from ffsubsync_amd.subtitle_raster import DeviceRaster

    v01 = np.asarray(v01) != 0
    packed = np.packbits(v01, bitorder="little")
    host = np.zeros((v01.size + 31) // 32 * 4, dtype=np.uint8)
    host[:packed.size] = packed
    return DeviceRaster(torch.from_numpy(host).cuda().view(torch.int32), levels[0], levels[1], v01.size)


def _match(refs, subs, pair_ref, pair_sub, w, top_k=3, e=300, algorithm="runs", r_lv=None, s_lv=None, pif=None):
    """Records of ``ffs_match_quality_batch`` for 0/1 host vectors (levels (0, 1) unless given per vector)."""
    from ffsubsync_amd import match

    rl, sl = (refs, subs) if isinstance(refs, Lists) else (Lists(refs), Lists(subs))
    r_lv = [(0.0, 1.0)] * rl.lens.size if r_lv is None else r_lv
    s_lv = [(0.0, 1.0)] * sl.lens.size if s_lv is None else s_lv
    return match.quality_from_lists(rl.ptr, rl.lens, [a for a, _ in r_lv], [b for _, b in r_lv], sl.ptr, sl.lens,
                                    [a for a, _ in s_lv], [b for _, b in s_lv], pair_ref, pair_sub, w, top_k, e, algorithm,
                                    pairs_in_flight=pif)


def _quality(pairs, w, top_k=3, e=300):
    """Records of ``quality.quality_batch`` for (ref 0/1, ref levels, sub 0/1, sub levels) host pairs."""
    from ffsubsync_amd import batch, quality

    db = batch.pack_pairs([(_raster01(r, rl), [_raster01(s, sl)]) for r, rl, s, sl in pairs])
    return quality.quality_batch(db, w, top_k, e, raw=True)


def _small_problems(n=64):
    """R < S and R > S, non-default levels and amplitudes 1/ratio, top_k 1..8, E from 1 to beyond the window,
    windowless on short vectors, windows past both ends and the negative-slice window."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(7000 + seed)
        R, S = int(rng.randint(40, 12000)), int(rng.randint(40, 12000))
        w = [None, 1, 2, 37, 300, 2500, 6000, 30000][seed % 8]
        if w is None:
            R, S = R % 3000 + 40, S % 3000 + 40
        if seed % 16 == 15:  # negative-slice window: W past N - 1 - S
            R, S = int(rng.randint(40, 400)), int(rng.randint(400, 900))
            w = qm.orc.fft_length(R, S) - S + int(rng.randint(0, 30))
        top_k = 1 + seed % 8
        e = [1, 2, 50, 300, 5000, 10 ** 6][seed % 6]
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8), (0.0, 1.0)][seed % 4]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25), (0.0, 1.0)][seed % 5]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        shift = int(rng.randint(-min(w or 3000, 3000), min(w or 3000, 3000) + 1))
        idx = np.arange(S) + shift
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False
        out.append(dict(rb=rb, sb=sb, r_lv=r_lv, s_lv=s_lv, w=w, top_k=top_k, e=e))
    return out


SMALL = _small_problems()
_cache = {}


def _small_records(algorithm):
    """The device's records of every SMALL problem on one algorithm (computed once per session)."""
    if algorithm not in _cache:
        _cache[algorithm] = [_match([pr["rb"]], [pr["sb"]], [0], [0], pr["w"], pr["top_k"], pr["e"], algorithm,
                                    [pr["r_lv"]], [pr["s_lv"]])[0] for pr in SMALL]
    return _cache[algorithm]


def _small_quality():
    if "quality" not in _cache:
        _cache["quality"] = [_quality([(pr["rb"], pr["r_lv"], pr["sb"], pr["s_lv"])], pr["w"], pr["top_k"], pr["e"])[0]
                             for pr in SMALL]
    return _cache["quality"]


def _close(a, b, scale):
    """|a - b| within 4 ulps of ``scale``, the magnitude of the terms a score sums (test_gpu_quality's rule)."""
    return abs(a - b) <= 4 * np.spacing(scale)


def _compare(q, pr):
    """None if the device's AlignmentQuality matches the model's report of problem ``pr``, else a description
    (test_gpu_quality's comparison rule: exact for 0/1 levels, 4 ulps otherwise)."""
    rep = qm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["w"], pr["top_k"], pr["e"])
    exact = pr["r_lv"] == (0.0, 1.0) and pr["s_lv"] == (0.0, 1.0)
    if q.n_lags != rep["n_lags"] or len(q.peaks) != len(rep["peaks"]):
        return ("n", q.n_lags, rep["n_lags"], len(q.peaks), len(rep["peaks"]))
    lags, sc = qm.scores(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["w"])
    m = lambda x: 2.0 * x - 1.0
    scale = min(pr["rb"].size, pr["sb"].size) * max(abs(m(a) * m(b)) for a in pr["r_lv"] for b in pr["s_lv"])
    for (ds, do), (ms, mo) in zip(q.peaks, rep["peaks"]):
        if exact:
            if do != mo or np.float64(ds).view(np.int64) != np.float64(ms).view(np.int64):
                return ("peak", ds, do, ms, mo)
            continue
        if do != mo:
            if not _close(float(sc[np.searchsorted(lags, do)]), ms, scale):
                return ("offset", do, mo)
            break
        if not _close(ds, ms, scale):
            return ("score", ds, ms)
    for got, want in ((q.mean, rep["mean"]), (q.std, rep["std"])):
        if abs(got - want) > 1e-9 * max(abs(want), 1e-300) and not (got == want == 0.0):
            return ("moments", q.mean, rep["mean"], q.std, rep["std"])
    if (q.flags & qm.FLAT) != (rep["flags"] & qm.FLAT):
        return ("flags", q.flags, rep["flags"])
    return None


# ---- 1, 2: the records ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_records_equal_quality_batch_byte_for_byte(algorithm):
    want = _small_quality()
    got = _small_records(algorithm)
    bad = [(i, SMALL[i]["w"], SMALL[i]["top_k"], SMALL[i]["e"]) for i in range(len(SMALL)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, bad[:8]
    assert sum(pr["w"] is None for pr in SMALL) >= 8
    assert sum(qm.lag_set(pr["rb"].size, pr["sb"].size, pr["w"]).size < 2 * (pr["w"] or 0) for pr in SMALL) >= 4
    assert any(pr["rb"].size < pr["sb"].size for pr in SMALL) and any(pr["rb"].size > pr["sb"].size for pr in SMALL)


def test_records_equal_the_model():
    from ffsubsync_amd import quality

    bad = []
    for i, (pr, rec) in enumerate(zip(SMALL, _small_records("runs"))):
        why = _compare(quality.from_record(rec), pr)
        if why is not None:
            bad.append((i, pr["w"], pr["top_k"], pr["e"], why))
    assert not bad, bad[:5]


# ---- 3: edge lists -------------------------------------------------------------------------------------------------
def _edge_vectors():
    rng = np.random.RandomState(42)
    touch = np.zeros(900, bool)
    touch[:7] = touch[-5:] = touch[300:420] = True  # runs that touch sample 0 and the last sample
    alt = (np.arange(12000) & 1) == 0  # 12 000 boundaries: longer than one LDS stage of the reference list
    seg = np.maximum(1, rng.geometric(1.0 / 40.0, size=200))
    plain = np.repeat(rng.rand(seg.size) < 0.5, seg)[:5000]
    return [np.zeros(500, bool), np.ones(700, bool), touch, alt, plain]


@pytest.mark.parametrize("w", [300, None])
def test_edge_lists_in_both_roles(w):
    vecs = _edge_vectors()
    n = len(vecs)
    pr, ps = np.divmod(np.arange(n * n), n)
    lists = Lists(vecs)
    got = _match(lists, lists, pr, ps, w, 4, 50, "runs")
    want = _quality([(vecs[i], (0.0, 1.0), vecs[j], (0.0, 1.0)) for i, j in zip(pr, ps)], w, 4, 50)
    bad = [(int(i), int(j)) for k, (i, j) in enumerate(zip(pr, ps)) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, bad
    for k in (0 * n + 3, 3 * n + 1, 2 * n + 2, 3 * n + 3):  # and straight against the model
        i, j = int(pr[k]), int(ps[k])
        rep = qm.report(vecs[i], vecs[j], (0.0, 1.0), (0.0, 1.0), w, 4, 50)
        assert [(float(a), int(b)) for a, b in zip(got[k]["peak_score"][:got[k]["n_peaks"]], got[k]["peak_offset"])] == rep["peaks"]
        assert int(got[k]["n_lags"]) == rep["n_lags"] and (int(got[k]["flags"]) & qm.FLAT) == (rep["flags"] & qm.FLAT)


def test_largest_cell_value():
    """Two identical alternating vectors of 65 532 samples, W = 64: h(0) = +65 532 and h(+-1) = -65 531, the largest
    second differences a pair of that length can have.  n11 at lags -1, 0, +1 against the model: lag 0 is peak 1 under
    levels (0, 1); with the reference's levels swapped every score changes sign and lags +-1 lead."""
    n = 65532
    alt = (np.arange(n) & 1) == 0
    lists = Lists([alt])
    lags = np.array([-1, 0, 1])
    n11, n1x, nx1, ov = qm.counts(alt, alt, lags)
    assert n11.tolist() == [0, n // 2, 0]
    assert [x.tolist() for x in mm.counts_sparse(alt, alt, lags)] == [n11.tolist(), n1x.tolist(), nx1.tolist(), ov.tolist()]
    plain = _match(lists, lists, [0], [0], 64, 3, 1, "runs")[0]
    swapped = _match(lists, lists, [0], [0], 64, 3, 1, "runs", r_lv=[(1.0, 0.0)])[0]
    # levels (0, 1) on both sides: score = ov - 2 (n1x + nx1) + 4 n11
    assert int(plain["peak_offset"][0]) == 0
    assert (float(plain["peak_score"][0]) - ov[1] + 2 * (n1x[1] + nx1[1])) / 4 == n11[1]
    assert sorted(int(x) for x in swapped["peak_offset"][:2]) == [-1, 1]
    for k in range(2):
        i = int(swapped["peak_offset"][k]) + 1
        assert (-float(swapped["peak_score"][k]) - ov[i] + 2 * (n1x[i] + nx1[i])) / 4 == n11[i]
    for rec, lv in ((plain, (0.0, 1.0)), (swapped, (1.0, 0.0))):
        assert rec.tobytes() == _quality([(alt, lv, alt, (0.0, 1.0))], 64, 3, 1)[0].tobytes()
        for alg in ("bits", "auto"):
            assert _match(lists, lists, [0], [0], 64, 3, 1, alg, r_lv=[lv])[0].tobytes() == rec.tobytes()


def test_several_lag_tiles_and_a_window_that_ends_mid_tile():
    from ffsubsync_amd import quality

    rng = np.random.RandomState(9)
    seg = np.maximum(1, rng.geometric(1.0 / 50.0, size=1200))
    r = np.repeat(rng.rand(seg.size) < 0.45, seg)[:20000]
    s = np.roll(r, 777) ^ (rng.rand(20000) < 0.05)
    for w in (None, 2500):  # 65 536 lags = 16 tiles of 4096; 5000 lags = one tile and 904 lags of the next
        got = _match([r], [s], [0], [0], w, 5, 300, "runs")[0]
        assert int(got["n_lags"]) == (65536 if w is None else 5000)
        assert got.tobytes() == _quality([(r, (0.0, 1.0), s, (0.0, 1.0))], w, 5, 300)[0].tobytes(), w
        assert _compare(quality.from_record(got), dict(rb=r, sb=s, r_lv=(0.0, 1.0), s_lv=(0.0, 1.0), w=w, top_k=5, e=300)) is None


# ---- 4: sharing and batching ----------------------------------------------------------------------------------------
def _table(n, seed, lo=1500, hi=4000):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        size = int(rng.randint(lo, hi))
        seg = np.maximum(1, rng.geometric(1.0 / 45.0, size=size // 10 + 16))
        out.append(np.repeat(rng.rand(seg.size) < 0.45, seg)[:size])
    return out


def test_shared_vectors_pair_order_batching_and_plan_reuse():
    from ffsubsync_amd import match

    refs, subs = _table(5, 1), _table(7, 2)
    rng = np.random.RandomState(3)
    order = rng.permutation(35)
    order = np.concatenate([order, order[:5], [order[0]]])  # scrambled, with repeats
    pr, ps = np.divmod(order, 7)
    rl, sl = Lists(refs), Lists(subs)
    want = _quality([(refs[i], (0.0, 1.0), subs[j], (0.0, 1.0)) for i, j in zip(pr, ps)], 2500, 5, 120)
    for alg in ALGORITHMS:
        for pif in (1, 7, None):
            match.clear_plan_cache()
            got = _match(rl, sl, pr, ps, 2500, 5, 120, alg, pif=pif)
            assert got.tobytes() == want.tobytes(), (alg, pif)
    # one plan, calls with different windows
    match.clear_plan_cache()
    first = _match(rl, sl, pr, ps, 2500, 5, 120, "runs")
    other = _match(rl, sl, pr, ps, 300, 5, 120, "runs")
    again = _match(rl, sl, pr, ps, 2500, 5, 120, "runs")
    assert first.tobytes() == want.tobytes() == again.tobytes()
    assert other.tobytes() == _quality([(refs[i], (0.0, 1.0), subs[j], (0.0, 1.0)) for i, j in zip(pr, ps)], 300, 5, 120).tobytes()


def _interval_track(spec_starts, spec_ends):
    start, end = spec_starts.astype(np.int64) * 10000, spec_ends.astype(np.int64) * 10000
    keep = end > start
    return start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)


def _spec_track(spec):
    j = spec.ratios.index(1.0)
    return _interval_track(spec.cand_starts[j], spec.cand_ends[j])


def test_a_batch_whose_rows_share_vectors_solves_like_private_copies():
    """The seven-ratio solve on a DeviceBatch whose rows point at shared boundary lists (what match_quality builds)
    against one with a private copy of every vector per pair: identical candidate and pair records."""
    from ffsubsync_amd import _native, batch
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import synth

    ratios = list(candidate_ratios())
    specs = [synth.make_pair_spec(seed, duration_s=300.0) for seed in (20, 21, 22)]
    ref_tracks = [_interval_track(sp.ref_starts, sp.ref_ends) for sp in specs]
    sub_tracks = [_spec_track(sp) for sp in specs]
    pairs = [(i, j) for i in range(3) for j in range(3)]
    private = batch.pairs_from_intervals([(ref_tracks[i], sub_tracks[j]) for i, j in pairs], ratios, lists=True)
    track_of = np.concatenate([np.arange(3), 3 + np.repeat(np.arange(3), 7)])
    ratio = np.concatenate([np.ones(3), np.tile(ratios, 3)])
    data, offs, lens, bounds = batch.TrackSet(ref_tracks + sub_tracks).rasterize_runs(track_of, ratio)
    hi = np.minimum(1.0 / ratio, 1.0)
    rows = np.array([[i] + [3 + 7 * j + k for k in range(7)] for i, j in pairs])
    shared = batch.DeviceBatch(data, offs[rows], lens[rows], np.zeros(rows.shape), hi[rows], _native.FFS_DTYPE_RUNS, None,
                               bounds[rows])
    assert np.array_equal(shared.lens, private.lens) and np.unique(shared.offs).size == 24 and np.unique(private.offs).size == 72
    out = []
    for db in (shared, private):
        al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=9)
        try:
            out.append(al.solve(db))
        finally:
            al.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert [int(b) for b in out[0][1]["best_cand"][[0, 4, 8]]] == [sp.true_ratio_index for sp in specs]


# ---- 5: refusals ----------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_output():
    from ffsubsync_amd import _native, match

    torch = _native.require_gpu()
    refs, subs = _table(2, 5, 400, 600), _table(2, 6, 400, 600)
    rl, sl = Lists(refs), Lists(subs)
    cut = Lists(refs, caps=[None, 4])  # the second list does not fit its block: n >= cap
    plan = _native.MatchPlan(4, 4096, 1024, 4)
    out = torch.zeros(4 * 160, dtype=torch.uint8, device="cuda")
    z, o = lambda n: np.zeros(n), lambda n: np.ones(n)

    def call(r=rl, s=sl, pr=(0, 1), ps=(1, 0), w=300, k=3, e=300, alg="runs", n_ref=2):
        plan.report(r.ptr[:n_ref], r.lens[:n_ref], z(n_ref), o(n_ref), s.ptr, s.lens, z(2), o(2), pr, ps, w, k, e, out, alg)

    try:
        cases = [(dict(r=cut), -1, "truncated"), (dict(s=cut), -1, "truncated"), (dict(pr=(0, 2)), -1, "index"),
                 (dict(ps=(-1, 0)), -1, "index"), (dict(k=0), -1, "top_k"), (dict(k=9), -1, "top_k"),
                 (dict(e=0), -1, "exclusion_samples"), (dict(alg=7), None, "algorithm")]
        for kw, code, word in cases:
            with pytest.raises((_native.NativeError, ValueError)) as err:
                call(**kw)
            assert word in str(err.value), (kw, str(err.value))
            if code is not None:
                assert err.value.code == code, kw
        small = _native.MatchPlan(4, 256, 1024, 3)
        try:
            with pytest.raises(_native.NativeError) as err:
                small.report(rl.ptr, rl.lens, z(2), o(2), sl.ptr, sl.lens, z(2), o(2), (0,), (0,), 300, 3, 300, out)
            assert err.value.code == -1 and "max_vectors" in str(err.value)
            with pytest.raises(_native.NativeError) as err:  # a vector longer than max_samples, a lag set beyond max_lags
                small.report(rl.ptr[:1], [2000], z(1), o(1), sl.ptr[:1], sl.lens[:1], z(1), o(1), (0,), (0,), 100, 3, 300, out)
            assert err.value.code == -1 and "max_samples" in str(err.value)
            with pytest.raises(_native.NativeError) as err:
                small.report(rl.ptr[:1], rl.lens[:1], z(1), o(1), sl.ptr[:1], sl.lens[:1], z(1), o(1), (0,), (0,), 300, 3, 300, out)
            assert err.value.code == -1 and "max_lags" in str(err.value)
            with pytest.raises(_native.NativeError) as err:
                small.report(rl.ptr[:1], [0], z(1), o(1), sl.ptr[:1], sl.lens[:1], z(1), o(1), (0,), (0,), 100, 3, 300, out)
            assert err.value.code == -5
        finally:
            small.close()
        torch.cuda.synchronize()
        assert int(out.sum()) == 0
        call()  # and the plan still serves a good call
        torch.cuda.synchronize()
        assert int(out[:320].to(torch.int64).sum()) != 0 and int(out[320:].sum()) == 0
    finally:
        plan.close()
    for kw in (dict(top_k=0), dict(top_k=9), dict(e=0), dict(algorithm="fft")):
        with pytest.raises(ValueError):
            _match(rl, sl, [0], [0], 300, **kw)
    with pytest.raises(ValueError, match="pair index"):
        _match(rl, sl, [0], [2], 300)
    del match


# ---- 6: matching end to end -----------------------------------------------------------------------------------------
def _library():
    """make_pair_spec seeds 0-7 (odd: 1 h, even: 10 min) with the subtitle order permuted, one subtitle without a video
    (seed 40's track) and one video without a subtitle (seed 41's reference)."""
    from workloads import synth

    dur = lambda seed: 3600.0 if seed & 1 else 600.0
    specs = [synth.make_pair_spec(seed, duration_s=dur(seed)) for seed in range(8)]
    orphan_sub = synth.make_pair_spec(40, duration_s=dur(40))
    orphan_ref = synth.make_pair_spec(41, duration_s=dur(41))
    refs = [synth.rasterize(sp.ref_len, sp.ref_starts, sp.ref_ends) for sp in specs + [orphan_ref]]
    perm = [5, 2, 7, 0, 3, 6, 1, 4]  # subtitle j belongs to video perm[j]
    tracks = [_spec_track(specs[i]) for i in perm] + [_spec_track(orphan_sub)]
    return specs, refs, tracks, perm


def test_match_library_end_to_end():
    from ffsubsync_amd import match
    from ffsubsync_amd.constants import candidate_ratios

    specs, refs, tracks, perm = _library()
    lib = match.match_library([r.astype(float) for r in refs], tracks, raw=True)
    m, a = lib.matrix, lib.assignment
    assert m.shape == (9, 9)
    assert a.reference == perm + [None]
    assert not a.ambiguous.any() and np.isnan(a.runner_up_psr).all()
    assert a.subtitles[8] == [] and sorted(j for s in a.subtitles for j in s) == list(range(8))
    for j, i in enumerate(perm):
        assert int(m.ratio_index[i, j]) == specs[i].true_ratio_index, (i, j)
        assert abs(int(m.offset[i, j]) - specs[i].true_offset_samples) <= 2, (i, j)
    assert [(p["subtitle"], p["reference"], p["ratio_index"], p["offset"]) for p in lib.pairs] == \
        [(j, i, int(m.ratio_index[i, j]), int(m.offset[i, j])) for j, i in enumerate(perm)]
    # peaks[0] of every pair is the solve's record, bit for bit
    found = m.ratio_index >= 0
    assert found.sum() >= 72
    assert m.records["peak_score"][..., 0][found].tobytes() == m.score[found].tobytes()
    assert np.array_equal(m.records["peak_offset"][..., 0][found], m.offset[found])
    assert (m.records["n_lags"][found] == 12000).all()
    # the device matrix against the model's
    model = mm.matrix(refs, tracks, 6000, list(candidate_ratios()), scores=mm.scores_sparse)
    want = mm.trusted(model)
    assert np.array_equal(m.trusted(), want), (m.psr, model["psr"])
    assert want.sum() == 8 and all(want[i, j] for j, i in enumerate(perm))
    assert mm.assign(model)["reference"] == a.reference
    for j, i in enumerate(perm):
        assert int(model["ratio_index"][i, j]) == int(m.ratio_index[i, j]) and int(model["offset"][i, j]) == int(m.offset[i, j])
        assert abs(float(model["score"][i, j]) - float(m.score[i, j])) <= 4 * np.spacing(float(refs[i].size))  # (_close's rule)
        assert abs(float(model["psr"][i, j]) - float(m.psr[i, j])) <= 1e-9 * float(model["psr"][i, j])
    # a subset of pairs, in another order: the same entries, nothing else requested
    sub = match.match_quality([r.astype(float) for r in refs], tracks, pairs=[(5, 0), (0, 3), (8, 8), (0, 0)])
    for i, j in ((5, 0), (0, 3), (8, 8), (0, 0)):
        assert (int(sub.ratio_index[i, j]), int(sub.offset[i, j]), float(sub.psr[i, j])) == \
            (int(m.ratio_index[i, j]), int(m.offset[i, j]), float(m.psr[i, j]))
    assert (sub.ratio_index >= 0).sum() <= 4


# ---- 7: nothing existing moved ----------------------------------------------------------------------------------------
def test_existing_entry_points_are_unmoved_by_match_calls():
    from ffsubsync_amd import batch, quality
    from workloads import synth

    gold = json.load(open(os.path.join(HERE, "golden", "headline_golden.json")))["pairs"][:16]
    db = synth.build_device_batch([synth.make_pair_spec(g["seed"]) for g in gold])

    def existing():
        al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=16)
        try:
            cres, pres = al.solve(db)
        finally:
            al.close()
        recs = quality.quality_batch(db.select_candidates(pres["best_cand"].astype(np.int64)), 6000, raw=True)
        return cres.tobytes(), pres.tobytes(), recs.tobytes(), pres

    before = existing()
    refs, subs = _table(3, 8), _table(4, 9)
    pr, ps = np.divmod(np.arange(12), 4)
    for alg in ALGORITHMS:
        _match(refs, subs, pr, ps, 2500, 3, 300, alg)
    after = existing()
    assert before[:3] == after[:3]
    assert [int(o) for o in after[3]["offset"]] == [g["offset"] for g in gold]
    assert [int(b) for b in after[3]["best_cand"]] == [g["index"] for g in gold]
