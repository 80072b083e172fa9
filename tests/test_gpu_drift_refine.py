"""Sample-exact jumps of a drift solve on the device (csrc/ffs_drift_refine.h via ffsubsync_amd.drift_refine): bit for
bit against the numpy model tests/drift_refine_model.py on seeded paths (jumps at the first and last block, adjacent
jumps, none, one per block, partners off either end of the reference, |o| > R), the widest window and the widest block,
sub-batches, the identity with ffs_split_refine_batch, a split plan untouched by the call, the refusals, hostile input
layouts, and the two entry points end to end."""
import math

import numpy as np
import pytest

import drift_refine_model as drm

pytestmark = pytest.mark.gpu

K = 256
RADII = (1, 100, 5000)
BETAS = (None, 0.0, 0.25, 1.0)


def _device_pairs(problems):
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs)


def _walk(rng, n_b, jumps, base, spread=3000):
    """Block offsets moving -2 .. 2 per block, by up to ``spread`` at the blocks of ``jumps``; the jump flags."""
    o = np.zeros(n_b, np.int64)
    o[0] = base
    for b in range(1, n_b):
        o[b] = o[b - 1] + (int(rng.randint(-spread, spread + 1)) if b in jumps else int(rng.randint(-2, 3)))
    jf = np.zeros(n_b, np.uint8)
    jf[list(jumps)] = 1
    jf[0] = int(rng.randint(2))  # ignored by the contract
    return o.astype(np.int32), jf


def _vectors(rng, R, S, o, k, r_lv, s_lv):
    """A run-structured reference and a subtitle that follows the path ``o`` a few samples off the block grid."""
    seg = np.maximum(1, rng.geometric(1.0 / 40.0, size=R // 10 + 16))
    rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
    rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
    idx = np.arange(S) + np.repeat(o.astype(np.int64), k)[:S] + int(rng.randint(-8, 9))
    sb = rng.rand(S) < 0.3
    ok = (idx >= 0) & (idx < R)
    sb[ok] = rb[idx[ok]]
    sb ^= rng.rand(S) < 0.08
    rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
    return dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                s_lv=s_lv, o=o, k=k)


def _fuzz_problems(n=64):
    """Seeded pairs at K = 256, S in 3 000 .. 20 000 (most no multiple of K or of 32), R != S, 0-6 jumps.  By seed % 8:
    0 jumps at block 1 and block B-1; 1 two adjacent jumps; 2 no jump; 3 a jump at every block; 4 / 5 a window partly
    off the low / the high end of the reference; 6 |o| > R; 7 as drawn.  Subtitle levels 1/ratio among them."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(7300 + seed)
        S = int(rng.randint(12000 if seed % 3 == 2 else 3000, 20001))  # radius 5 000 gets room for a wide window
        if seed % 16 == 9:
            S = S // K * K  # a few multiples of K too: U = S on a block boundary
        R = S + int(rng.choice([-1500, -333, 77, 1200, 4000]))
        n_b = -(-S // K)
        kind = seed % 8
        n_j = int(rng.randint(0, 7))
        jumps = set(rng.choice(np.arange(1, n_b), size=min(n_j, n_b - 1), replace=False).tolist())
        base, spread = int(rng.randint(-300, 301)), 3000
        if kind == 0:
            jumps |= {1, n_b - 1}
        elif kind == 1:
            b = int(rng.randint(2, n_b - 1))
            jumps |= {b, b + 1}
        elif kind == 2:
            jumps = set()
        elif kind == 3:
            jumps, spread = set(range(1, n_b)), 50
        elif kind in (4, 5):
            f = int(rng.randint(n_b // 3, 2 * n_b // 3 + 1))
            jumps = {f}
            base, spread = (-f * K + 40 if kind == 4 else R - f * K - 40), 30
        elif kind == 6:
            base, spread = [R + 3000, -(R + S + 3000)][seed // 8 % 2], 200
        o, jf = _walk(rng, n_b, jumps, base, spread)
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8)][seed % 3]
        s_lv = [(0.0, 25.0 / 24.0), (0.0, 1.0), (0.0, 1.001), (-0.5, 1.25), (0.0, 24.0 / 23.976)][seed % 5]
        pr = _vectors(rng, R, S, o, K, r_lv, s_lv)
        pr.update(jf=jf, kind=kind, radius=RADII[seed % 3], beta=BETAS[(seed // 3) % 4])
        out.append(pr)
    return out


FUZZ = _fuzz_problems()


def _drift_result(pr):
    from ffsubsync_amd import drift_align as da

    sc = np.zeros(pr["o"].size)
    return da.DriftResult(da.segments_from_blocks(pr["o"], sc, pr["jf"], pr["k"], pr["sb"].size), 0.0, pr["o"], sc, pr["jf"])


_OWN = object()


def _model(pr, radius=_OWN, beta=_OWN):
    """The model's records of a problem, at its own radius and margin unless given."""
    return drm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["o"], pr["jf"], pr["k"],
                      pr["radius"] if radius is _OWN else radius, pr["beta"] if beta is _OWN else beta)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _diff(got, want):
    """Names of the fields that differ, bit for bit (the record count first)."""
    if got.shape != want.shape:
        return ["count %d != %d" % (got.size, want.size)]
    return [f for f in want.dtype.names if not _same_bits(got[f], want[f])]


def test_device_equals_model_bit_for_bit():
    """The 64 seeded pairs, one call per (radius, margin) with every pair of that cell in it, so the rows of a call have
    different block counts and the zeroed tails are checked against max_b."""
    from ffsubsync_amd import drift_refine as dref

    bad, seen = [], dict(jumps=0, unmatched=0, clipped=0, wide=0, kinds=set())
    for radius in RADII:
        for beta in BETAS:
            cell = [pr for pr in FUZZ if pr["radius"] == radius and pr["beta"] == beta]
            assert cell
            db = _device_pairs([(pr["ref"], pr["sub"]) for pr in cell])
            recs, counts = dref.refine_jumps_batch(db, [_drift_result(pr) for pr in cell], K, radius, beta, raw=True)
            assert recs.shape[1] == max(pr["o"].size for pr in cell)
            for p, pr in enumerate(cell):
                want = _model(pr)
                assert len(want) == len(drm.jumps_of(pr["jf"]))
                n = int(counts[p])
                d = _diff(recs[p, :n], want) + (["tail"] if recs[p, n:].tobytes().strip(b"\0") else [])
                if d:
                    bad.append((pr["kind"], radius, beta, pr["sb"].size, n, d))
                seen["jumps"] += len(want)
                seen["unmatched"] += int((want["flags"] & drm.UNMATCHED != 0).sum())
                seen["clipped"] += int((want["flags"] & drm.CLIPPED != 0).sum())
                seen["wide"] += int(((want["hi"] >> 5) - (want["lo"] >> 5) + 1 > 256).sum())  # a thread owns several words
                seen["kinds"].add(pr["kind"])
    assert not bad, bad[:6]
    assert seen["jumps"] >= 300 and seen["unmatched"] >= 5 and seen["clipped"] >= 100 and seen["wide"] >= 5 \
        and seen["kinds"] == set(range(8)), seen
    dref.clear_plan_cache()


def _raw_call(plan, db, offs, jumps, k, radius, beta, rec=None, cnt=None):
    """SplitPlan.drift_refine on a one-candidate DeviceBatch; (records [n, max_b], counts, the two output tensors)."""
    import torch

    from ffsubsync_amd import _native

    n, max_b = offs.shape
    dev = db.data.device
    rec = torch.zeros(n * max_b * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev) if rec is None else rec
    cnt = torch.zeros(n, dtype=torch.int32, device=dev) if cnt is None else cnt
    plan.drift_refine(*db.pair_arrays(), k, torch.from_numpy(np.ascontiguousarray(offs).reshape(-1)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(jumps).reshape(-1)).to(dev), radius,
                      math.nan if beta is None else beta, rec, cnt)
    return rec.cpu().numpy().view(_native.BREAK_REFINE_DTYPE).reshape(n, max_b), cnt.cpu().numpy(), rec, cnt


def _rows(probs):
    max_b = max(pr["o"].size for pr in probs)
    offs, jumps = np.zeros((len(probs), max_b), np.int32), np.zeros((len(probs), max_b), np.uint8)
    for p, pr in enumerate(probs):
        offs[p, :pr["o"].size], jumps[p, :pr["o"].size] = pr["o"], pr["jf"]
    return offs, jumps


@pytest.mark.parametrize("beta", [None, 0.25])
def test_widest_window(beta):
    """S = 300 000 at K = 256 with one jump in the middle and the largest radius: a window of 262 144 samples over 1 025
    blocks, the top of the LDS staging, 33 words per thread."""
    from ffsubsync_amd import drift_refine as dref

    rng = np.random.RandomState(31)
    S, R = 300000, 290017
    n_b = -(-S // K)
    o, jf = _walk(rng, n_b, {586}, -150, 4000)
    pr = _vectors(rng, R, S, o, K, (0.0, 1.0), (0.0, 25.0 / 24.0))
    pr.update(jf=jf)
    want = _model(pr, 131072, beta)
    assert len(want) == 1 and want[0]["hi"] - want[0]["lo"] == 262144
    assert int(want[0]["hi"]) // K - int(want[0]["lo"]) // K + 1 == 1025 > 1024
    la, lb = drm.sample_lags(o, K, 586, int(want[0]["lo"]), int(want[0]["hi"]))
    assert len(set(la.tolist())) > 10 and len(set(lb.tolist())) > 10  # the lookup matters
    db = _device_pairs([(pr["ref"], pr["sub"])])
    recs, counts = dref.refine_jumps_batch(db, [_drift_result(pr)], K, 131072, beta, raw=True)
    assert int(counts[0]) == 1 and not _diff(recs[0, :1], want), _diff(recs[0, :1], want)
    assert not recs[0, 1:].tobytes().strip(b"\0")
    dref.clear_plan_cache()


def test_widest_block():
    """K = 32 768 and radius 5 000: every window lies inside one block on each side of its cut."""
    from ffsubsync_amd import drift_refine as dref

    rng = np.random.RandomState(32)
    k, S, R = 32768, 4 * 32768 + 4321, 4 * 32768 - 999
    o, jf = _walk(rng, 5, {1, 3, 4}, 77, 2000)
    pr = _vectors(rng, R, S, o, k, (-1.0, 2.5), (0.0, 24.0 / 25.0))
    pr.update(jf=jf)
    db = _device_pairs([(pr["ref"], pr["sub"])])
    for beta in (None, 0.25):
        want = _model(pr, 5000, beta)
        recs, counts = dref.refine_jumps_batch(db, [_drift_result(pr)], k, 5000, beta, raw=True)
        assert int(counts[0]) == 3 and not _diff(recs[0, :3], want), _diff(recs[0, :3], want)
    dref.clear_plan_cache()


def test_sub_batches_in_shuffled_order_equal_the_per_pair_results():
    from ffsubsync_amd import _native

    order = np.random.RandomState(5).permutation(len(FUZZ))[:8]
    probs = [FUZZ[i] for i in order]
    assert len({pr["o"].size for pr in probs}) >= 4
    db = _device_pairs([(pr["ref"], pr["sub"]) for pr in probs])
    offs, jumps = _rows(probs)
    plan = _native.SplitPlan(3, 1, 2, 1)  # 3 pairs in flight: sub-batches of 3, 3 and 2
    try:
        recs, counts, _, _ = _raw_call(plan, db, offs, jumps, K, 700, 0.25)
    finally:
        plan.close()
    total = 0
    for p, pr in enumerate(probs):
        want = _model(pr, 700, 0.25)
        n = int(counts[p])
        assert not _diff(recs[p, :n], want) and not recs[p, n:].tobytes().strip(b"\0"), (p, _diff(recs[p, :n], want))
        total += n
    assert total >= 8


def test_constant_segments_equal_split_refine_byte_for_byte():
    """16 of test_gpu_split_refine's split problems: the split solve's offsets with a flag wherever they change give
    ffs_split_refine_batch's records and counts, whole buffers compared."""
    import test_gpu_split_refine as t_refine
    from ffsubsync_amd import drift_align as da
    from ffsubsync_amd import drift_refine as dref
    from ffsubsync_amd import split_align as sa
    from ffsubsync_amd import split_refine as sr

    n_breaks = 0
    for pr in t_refine.SMALL[:16]:
        db = t_refine._device_pairs([(pr["ref"], pr["sub"])])
        res = sa.split_align_batch(db, pr["w"], pr["k"], pr["p"])
        o = res[0].block_offsets
        jf = np.concatenate([[1], o[1:] != o[:-1]]).astype(np.uint8)
        want, want_n = sr.refine_breaks_batch(db, res, pr["k"], pr["radius"], pr["beta"], raw=True)
        d = da.DriftResult(da.segments_from_blocks(o, res[0].block_scores, jf, pr["k"], pr["sb"].size), res[0].total, o,
                           res[0].block_scores, jf)
        got, got_n = dref.refine_jumps_batch(db, [d], pr["k"], pr["radius"], pr["beta"], raw=True)
        assert got.tobytes() == want.tobytes() and got_n.tobytes() == want_n.tobytes()
        n_breaks += int(want_n[0])
    assert n_breaks >= 30
    sa.clear_plan_cache()
    sr.clear_plan_cache()
    dref.clear_plan_cache()


def test_nothing_else_moves_on_the_plan():
    """Split results and ffs_split_refine_batch records of one plan are byte-identical before and after a drift-refine
    call; a plan that never refines keeps its workspace size, and the first call of either kind adds the same bytes."""
    import torch

    import test_gpu_split_refine as t_refine
    from ffsubsync_amd import _native

    pr = t_refine.SMALL[1]
    db = t_refine._device_pairs([(pr["ref"], pr["sub"])])
    a = db.pair_arrays()
    k, w = 256, 2500
    mb = int(-(-a[5][0] // k))
    dev = db.data.device
    plan = _native.SplitPlan(1, mb, 2 * w, int(a[5][0]))
    other = _native.SplitPlan(1, mb, 2 * w, int(a[5][0]))
    try:
        ws_new = plan.workspace_bytes
        outs = [torch.empty(mb, dtype=torch.int32, device=dev), torch.empty(mb, dtype=torch.float64, device=dev),
                torch.empty(1, dtype=torch.float64, device=dev)]
        new = lambda: (torch.empty(mb * _native.BREAK_REFINE_BYTES, dtype=torch.uint8, device=dev),
                       torch.empty(1, dtype=torch.int32, device=dev))
        plan.align(*a, k, w, 10.0, *outs)
        first = [t.clone() for t in outs]
        assert plan.workspace_bytes == ws_new == other.workspace_bytes  # never refined: the split workspace alone
        rec0, cnt0 = new()
        other.refine(*a, k, outs[0], 3000, 0.25, rec0, cnt0)
        jf = torch.cat([torch.zeros(1, dtype=torch.bool, device=dev), outs[0][1:] != outs[0][:-1]]).to(torch.uint8)
        rec1, cnt1 = new()
        plan.drift_refine(*a, k, outs[0], jf, 3000, 0.25, rec1, cnt1)
        torch.cuda.synchronize()
        assert int(cnt1[0]) >= 1 and all(torch.equal(x, y) for x, y in zip(first, outs))
        assert torch.equal(rec1, rec0) and torch.equal(cnt1, cnt0)
        assert 0 < plan.workspace_bytes - ws_new == other.workspace_bytes - ws_new < 4096
        ws1 = plan.workspace_bytes
        plan.align(*a, k, w, 10.0, *outs)
        rec2, cnt2 = new()
        plan.refine(*a, k, outs[0], 3000, 0.25, rec2, cnt2)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(first, outs))
        assert torch.equal(rec2, rec0) and torch.equal(cnt2, cnt0) and plan.workspace_bytes == ws1
    finally:
        plan.close()
        other.close()


class _Ptr:
    """A stand-in for a tensor argument: an address (0 = null) and a size that passes the binding's own checks."""

    def __init__(self, ptr, numel=1 << 40):
        self._ptr, self._n = ptr, numel

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n

    def element_size(self):
        return 1


def test_refused_calls_leave_outputs_untouched():
    import torch

    from ffsubsync_amd import _native
    from ffsubsync_amd import drift_refine as dref

    pr = FUZZ[0]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    with pytest.raises(ValueError):
        dref.refine_jumps_batch(db, [_drift_result(pr)], K, 0, 0.25)
    with pytest.raises(ValueError):
        dref.refine_jumps_batch(db, [_drift_result(pr)], 512, 300, 0.25)  # a path of another K
    with pytest.raises(ValueError):
        dref.refine_jumps_batch(db, [_drift_result(pr)] * 2, K, 300, 0.25)
    a = db.pair_arrays()
    dev = db.data.device
    mb = pr["o"].size
    offs = torch.from_numpy(pr["o"]).to(dev)
    jf = torch.from_numpy(pr["jf"]).to(dev)
    rec = torch.full((mb * _native.BREAK_REFINE_BYTES + 8,), 0xAB, dtype=torch.uint8, device=dev)
    cnt = torch.full((1,), -9, dtype=torch.int32, device=dev)
    before = [t.clone() for t in (offs, jf, rec, cnt)]
    zero = np.zeros(1, np.int64)
    plan = _native.SplitPlan(1, 1, 2, 1)
    try:
        ws0 = plan.workspace_bytes
        cases = [dict(radius=0), dict(radius=_native.REFINE_MAX_RADIUS + 1), dict(beta=-1.0), dict(beta=math.inf),
                 dict(rec=_Ptr(0)), dict(rec=rec[4:]), dict(cnt=_Ptr(0)), dict(cnt=_Ptr(cnt.data_ptr() + 2)),
                 dict(jf=_Ptr(0)), dict(offs=_Ptr(0, mb)), dict(k=300), dict(k=128), dict(sl=zero), dict(rl=zero)]
        for case in cases:
            v = dict(k=K, radius=300, beta=0.25, rec=rec, cnt=cnt, jf=jf, offs=offs, sl=a[5], rl=a[1])
            v.update(case)
            with pytest.raises(_native.NativeError) as ei:
                plan.drift_refine(a[0], v["rl"], a[2], a[3], a[4], v["sl"], a[6], a[7], v["k"], v["offs"], v["jf"],
                                  v["radius"], v["beta"], v["rec"], v["cnt"])
            assert ei.value.code == (-5 if "sl" in case or "rl" in case else -1), case  # FFS_E_EMPTY / FFS_E_INVALID
        empty = [x[:0] for x in a]
        plan.drift_refine(*empty, K, offs, jf, 300, 0.25, rec, cnt)  # n_pairs = 0: nothing to do, nothing written
        torch.cuda.synchronize()
        for x, y in zip(before, (offs, jf, rec, cnt)):
            assert torch.equal(x, y)
        assert plan.workspace_bytes == ws0  # the refine scratch is made by the first call that runs
        plan.drift_refine(*a, K, offs, jf, 300, math.nan, rec, cnt)
        torch.cuda.synchronize()
        assert plan.workspace_bytes > ws0 and int(cnt[0]) == len(drm.jumps_of(pr["jf"]))
    finally:
        plan.close()
    dref.clear_plan_cache()


@pytest.mark.parametrize("layout", ["poisoned", "shifted", "abutting"])
def test_hostile_layouts(layout):
    """tests/layout_cases.py's images: bit-packed vectors at the least alignment the header grants (4 bytes), 0xFF in
    every gap, guard and tail bit; the block offsets (4-byte aligned), jump flags (no alignment) and both outputs (8 / 4)
    in a 0xFF-filled buffer at the least residues.  Results equal the model; the inputs and every byte around the outputs
    are unchanged."""
    import torch

    import layout_cases as lc
    from ffsubsync_amd import _native

    probs = [FUZZ[i] for i in (0, 1, 3, 12, 13, 22)]  # first / last block, adjacent, every block, off either end, |o| > R
    vectors = [v for pr in probs for v in (pr["rb"], pr["sb"])]
    img = lc.build(vectors, lc.U1, layout).upload()
    n = len(probs)
    db = img.device_batch((n, 2), [[pr["r_lv"][0], pr["s_lv"][0]] for pr in probs],
                          [[pr["r_lv"][1], pr["s_lv"][1]] for pr in probs], _native.FFS_DTYPE_U1)
    offs, jumps = _rows(probs)
    max_b = offs.shape[1]
    # slots: block offsets, jump flags, records, counts
    can = lc.Canaries([offs.nbytes, jumps.nbytes, n * max_b * _native.BREAK_REFINE_BYTES, 4 * n], [4, 3, 8, 4])
    can.tensor(0).copy_(torch.from_numpy(offs.reshape(-1).view(np.uint8)))
    can.tensor(1).copy_(torch.from_numpy(jumps.reshape(-1)))
    plan = _native.SplitPlan(4, 1, 2, 1)
    try:
        for radius, beta in ((5000, 0.25), (100, math.nan)):
            plan.drift_refine(*db.pair_arrays(), K, can.tensor(0, torch.int32), can.tensor(1), radius, beta, can.tensor(2),
                              can.tensor(3, torch.int32))
            torch.cuda.synchronize()
            recs = can.tensor(2).cpu().numpy().view(_native.BREAK_REFINE_DTYPE).reshape(n, max_b)
            counts = can.tensor(3, torch.int32).cpu().numpy()
            for p, pr in enumerate(probs):
                want = _model(pr, radius, None if math.isnan(beta) else beta)
                m = int(counts[p])
                assert not _diff(recs[p, :m], want) and not recs[p, m:].tobytes().strip(b"\0"), (layout, p, radius)
            img.assert_inputs_untouched("drift_refine")
            can.assert_canaries_intact("drift_refine")
            assert np.array_equal(can.tensor(0).cpu().numpy(), offs.reshape(-1).view(np.uint8))
            assert np.array_equal(can.tensor(1).cpu().numpy(), jumps.reshape(-1))
    finally:
        plan.close()


def _host_bits(db, p, col):
    """Vector (p, col) of a bit-packed DeviceBatch as a bool host array."""
    from ffsubsync_amd import _native

    assert db.dtype == _native.FFS_DTYPE_U1
    n, o = int(db.lens[p, col]), int(db.offs[p, col])
    raw = db.data[o:o + (n + 31) // 32 * 4].cpu().numpy()
    return np.unpackbits(raw, bitorder="little")[:n] != 0


def _shift_samples(out_us, in_us, ratio, sample_rate=100):
    from ffsubsync_amd.split_align import _scaled_us

    return np.array([(o - _scaled_us(s, ratio)) * sample_rate / 1e6 for o, s in zip(out_us, in_us)])


def test_refined_cut_drift_sync_end_to_end():
    """The first four seeds of workloads/drift_cuts.py (one hour, full range, defaults) through refined_cut_drift_sync.
    The records are the model's on the device's own smooth offsets.  Over the four problems together: at least half of
    the cut-scene cues are found unmatched, the false unmatched are at most a quarter of the found, and no more matched
    cues are wrong (50 samples) than under smooth_cut_sync's mapping of the same solve.  The CPU models meet these on
    the same seeds (profiles/drift_refine_calibration.json, cues = the runs of ones of the subtitle vector: 63 of 75
    found, 1 false, wrong 5 -> 2)."""
    from ffsubsync_amd import cut_align as ca
    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs
    from ffsubsync_amd import drift_refine as dref
    from ffsubsync_amd import drift_smooth as ds
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import cuts, drift_cuts

    seeds = drift_cuts.seeds(4)
    probs = [drift_cuts.make_problem(s) for s in seeds]
    items = [(p.ref.astype(float), p.track) for p in probs]
    got = dref.refined_cut_drift_sync(items)
    k = drs.DEFAULT_BLOCK_SAMPLES
    db, best, _ = ca.solve_ratios_windowless(items, list(candidate_ratios()))
    chosen = db.select_candidates(best)
    fits = drs.smooth_align_range_batch(chosen)
    recs, counts = dref.refine_jumps_batch(chosen, fits, raw=True)
    tot = dict(cut=0, found=0, false=0, wrong=0, wrong_smooth=0)
    for p, (pr, g, f) in enumerate(zip(probs, got, fits)):
        assert g.ratio_index == pr.ratio_index == int(best[p])
        assert np.array_equal(g.smooth_offsets, f.smooth_offsets) and np.array_equal(g.block_jump, f.drift.block_jump)
        rb, sb = _host_bits(chosen, p, 0), _host_bits(chosen, p, 1)
        want = drm.refine(rb, sb, (chosen.lo[p, 0], chosen.hi[p, 0]), (chosen.lo[p, 1], chosen.hi[p, 1]), f.smooth_offsets,
                          f.drift.block_jump, k, dref.DEFAULT_RADIUS_SAMPLES, dref.DEFAULT_UNMATCHED_MARGIN)
        n = int(counts[p])
        assert n == len(g.breaks) == len(g.segments) - 1 >= 1
        assert not _diff(recs[p, :n], want), (seeds[p], _diff(recs[p, :n], want))
        assert [(b.block, b.t1, b.t2, b.flags) for b in g.breaks] == \
            [(int(r["block"]), int(r["t1"]), int(r["t2"]), int(r["flags"])) for r in want]
        assert np.array_equal(g.cue_unmatched, g.cue_segment == dref.UNMATCHED_PIECE)
        s_us = pr.track[0]
        x = cuts.cue_samples(pr.track, g.ratio)
        sc = drift_cuts.score_cues(pr, x, _shift_samples(g.cue_start_us, s_us, g.ratio), g.cue_unmatched)
        cs, _, _ = ds.map_cues_smooth(pr.track[0], pr.track[1], g.ratio, f, k)
        sc0 = drift_cuts.score_cues(pr, x, _shift_samples(cs, s_us, g.ratio), np.zeros(x.size, bool))
        print("seed %d: cut-scene cues %d, found %d, false %d, wrong %d (smooth_cut_sync's mapping: %d)"
              % (seeds[p], sc["cut_cues"], sc["found"], sc["false"], sc["wrong"], sc0["wrong"]))
        tot["cut"] += sc["cut_cues"]
        tot["found"] += sc["found"]
        tot["false"] += sc["false"]
        tot["wrong"] += sc["wrong"]
        tot["wrong_smooth"] += sc0["wrong"]
    print(tot)
    assert tot["cut"] >= 20
    assert 2 * tot["found"] >= tot["cut"], tot
    assert 4 * tot["false"] <= tot["found"], tot
    assert tot["wrong"] <= tot["wrong_smooth"], tot
    for m in (ca, dr, drs, dref):
        m.clear_plan_cache()


def test_refined_cut_drift_sync_on_a_clean_file_is_smooth_cut_sync():
    """One segment: every field of smooth_cut_sync's result, no breaks, no unmatched cue; and the plain variant against
    cut_drift_sync."""
    import dataclasses

    from ffsubsync_amd import drift_range as dr
    from ffsubsync_amd import drift_range_smooth as drs
    from ffsubsync_amd import drift_refine as dref
    from workloads import drift

    pr = drift.make_problem(3, duration_s=600.0, clean=True)
    items = [(pr.ref.astype(float), pr.track)]
    for smooth, base in ((True, drs.smooth_cut_sync), (False, dr.cut_drift_sync)):
        g, w = dref.refined_cut_drift_sync(items, smooth=smooth)[0], base(items)[0]
        assert len(w.segments) == 1
        for fl in dataclasses.fields(w):
            x, y = getattr(g, fl.name), getattr(w, fl.name)
            assert np.array_equal(x, y) if isinstance(y, np.ndarray) else repr(x) == repr(y), fl.name
        assert g.breaks == [] and not g.cue_unmatched.any() and len(g.cue_unmatched) == len(g.cue_start_us)
    for m in (dr, drs, dref):
        m.clear_plan_cache()


def test_refined_drift_sync_window_entry_point():
    """Two workloads/drift.py seeds with an inserted stretch, +-5 min: the jump's refined cut lies within one block of
    the insert's reference time mapped to candidate samples.  A seed without a break: smooth_sync's cue times."""
    from ffsubsync_amd import drift_refine as dref
    from ffsubsync_amd import drift_smooth as ds
    from workloads import drift

    k = ds.DEFAULT_BLOCK_SAMPLES
    probs = [drift.make_problem(s, duration_s=1800.0, insert_break=True) for s in (0, 1)]
    flat = drift.make_problem(2, duration_s=1800.0)
    items = [(p.ref.astype(float), p.track) for p in probs + [flat]]
    got = dref.refined_drift_sync(items, 300)
    for p, g in zip(probs, got):
        # the insert's place on the subtitle clock, in samples of the candidate the ratio solve chose
        at = drift._to_sub(p.break_ref_s, p.ratio, p.eps, p.offset_s, p.wobble_s, p.wobble_phase, p.period_s) * g.ratio * 100
        assert len(g.breaks) == len(g.segments) - 1 >= 1
        near = min(g.breaks, key=lambda b: abs(b.cut - at))
        print("seed %d: insert at candidate sample %.1f, refined %s" % (p.seed, at, near))
        assert abs(near.t1 - at) <= k and abs(near.t2 - at) <= k, (p.seed, at, near)
        assert np.array_equal(g.cue_unmatched, g.cue_segment == dref.UNMATCHED_PIECE)
    want = ds.smooth_sync(items[2:], 300)[0]
    assert len(want.segments) == 1 and got[2].breaks == []
    assert np.array_equal(got[2].cue_start_us, want.cue_start_us) and np.array_equal(got[2].cue_end_us, want.cue_end_us)
    plain = dref.refined_drift_sync(items[:1], 300, smooth=False)[0]
    assert [b.block for b in plain.breaks] == [b.block for b in got[0].breaks]
    ds.clear_plan_cache()
    dref.clear_plan_cache()
