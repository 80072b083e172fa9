"""Shuffled-cue significance on the device: ``ffs_surrogate_lists`` byte for byte and ``ffs_null_stats``
record for record against tests/surrogate_model.py, on hostile layouts (blocks at 8-byte alignment only, 0xFF in every
gap and behind every input sentinel, blocks right behind blocks); ``null_test_lists`` and ``null_sync`` end to end against
the model.  Expected values never come from a device run.  Need a real MI355X."""
import math

import numpy as np
import pytest

import surrogate_cases as cases
import surrogate_model as sm

pytestmark = pytest.mark.gpu
POISON_OUT, POISON_STATUS = 0xAB, 0x5A5A5A5A


class Call:
    """One ``ffs_surrogate_lists`` call on a hostile layout.  ``blocks``: the int32 words of every input list up to its
    sentinel (header included; the header's cap decides how many 0xFF entries follow the sentinel).  The input image puts
    every block at an address that is 8 but not 16 mod 16, with 0xFF in the gaps; the output image is POISON_OUT
    everywhere, vector v's K blocks of capacity n_bound + 1 + slack back to back, the next vector's 0, 8 or 24 bytes on."""

    def __init__(self, blocks, n_bound, seeds, k, block_units, slack=None):
        import torch

        self.torch, self.k, self.b = torch, int(k), int(block_units)
        self.blocks = [np.asarray(w, np.int32) for w in blocks]
        self.n_bound = np.asarray(n_bound, np.int32)
        self.seeds = np.asarray(seeds, np.uint32)
        nv = len(self.blocks)
        slack = [(0, 3, 1)[v % 3] for v in range(nv)] if slack is None else list(slack)
        in_bytes = [max(16 + 8 * max(int(w[3]), 1), w.size * 4) for w in self.blocks]  # the block the header's cap describes
        self.in_off, at = [], 8
        for nb in in_bytes:
            at = at if at % 16 == 8 else at + 8
            self.in_off.append(at)
            at += nb + 8 * (1 + len(self.in_off) % 2)
        self.in_host = np.full(at + 64, 0xFF, np.uint8)
        for w, o in zip(self.blocks, self.in_off):
            self.in_host[o:o + w.size * 4] = w.view(np.uint8)
        self.caps = (self.n_bound.astype(np.int64) + 1 + np.asarray(slack, np.int64))
        self.out_off, at = np.zeros(nv, np.int64), 8
        for v in range(nv):
            self.out_off[v] = at
            at += self.k * (16 + 8 * int(self.caps[v])) + (0, 8, 24)[v % 3]
        self.out_bytes = at + 40
        self.inp = torch.from_numpy(self.in_host.copy()).cuda()
        self.out = torch.full((self.out_bytes,), POISON_OUT, dtype=torch.uint8, device="cuda")
        self.status = torch.full((nv + 2,), POISON_STATUS, dtype=torch.int32, device="cuda")
        self.ptrs = np.array([self.inp.data_ptr() + o for o in self.in_off], np.uint64)
        assert self.inp.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def run(self):
        from ffsubsync_amd import _native

        _native.surrogate_lists(self.ptrs, self.n_bound, self.seeds, self.out_off, self.caps, self.k, self.b, self.out,
                                self.status)
        self.torch.cuda.synchronize()
        return self

    def want_block(self, v, s):
        w = self.blocks[v]
        n, length, cap_in = int(w[0]), int(w[2]), int(w[3])
        if sm.status(n, cap_in, int(self.n_bound[v])):
            return sm.empty_block(length, int(self.caps[v]))
        pos = w[4:4 + 2 * n:2].astype(np.int64)
        return sm.encode(sm.surrogate(pos, int(self.seeds[v]), s, self.b), length, int(self.caps[v]))

    def want_image(self):
        img = np.full(self.out_bytes, POISON_OUT, np.uint8)
        for v in range(len(self.blocks)):
            for s in range(self.k):
                w = self.want_block(v, s).view(np.uint8)
                o = int(self.out_off[v]) + s * (16 + 8 * int(self.caps[v]))
                img[o:o + w.size] = w
        return img

    def want_status(self):
        st = [sm.status(int(w[0]), int(w[3]), int(b)) for w, b in zip(self.blocks, self.n_bound)]
        return np.array(st + [POISON_STATUS] * 2, np.int32)

    def check(self):
        """Every byte of the output image (blocks, gaps, the entries behind every sentinel), every status word and the
        input image."""
        got, want = self.out.cpu().numpy(), self.want_image()
        if not np.array_equal(got, want):
            at = int(np.flatnonzero(got != want)[0])
            v = int(np.searchsorted(self.out_off, at, side="right")) - 1
            raise AssertionError("output image differs first at byte %d (vector %d, byte %d of its blocks)"
                                 % (at, v, at - int(self.out_off[max(v, 0)])))
        assert np.array_equal(self.status.cpu().numpy(), self.want_status())
        assert np.array_equal(self.inp.cpu().numpy(), self.in_host), "an input was written"

    def untouched(self):
        assert bool((self.out == POISON_OUT).all()) and bool((self.status == POISON_STATUS).all())
        assert np.array_equal(self.inp.cpu().numpy(), self.in_host)


def _block(pos, length, spare=0):
    """Input words of a valid list, its header's cap = n + 1 + spare."""
    return sm.encode(pos, length, len(pos) + 1 + spare)


def _mixed_lists(seed):
    """One list per entry of cases.UNITS plus the list without any run, in a shuffled order: the vectors of one call."""
    rng = np.random.RandomState(seed)
    lists = [cases.random_list(rng, u, kind=i % 4) for i, u in enumerate(cases.UNITS)]
    lists.append((np.zeros(0, np.int64), 17))  # m = 0
    order = rng.permutation(len(lists))
    return [lists[i] for i in order]


@pytest.mark.parametrize("block_units,k", [(1, 64), (2, 3), (7, 3), (64, 3), (8192, 1), (1, 1), (5000, 3)])
def test_lists_equal_the_model_byte_for_byte(block_units, k):
    lists = _mixed_lists(100 + block_units)
    rng = np.random.RandomState(k)
    blocks = [_block(p, n, spare=i % 3) for i, (p, n) in enumerate(lists)]
    bound = [p.size + (0, 2, 6)[i % 3] for i, (p, _) in enumerate(lists)]
    call = Call(blocks, bound, rng.randint(0, 2 ** 32, len(lists), dtype=np.uint64), k, block_units).run()
    call.check()
    assert not call.want_status()[:-2].any()


@pytest.mark.parametrize("n_vec,block_units,k", [(17, 1, 3), (41, 7, 2), (300, 2, 1)])
def test_many_vectors_of_mixed_sizes_with_bad_lists_among_them(n_vec, block_units, k):
    """Calls of many vectors: every descriptor of the uploaded table is read by its own workgroups (each vector its own
    size, seed, bound, capacity and offset), with an odd, a truncated and an over-bound list among the good ones."""
    rng = np.random.RandomState(n_vec)
    sizes = [(0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 31, 9)[i % 13] + (i // 13) for i in range(n_vec)]
    lists = [cases.random_list(rng, u, kind=i % 4) for i, u in enumerate(sizes)]
    blocks = [_block(p, n, spare=i % 3).copy() for i, (p, n) in enumerate(lists)]
    bound = [p.size + (0, 2, 6)[i % 3] for i, (p, _) in enumerate(lists)]
    blocks[4][0] = 127  # 63 units: an odd header
    blocks[n_vec - 1][3] = blocks[n_vec - 1][0]  # the last vector: n >= cap
    bound[9] -= 2  # 257 units: above its bound
    call = Call(blocks, bound, rng.randint(0, 2 ** 32, n_vec, dtype=np.uint64), k, block_units).run()
    bad = {4: sm.BAD_ODD, n_vec - 1: sm.BAD_TRUNCATED, 9: sm.BAD_BOUND}
    assert list(call.want_status()[:n_vec]) == [bad.get(v, 0) for v in range(n_vec)]
    call.check()


def test_the_short_last_block_first_in_the_middle_and_last():
    rng = np.random.RandomState(8)
    blocks, bound, seeds = [], [], []
    for units, b in ((65, 7), (257, 7), (15, 7)):
        pos, length = cases.random_list(rng, units)
        seed = cases.seed_placing_short_block(units, b)
        nb = (units + b - 1) // b
        assert [cases.short_block_place(seed, s, units, b) for s in (0, 1)] == [0, nb - 1]
        assert 0 < cases.short_block_place(seed, 2, units, b) < nb - 1
        blocks.append(_block(pos, length))
        bound.append(pos.size)
        seeds.append(seed)
    Call(blocks, bound, seeds, 3, 7).run().check()


def test_the_unit_limit_with_seeds_at_the_ends_of_uint32():
    """U = 8192, B = 1 (the full 8192-key sort, 96 KiB of LDS) with seeds 0 and 2^32 - 1 and the last surrogate index
    the call allows: K = 4096 on a two-unit list beside it.  (Two blocks of one surrogate never share a key -- fmix32 is
    a bijection, tests/test_surrogate_model_host.py -- so no input exercises the index half of the (key, b) order.)"""
    rng = np.random.RandomState(21)
    pos, length = cases.random_list(rng, 8192, kind=3)
    Call([_block(pos, length), _block(pos, length)], [pos.size, pos.size], [0, 0xFFFFFFFF], 2, 1).run().check()
    small, n = cases.random_list(rng, 2)
    Call([_block(small, n)], [small.size], [12345], 4096, 1).run().check()


def test_properties_of_the_device_output():
    """On the device's own output: every surrogate expands (``ffs_runs_to_bits``) to the input's popcount and length, and
    the sorted multiset of (run, following silence) pairs is the input's."""
    import torch
    from ffsubsync_amd import _native

    rng = np.random.RandomState(4)
    pos, length = cases.random_list(rng, 257, kind=2)
    v = sm.expand(pos, length)
    pairs = lambda p: sorted(zip((p[1:-2:2] - p[0:-2:2]).tolist(), (p[2::2] - p[1:-2:2]).tolist()))
    for b in (1, 7):
        call = Call([_block(pos, length)], [pos.size], [99], 3, b, slack=[0]).run()
        distinct = set()
        for s in range(3):
            o = int(call.out_off[0]) + s * (16 + 8 * int(call.caps[0]))
            block = call.out[o:o + 16 + 8 * int(call.caps[0])].clone()  # (an aligned copy for the int32 view)
            words = _native.runs_to_bits(block.view(torch.int32), length)
            bits = _native.unpack_bits(words, length).cpu().numpy()
            assert bits.size == length and int(bits.sum()) == int(v.sum())
            got_pos, got_before, ones = _native.runs_list_host(block.view(torch.int32))
            assert ones == int(v.sum()) and pairs(got_pos.astype(np.int64)) == pairs(pos)
            assert np.array_equal(sm.boundaries(bits), got_pos) and np.array_equal(np.concatenate([[0], np.cumsum(bits)])[got_pos], got_before)
            distinct.add(got_pos.tobytes())
        assert len(distinct) == 3 and pos.tobytes() not in distinct


def test_bad_lists_inside_a_call_of_good_ones():
    rng = np.random.RandomState(6)
    good = [cases.random_list(rng, u) for u in (64, 3, 300, 65)]
    blocks = [_block(p, n, spare=2) for p, n in good]
    bound = [p.size for p, _ in good]
    odd = _block(*cases.random_list(rng, 9)).copy()
    odd[0] = 5  # an odd header
    trunc = _block(*cases.random_list(rng, 9)).copy()
    trunc[3] = trunc[0]  # n >= cap
    above = _block(*cases.random_list(rng, 9))  # n = 20 against a bound of 18
    big_pos, big_len = cases.random_list(rng, 8193)  # one unit above the limit
    negative = _block(*cases.random_list(rng, 4)).copy()
    negative[0] = -2
    blocks = [blocks[0], odd, blocks[1], trunc, above, blocks[2], _block(big_pos, big_len), negative, blocks[3]]
    bound = [bound[0], 20, bound[1], 20, 18, bound[2], big_pos.size, 10, bound[3]]
    call = Call(blocks, bound, np.arange(9) * 1000003 + 7, 3, 2).run()
    assert list(call.want_status()[:9]) == [0, sm.BAD_ODD, 0, sm.BAD_TRUNCATED, sm.BAD_BOUND, 0, sm.BAD_UNITS,
                                            sm.BAD_TRUNCATED, 0]
    call.check()


def test_refusals_leave_outputs_and_status_untouched():
    from ffsubsync_amd import _native

    rng = np.random.RandomState(12)
    lists = [cases.random_list(rng, u) for u in (5, 64)]
    call = Call([_block(p, n) for p, n in lists], [p.size for p, _ in lists], [1, 2], 3, 1, slack=[0, 0])
    lib, st = _native.load(), _native.current_stream_ptr(call.torch)
    i64 = lambda a: np.ascontiguousarray(a, np.int64)

    def raw(ptrs=call.ptrs, bound=call.n_bound, seeds=call.seeds, off=call.out_off, caps=call.caps, n=2, k=3, b=1,
            out=call.out.data_ptr(), nbytes=call.out_bytes, status=call.status.data_ptr()):
        arrs = [None if a is None else np.ascontiguousarray(a) for a in (ptrs, bound, seeds, None if off is None else i64(off),
                                                                         None if caps is None else i64(caps))]
        return lib.ffs_surrogate_lists(*[None if a is None else a.ctypes.data for a in arrs], n, k, b, out, nbytes, status, st)

    tight = int(call.out_off[1]) + 3 * (16 + 8 * int(call.caps[1]))  # where the last block ends
    bad = [dict(k=0), dict(k=4097), dict(b=0), dict(b=8193), dict(n=-1), dict(nbytes=-8), dict(ptrs=None), dict(bound=None),
           dict(seeds=None), dict(off=None), dict(caps=None), dict(out=None), dict(status=None),
           dict(out=call.out.data_ptr() + 4), dict(status=call.status.data_ptr() + 2),
           dict(ptrs=call.ptrs + np.uint64(4)), dict(ptrs=np.array([call.ptrs[0], 0], np.uint64)),
           dict(bound=np.array([-1, 10], np.int32)), dict(off=call.out_off + 4), dict(off=np.array([8, -8])),
           dict(caps=call.caps - np.array([0, 1])), dict(nbytes=tight - 8), dict(off=call.out_off + np.array([0, 48]), nbytes=tight + 40)]
    for kw in bad:
        assert raw(**kw) == -1, kw
        assert _native.load().ffs_last_error().decode().startswith("ffs_surrogate_lists"), kw
    call.torch.cuda.synchronize()
    call.untouched()
    assert raw(n=0) == 0 and raw(nbytes=tight) == 0  # nothing to do; and the exact fit is taken
    call.torch.cuda.synchronize()
    call.check()


# ---- ffs_null_stats ---------------------------------------------------------------------------------------------------
STATS_K = [1, 2, 63, 64, 65, 257, 4096]


def _stats_files(k):
    from ffsubsync_amd import _native

    rng = np.random.RandomState(k)

    def blank():
        rec = np.zeros(k + 1, _native.CAND_RESULT_DTYPE)
        rec["score"] = rng.randint(0, 40, k + 1) * 0.37 - 2.0 + 1e4
        rec["offset"] = rng.randint(-6000, 6001, k + 1)
        rec["flags"][rng.rand(k + 1) < 0.3] |= _native.FLAG_DIRECT  # a flag the reduction ignores
        return rec

    files = [blank()]
    ties = blank()  # nulls equal to the real score: n_ge against n_gt
    ties["score"][1:1 + (k + 1) // 2] = ties["score"][0]
    files.append(ties)
    flat = blank()  # all equal: FLAT, std exactly 0
    flat["score"][1:] = 0.1
    files.append(flat)
    holes = blank()  # non-finite and EMPTY_WINDOW records skipped
    pick = rng.rand(k + 1)
    holes["score"][(pick < 0.15)] = -np.inf
    holes["score"][(pick >= 0.15) & (pick < 0.25)] = np.nan
    holes["score"][(pick >= 0.25) & (pick < 0.3)] = np.inf
    holes["flags"][(pick >= 0.3) & (pick < 0.45)] |= _native.FLAG_EMPTY_WINDOW
    holes["score"][0], holes["flags"][0] = 10001.5, 0
    files.append(holes)
    none = blank()  # no usable null, one of them ambiguous
    none["score"][1:] = -np.inf
    none["flags"][k] |= _native.FLAG_AMBIGUOUS
    files.append(none)
    unreal = blank()  # an unusable real record
    unreal["flags"][0] |= _native.FLAG_EMPTY_WINDOW
    unreal["score"][0] = -np.inf
    files.append(unreal)
    nan_real = blank()
    nan_real["score"][0] = np.nan
    files.append(nan_real)
    amb = blank()  # AMBIGUOUS carried: on the real record here, on the last null above
    amb["flags"][0] |= _native.FLAG_AMBIGUOUS
    files.append(amb)
    big = blank()  # a large mean over a small spread: the two-pass moments
    big["score"] = 3e5 + rng.rand(k + 1)
    files.append(big)
    return files


def _same_bits(a, b):
    return np.array([a], np.float64).tobytes() == np.array([b], np.float64).tobytes()


@pytest.mark.parametrize("k", STATS_K)
def test_null_stats_equal_the_model(k):
    import torch
    from ffsubsync_amd import _native, surrogate

    files = _stats_files(k)
    host = np.concatenate(files + [np.zeros(1, files[0].dtype)])
    table = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    out = torch.full((len(files) * _native.NULL_RESULT_BYTES + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    _native.null_stats(table, len(files), k, out=out[8:])
    raw = out.cpu().numpy()
    assert (raw[:8] == 0xAB).all() and (raw[8 + len(files) * _native.NULL_RESULT_BYTES:] == 0xAB).all()
    assert np.array_equal(table.cpu().numpy(), host.view(np.uint8))  # records are read, never written
    got = raw[8:8 + len(files) * _native.NULL_RESULT_BYTES].view(_native.NULL_RESULT_DTYPE)
    assert np.array_equal(surrogate.null_stats(table, len(files), k).view(np.uint8), got.view(np.uint8))
    for f, (rec, g) in enumerate(zip(files, got)):
        want = sm.stats(rec["score"], rec["flags"])
        for name in ("n_null", "n_ge", "n_gt", "flags"):
            assert int(g[name]) == want[name], (f, name, int(g[name]), want[name])
        for name in ("real_score", "null_min", "null_max"):
            assert _same_bits(float(g[name]), want[name]), (f, name, float(g[name]), want[name])
        # fixed-order fp64 sums of at most 4096 terms against numpy's pairwise sums: K 2^-53 ~ 4.6e-13 relative
        for name in ("null_mean", "null_std"):
            assert math.isclose(float(g[name]), want[name], rel_tol=1e-12, abs_tol=0.0), (f, name, float(g[name]), want[name])
        if want["flags"] & sm.FLAT:
            assert float(g["null_std"]) == 0.0
    flags = [int(g["flags"]) for g in got]
    assert flags[2] == sm.FLAT and flags[4] == sm.FLAT | sm.EMPTY | sm.AMBIGUOUS and flags[5] & sm.EMPTY and flags[6] & sm.EMPTY
    assert flags[7] & sm.AMBIGUOUS and int(got[1]["n_ge"]) > int(got[1]["n_gt"])


def test_null_stats_refusals_leave_the_outputs_untouched():
    import torch
    from ffsubsync_amd import _native

    files = _stats_files(3)
    table = torch.from_numpy(np.concatenate(files).view(np.uint8).copy()).cuda()
    out = torch.full((len(files) * _native.NULL_RESULT_BYTES + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    lib, st = _native.load(), _native.current_stream_ptr(torch)
    for args in ((table.data_ptr(), -1, 3, out.data_ptr()), (table.data_ptr(), 2, 0, out.data_ptr()),
                 (table.data_ptr(), 2, 4097, out.data_ptr()), (None, 2, 3, out.data_ptr()), (table.data_ptr(), 2, 3, None),
                 (table.data_ptr() + 4, 2, 3, out.data_ptr()), (table.data_ptr(), 2, 3, out.data_ptr() + 4)):
        assert lib.ffs_null_stats(*args, st) == -1, args
        assert lib.ffs_last_error().decode().startswith("ffs_null_stats")
    assert lib.ffs_null_stats(table.data_ptr(), 0, 3, out.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())


# ---- end to end --------------------------------------------------------------------------------------------------------
E2E = (0, 1, 6, 7)  # problems of cases.sync_problems(): two matched, two wrong
_memo = {}


def _device_lists():
    """The four E2E problems as device-resident lists: the reference through ``ffs_runs_from_bits``, the track rasterised
    by the CPU oracle at the ratio the model's seven-ratio solve chose."""
    if "lists" not in _memo:
        import torch
        from ffsubsync_amd import _native, surrogate
        from oracle import raster_oracle as ro

        keep, rows = [], []
        for i in E2E:
            ref, track = cases.sync_problems()[i]
            model = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
            sub = (ro.rasterize(track[0], track[1], track[2], model["ratio"], 100, 0) > 0).astype(np.uint8)
            blocks = []
            for v in (ref != 0, sub):
                packed = np.packbits(v, bitorder="little").tobytes().ljust((v.size + 31) // 32 * 4, b"\0")
                words = torch.from_numpy(np.frombuffer(packed, np.int32).copy()).cuda()
                n = sm.boundaries(v).size
                blocks.append((_native.runs_from_bits(words, v.size, cap=n + 2), n, v.size))
            keep.append(blocks)
            rows.append((blocks[0][0].data_ptr(), blocks[0][2], blocks[0][1], blocks[1][0].data_ptr(), blocks[1][2], blocks[1][1],
                         min(1.0 / model["ratio"], 1.0), sm.file_seed(cases.SEED, i)))
        torch.cuda.synchronize()
        _memo["lists"] = (keep, [np.array(c) for c in zip(*rows)])
    return _memo["lists"][1]


def _null_test(sel=slice(None), **kw):
    from ffsubsync_amd import surrogate

    rp, rl, rb, sp, sl, sb, hi, seeds = [c[sel] for c in _device_lists()]
    return surrogate.null_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, cases.W, cases.K, 1,
                                     sub_hi=hi, seeds=seeds, **kw)


def _check_record(rec, want):
    for name in ("n_null", "n_ge", "n_gt", "flags"):
        assert int(rec[name]) == want[name], (name, int(rec[name]), want[name])
    for name in ("real_score", "null_min", "null_max"):
        assert float(rec[name]) == want[name], (name, float(rec[name]), want[name])
    for name in ("null_mean", "null_std"):
        assert math.isclose(float(rec[name]), want[name], rel_tol=1e-12), (name, float(rec[name]), want[name])


def test_null_test_lists_equal_the_model():
    from ffsubsync_amd import surrogate

    test = _null_test()
    assert not test.status.any() and test.stats["careful_files"] == 0 and test.stats["chunks"] == 1
    solves = test.solves()
    assert solves.shape == (len(E2E), cases.K + 1)
    for row, i in enumerate(E2E):
        model = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
        assert np.array_equal(solves[row]["score"], model["scores"]), i  # every null score, as a value
        assert not solves[row]["flags"].any() and int(solves[row][0]["offset"]) == model["offset"]
        _check_record(test.records[row], model["record"])


def test_a_file_alone_equals_the_file_inside_a_batch_and_chunks_change_nothing():
    whole = _null_test()
    for row in (0, 3):
        alone = _null_test(slice(row, row + 1))
        assert alone.records.tobytes() == whole.records[row:row + 1].tobytes()
        assert alone.solves().tobytes() == whole.solves()[row:row + 1].tobytes()
    parts = _null_test(budget_bytes=1)  # one file per chunk
    assert parts.stats["chunks"] == len(E2E)
    assert parts.records.tobytes() == whole.records.tobytes() and parts.solves().tobytes() == whole.solves().tobytes()


def test_two_calls_queued_on_one_stream_equal_the_calls_made_apart():
    """``raw``: nothing is read back, so two whole null tests (lists, solves, reduction) queue behind each other on a
    side stream with no synchronisation in between."""
    import torch

    apart = [_null_test(slice(0, 2)), _null_test(slice(2, 4))]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        first = _null_test(slice(0, 2), raw=True)
        second = _null_test(slice(2, 4), raw=True)
    stream.synchronize()
    from ffsubsync_amd import _native

    for got, want in zip((first, second), apart):
        recs = got.records.cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:2]
        assert recs.tobytes() == want.records.tobytes()
        assert got.table.cpu().numpy().tobytes() == want.table.cpu().numpy().tobytes()
        assert not got.status.cpu().numpy().any()


def test_null_sync_equals_the_model_and_separates_the_classes():
    from ffsubsync_amd import _native, surrogate

    problems, kinds = cases.sync_problems(), cases.sync_kinds()
    got = surrogate.null_sync(problems, 60)
    assert len(got) == len(problems) == 12
    for i, (r, kind) in enumerate(zip(got, kinds)):
        model = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        _check_record(vars(r.null), model["record"])
        assert math.isclose(r.z, model["z"], rel_tol=1e-9) and r.p == model["p"]
        assert r.trusted == model["trusted"] == (kind == "matched"), (i, kind, r.z, r.null.n_ge)
        assert [x.split(" ")[0] for x in r.reasons] == [x.split(" ")[0] for x in model["reasons"]]
        if kind == "matched":
            assert r.null.n_ge == 0 and r.reasons == []
        else:
            assert r.reasons


def test_many_files_in_one_chunk_equal_the_files_solved_alone():
    """20 files in one ``ffs_surrogate_lists`` / ``align_batch`` / ``ffs_null_stats`` chunk (the four E2E pairs five
    times over, every copy with its own seed) against the same files solved one call each; the copies that keep the E2E
    seed also against the model."""
    from ffsubsync_amd import surrogate

    cols = _device_lists()
    rows = np.arange(20) % len(E2E)
    rp, rl, rb, sp, sl, sb, hi, seeds = [c[rows] for c in cols]
    seeds = np.array([int(s) if j < len(E2E) else sm.file_seed(1000 + j, 0) for j, s in enumerate(seeds)], np.int64)
    k = 16
    run = lambda sel: surrogate.null_test_lists(rp[sel].astype(np.uint64), rl[sel], rb[sel], sp[sel].astype(np.uint64), sl[sel],
                                                sb[sel], cases.W, k, 1, sub_hi=hi[sel], seeds=seeds[sel])
    whole = run(slice(None))
    assert whole.stats["chunks"] == 1 and not whole.status.any() and whole.solves().shape == (20, k + 1)
    for j in range(20):
        alone = run(slice(j, j + 1))
        assert alone.records.tobytes() == whole.records[j:j + 1].tobytes(), j
        assert alone.solves().tobytes() == whole.solves()[j:j + 1].tobytes(), j
    for row, i in enumerate(E2E):  # surrogate s does not depend on K: the model's first k nulls
        model = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
        assert np.array_equal(whole.solves()[row]["score"], model["scores"][:k + 1]), i
    assert len({whole.solves()[j]["score"].tobytes() for j in range(20)}) == 20  # every seed its own null


def test_the_careful_path_gives_the_fast_path_s_scores():
    """``surrogate._careful`` (the redo of an AMBIGUOUS file: surrogates expanded and solved pair by pair through
    ``solve_pairs``) on one matched and one wrong E2E file: its K + 1 scores are the rows of the fast path's table."""
    from ffsubsync_amd import surrogate

    fast = _null_test().solves()
    rp, rl, rb, sp, sl, sb, hi, seeds = _device_lists()
    for row in (0, 2):
        recs = surrogate._careful((int(rp[row]), int(rb[row]), int(rl[row]), 0.0, 1.0),
                                  (int(sp[row]), int(sb[row]), int(sl[row]), 0.0, float(hi[row])), int(seeds[row]), cases.K, 1,
                                  cases.W)
        assert recs.dtype == fast.dtype and recs.shape == (cases.K + 1,)
        assert np.array_equal(recs["score"], fast[row]["score"]), row
        assert int(recs[0]["offset"]) == int(fast[row][0]["offset"])
