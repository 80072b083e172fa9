"""Half-sample stability on the device: ``ffs_subsample_lists`` byte for byte and ``ffs_offset_stats`` bit
for bit against tests/stability_model.py, on hostile layouts (blocks at 8-byte alignment only, 0xFF in every gap and
behind every sentinel, blocks right behind blocks); ``stability_test_lists`` and ``stable_sync`` end to end against the
model.  Expected values never come from a device run.  Need a real MI355X."""
import numpy as np
import pytest

import stability_cases as sc
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm

pytestmark = pytest.mark.gpu
POISON, POISON_STATUS = 0xFF, 0x5A5A5A5A
RUNS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16383)


class Call:
    """One ``ffs_subsample_lists`` call on a hostile layout.  ``blocks``: the int32 words of every input list up to its
    sentinel (header included; the header's cap decides how many 0xFF entries follow the sentinel).  The input image puts
    every block at an address that is 8 but not 16 mod 16, with 0xFF in the gaps; the output image is 0xFF everywhere,
    vector v's K blocks of capacity n_bound + 1 + slack back to back, the next vector's 0, 8 or 24 bytes on."""

    def __init__(self, blocks, n_bound, seeds, k, block_runs, slack=None):
        import torch

        self.torch, self.k, self.b = torch, int(k), int(block_runs)
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
        self.caps = self.n_bound.astype(np.int64) + 1 + np.asarray(slack, np.int64)
        self.out_off, at = np.zeros(nv, np.int64), 8
        for v in range(nv):
            self.out_off[v] = at
            at += self.k * (16 + 8 * int(self.caps[v])) + (0, 8, 24)[v % 3]
        self.out_bytes = at + 40
        self.inp = torch.from_numpy(self.in_host.copy()).cuda()
        self.out = torch.full((self.out_bytes,), POISON, dtype=torch.uint8, device="cuda")
        self.status = torch.full((nv + 2,), POISON_STATUS, dtype=torch.int32, device="cuda")
        self.ptrs = np.array([self.inp.data_ptr() + o for o in self.in_off], np.uint64)
        assert self.inp.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0

    def run(self):
        from ffsubsync_amd import _native

        _native.subsample_lists(self.ptrs, self.n_bound, self.seeds, self.out_off, self.caps, self.k, self.b, self.out,
                                self.status)
        self.torch.cuda.synchronize()
        return self

    def input_pos(self, v):
        w = self.blocks[v]
        return w[4:4 + 2 * int(w[0]):2].astype(np.int64)

    def want_pos(self, v, s):
        return stm.subsample(self.input_pos(v), int(self.seeds[v]), s, self.b)

    def want_block(self, v, s):
        w = self.blocks[v]
        n, length, cap_in = int(w[0]), int(w[2]), int(w[3])
        if stm.status(n, cap_in, int(self.n_bound[v])):
            return stm.empty_block(length, int(self.caps[v]))
        return stm.encode(self.want_pos(v, s), length, int(self.caps[v]))

    def block_at(self, v, s):
        return int(self.out_off[v]) + s * (16 + 8 * int(self.caps[v]))

    def want_image(self):
        img = np.full(self.out_bytes, POISON, np.uint8)
        for v in range(len(self.blocks)):
            for s in range(self.k):
                w = self.want_block(v, s).view(np.uint8)
                img[self.block_at(v, s):self.block_at(v, s) + w.size] = w
        return img

    def want_status(self):
        st = [stm.status(int(w[0]), int(w[3]), int(b)) for w, b in zip(self.blocks, self.n_bound)]
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
        assert bool((self.out == POISON).all()) and bool((self.status == POISON_STATUS).all())
        assert np.array_equal(self.inp.cpu().numpy(), self.in_host)


def _list(rng, runs, kind=0):
    """(pos, len) of a valid list with ``runs`` runs."""
    return cases.random_list(rng, runs - 1, kind) if runs else (np.zeros(0, np.int64), 17)


def _block(pos, length, spare=0):
    """Input words of a valid list, its header's cap = n + 1 + spare."""
    return sm.encode(pos, length, len(pos) + 1 + spare)


def _mixed_lists(seed):
    """One list per entry of RUNS, in a shuffled order: the vectors of one call."""
    rng = np.random.RandomState(seed)
    lists = [_list(rng, m, kind=i % 4) for i, m in enumerate(RUNS)]
    return [lists[i] for i in rng.permutation(len(lists))]


@pytest.mark.parametrize("block_runs,k", [(1, 64), (2, 3), (7, 65), (64, 2), (16383, 3), (1 << 24, 2), (1, 1)])
def test_lists_equal_the_model_byte_for_byte(block_runs, k):
    lists = _mixed_lists(100 + block_runs % 1000)
    rng = np.random.RandomState(k)
    blocks = [_block(p, n, spare=i % 3) for i, (p, n) in enumerate(lists)]
    bound = [p.size + (0, 2, 6)[i % 3] for i, (p, _) in enumerate(lists)]
    call = Call(blocks, bound, rng.randint(0, 2 ** 32, len(lists), dtype=np.uint64), k, block_runs).run()
    call.check()
    assert not call.want_status()[:-2].any()
    if block_runs >= max(RUNS) and k >= 2:  # one block: a half-sample that keeps nothing beside one that keeps everything
        for v, (p, _) in enumerate(lists):
            assert sorted(call.want_pos(v, s).size for s in (0, 1)) == [0, p.size]


def test_the_largest_k_and_seeds_at_the_ends_of_uint32():
    rng = np.random.RandomState(21)
    big, small = _list(rng, 16383, kind=3), _list(rng, 1025, kind=1)
    Call([_block(*big), _block(*big), _block(*small), _block(*small)], [big[0].size, big[0].size, small[0].size, small[0].size],
         [0, 0xFFFFFFFF, 0xFFFFFFFF, 0], 3, 7).run().check()
    few = _list(rng, 3)
    Call([_block(*few), _block(*_list(rng, 65))], [few[0].size, 130], [12345, 0xFFFFFFFF], 4096, 2).run().check()


def test_the_short_last_block_kept_and_dropped():
    """65 runs in blocks of 7: block 9 holds two runs.  Of every pair one member keeps it and one drops it; over the first
    pairs either member does."""
    rng = np.random.RandomState(8)
    pos, length = _list(rng, 65)
    call = Call([_block(pos, length)], [pos.size], [3], 16, 7, slack=[0]).run()
    kept_by_even = set()
    for j in range(8):
        last = [bool(stm.keep_mask(3, 2 * j + i, 10)[9]) for i in (0, 1)]
        assert sorted(last) == [False, True]
        kept_by_even.add(last[0])
        for i in (0, 1):
            assert (int(pos[-1]) in call.want_pos(0, 2 * j + i).tolist()) == last[i]
    assert kept_by_even == {False, True}
    call.check()


@pytest.mark.parametrize("n_vec,block_runs,k", [(1, 1, 3), (17, 1, 3), (41, 7, 2), (300, 2, 1)])
def test_many_vectors_of_mixed_sizes_with_bad_lists_among_them(n_vec, block_runs, k):
    """Calls of many vectors: every descriptor of the uploaded table is read by its own workgroups (each vector its own
    size, seed, bound, capacity and offset), with an odd, a truncated, an over-bound and a negative list among the good
    ones: their half-samples are empty lists of the same length, their neighbours are what the model says."""
    rng = np.random.RandomState(n_vec)
    sizes = [(0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 31, 9)[i % 13] + (i // 13) for i in range(n_vec)]
    lists = [_list(rng, m, kind=i % 4) for i, m in enumerate(sizes)]
    blocks = [_block(p, n, spare=i % 3).copy() for i, (p, n) in enumerate(lists)]
    bound = [p.size + (0, 2, 6)[i % 3] for i, (p, _) in enumerate(lists)]
    bad = {}
    if n_vec > 12:
        blocks[4][0] = 125  # 63 runs: an odd header
        blocks[n_vec - 1][3] = blocks[n_vec - 1][0]  # the last vector: n >= cap
        bound[9] -= 2  # 257 runs: above its bound
        blocks[12][0] = -2  # negative
        bad = {4: stm.BAD_ODD, n_vec - 1: stm.BAD_TRUNCATED, 9: stm.BAD_BOUND, 12: stm.BAD_TRUNCATED}
    call = Call(blocks, bound, rng.randint(0, 2 ** 32, n_vec, dtype=np.uint64), k, block_runs).run()
    assert list(call.want_status()[:n_vec]) == [bad.get(v, 0) for v in range(n_vec)]
    call.check()


def test_properties_of_the_device_output():
    """On the device's own output: every half-sample round-trips through ``ffs_runs_to_bits`` with exact ones_before, and
    the members of a pair are disjoint and together the input."""
    import torch
    from ffsubsync_amd import _native

    rng = np.random.RandomState(4)
    pos, length = _list(rng, 257, kind=2)
    v = sm.expand(pos, length)
    for b in (1, 7):
        call = Call([_block(pos, length)], [pos.size], [99], 5, b, slack=[0]).run()
        halves = []
        for s in range(5):
            o = call.block_at(0, s)
            block = call.out[o:o + 16 + 8 * int(call.caps[0])].clone()  # (an aligned copy for the int32 view)
            got_pos, got_before, ones = _native.runs_list_host(block.view(torch.int32))
            words = _native.runs_to_bits(block.view(torch.int32), length)
            bits = _native.unpack_bits(words, length).cpu().numpy().astype(np.int64)
            assert bits.size == length and int(bits.sum()) == ones
            assert np.array_equal(sm.boundaries(bits), got_pos) and np.array_equal(np.concatenate([[0], np.cumsum(bits)])[got_pos], got_before)
            assert 0 < got_pos.size < pos.size
            halves.append(bits)
        for j in (0, 1):
            assert not (halves[2 * j] & halves[2 * j + 1]).any() and np.array_equal(halves[2 * j] + halves[2 * j + 1], v)
        assert not np.array_equal(halves[0], halves[2]) and not np.array_equal(halves[0], halves[4])


def test_refusals_leave_outputs_and_status_untouched():
    from ffsubsync_amd import _native

    rng = np.random.RandomState(12)
    lists = [_list(rng, m) for m in (6, 65)]
    call = Call([_block(p, n) for p, n in lists], [p.size for p, _ in lists], [1, 2], 3, 1, slack=[0, 0])
    lib, st = _native.load(), _native.current_stream_ptr(call.torch)
    i64 = lambda a: np.ascontiguousarray(a, np.int64)

    def raw(ptrs=call.ptrs, bound=call.n_bound, seeds=call.seeds, off=call.out_off, caps=call.caps, n=2, k=3, b=1,
            out=call.out.data_ptr(), nbytes=call.out_bytes, status=call.status.data_ptr()):
        arrs = [None if a is None else np.ascontiguousarray(a) for a in (ptrs, bound, seeds, None if off is None else i64(off),
                                                                         None if caps is None else i64(caps))]
        return lib.ffs_subsample_lists(*[None if a is None else a.ctypes.data for a in arrs], n, k, b, out, nbytes, status, st)

    tight = int(call.out_off[1]) + 3 * (16 + 8 * int(call.caps[1]))  # where the last block ends
    bad = [dict(k=0), dict(k=4097), dict(b=0), dict(b=(1 << 24) + 1), dict(n=-1), dict(nbytes=-8), dict(ptrs=None), dict(bound=None),
           dict(seeds=None), dict(off=None), dict(caps=None), dict(out=None), dict(status=None),
           dict(out=call.out.data_ptr() + 4), dict(status=call.status.data_ptr() + 2),
           dict(ptrs=call.ptrs + np.uint64(4)), dict(ptrs=np.array([call.ptrs[0], 0], np.uint64)),
           dict(bound=np.array([-1, 10], np.int32)), dict(off=call.out_off + 4), dict(off=np.array([8, -8])),
           dict(caps=call.caps - np.array([0, 1])), dict(caps=np.array([call.caps[0], 1 << 28])), dict(nbytes=tight - 8),
           dict(off=call.out_off + np.array([0, 48]), nbytes=tight + 40)]
    for kw in bad:
        assert raw(**kw) == -1, kw
        assert lib.ffs_last_error().decode().startswith("ffs_subsample_lists: "), kw
    call.torch.cuda.synchronize()
    call.untouched()
    assert raw(n=0) == 0
    call.torch.cuda.synchronize()
    call.untouched()
    assert raw(nbytes=tight) == 0  # the exact fit is taken
    call.torch.cuda.synchronize()
    call.check()


# ---- ffs_offset_stats --------------------------------------------------------------------------------------------------
STATS_K = [1, 2, 3, 63, 64, 65, 257, 4096]
STATS_TOL = {1: 0, 2: 0, 3: 5, 63: 5, 64: 40, 65: 1 << 41, 257: 3, 4096: 100}


def _stats_files(k):
    from ffsubsync_amd import _native

    rng = np.random.RandomState(k)

    def blank(spread=6):
        rec = np.zeros(k + 1, _native.CAND_RESULT_DTYPE)
        rec["score"] = rng.randint(0, 40, k + 1) * 0.37 - 2.0 + 1e4
        rec["offset"] = -2000 + rng.randint(-spread, spread + 1, k + 1)  # negative offsets, with ties
        rec["flags"][rng.rand(k + 1) < 0.3] |= _native.FLAG_DIRECT  # a flag the reduction ignores
        return rec

    files = [blank()]
    wide = blank(6000)  # offsets all over a window
    files.append(wide)
    far = blank()  # offsets beyond +-2^31: a 32-bit shortcut fails
    far["offset"] = far["offset"] + (np.int64(1) << 40) * rng.randint(-1, 2, k + 1)
    far["offset"][0] = -(np.int64(1) << 40) + 3
    files.append(far)
    same = blank(0)  # every offset the same
    files.append(same)
    holes = blank(50)  # non-finite and EMPTY_WINDOW records skipped; pairs with one member unusable
    pick = rng.rand(k + 1)
    holes["score"][(pick < 0.15)] = -np.inf
    holes["score"][(pick >= 0.15) & (pick < 0.25)] = np.nan
    holes["score"][(pick >= 0.25) & (pick < 0.3)] = np.inf
    holes["flags"][(pick >= 0.3) & (pick < 0.45)] |= _native.FLAG_EMPTY_WINDOW
    holes["offset"][pick < 0.45] = 7777777  # what an unusable record holds does not count
    holes["score"][0], holes["flags"][0], holes["offset"][0] = 10001.5, 0, -2000
    if k >= 2:
        holes["score"][1], holes["flags"][1], holes["offset"][1], holes["score"][2] = 5.0, 0, -1990, np.nan  # pair 0: one member unusable
    files.append(holes)
    none = blank()  # no usable subsample, one of them ambiguous
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
    amb = blank()  # AMBIGUOUS carried: on the real record here, on the last subsample above
    amb["flags"][0] |= _native.FLAG_AMBIGUOUS
    files.append(amb)
    sums = blank()  # pair sums that round: the sum is one fp64 addition
    sums["score"] = 1e4 + rng.rand(k + 1) * np.exp2(rng.randint(-30, 10, k + 1))
    files.append(sums)
    return files


def _want_record(rec, tol):
    from ffsubsync_amd import _native

    want = stm.offset_stats(rec["score"], rec["offset"], rec["flags"], tol)
    row = np.zeros(1, _native.STABILITY_RESULT_DTYPE)
    for name in stm.FIELDS:
        row[name] = want[name]
    return want, row


@pytest.mark.parametrize("k", STATS_K)
def test_offset_stats_equal_the_model_bit_for_bit(k):
    import torch
    from ffsubsync_amd import _native, stability

    files, tol, size = _stats_files(k), STATS_TOL[k], _native.STABILITY_RESULT_BYTES
    host = np.concatenate(files + [np.zeros(1, files[0].dtype)])
    table = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    out = torch.full((len(files) * size + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    _native.offset_stats(table, len(files), k, tol, out=out[8:])
    raw = out.cpu().numpy()
    assert (raw[:8] == 0xAB).all() and (raw[8 + len(files) * size:] == 0xAB).all()
    assert np.array_equal(table.cpu().numpy(), host.view(np.uint8))  # records are read, never written
    got = raw[8:8 + len(files) * size].view(_native.STABILITY_RESULT_DTYPE)
    assert np.array_equal(stability.offset_stats(table, len(files), k, tol).view(np.uint8), got.view(np.uint8))
    flags = []
    for f, (rec, g) in enumerate(zip(files, got)):
        want, row = _want_record(rec, tol)
        for name in stm.FIELDS:
            assert g[name].tobytes() == row[name][0].tobytes(), (f, name, g[name], want[name])
        assert g.tobytes() == row.tobytes(), f  # the reserved word too
        flags.append(want["flags"])
    no_pairs = stm.NO_PAIRS if k < 2 else 0
    assert flags[0] == flags[1] == flags[2] == flags[3] == no_pairs and flags[5] == stm.EMPTY | stm.NO_PAIRS | stm.AMBIGUOUS
    assert flags[6] == flags[7] == stm.EMPTY | no_pairs and flags[8] == stm.AMBIGUOUS | no_pairs
    assert int(got[3]["max_dev"]) == 0 and int(got[3]["n_within"]) == k and int(got[3]["off_lo"]) == int(got[3]["off_hi"]) == -2000
    if k >= 63:
        assert int(got[2]["max_dev"]) >= (1 << 41) - 3000 and int(got[2]["off_min"]) < -(1 << 39) and int(got[2]["off_max"]) > 1 << 39
    assert int(got[2]["real_offset"]) == -(1 << 40) + 3 and int(got[6]["off_max"]) == 0 and int(got[6]["n_sub"]) == k
    if k >= 64:
        assert 0 < int(got[4]["n_pairs"]) < k // 2 and 0 < int(got[4]["n_sub"]) < k and int(got[4]["off_max"]) < 7777777


def test_offset_stats_refusals_leave_the_outputs_untouched():
    import torch
    from ffsubsync_amd import _native

    files = _stats_files(3)
    table = torch.from_numpy(np.concatenate(files).view(np.uint8).copy()).cuda()
    out = torch.full((len(files) * _native.STABILITY_RESULT_BYTES + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    lib, st = _native.load(), _native.current_stream_ptr(torch)
    for args in ((table.data_ptr(), -1, 3, 0, out.data_ptr()), (table.data_ptr(), 2, 0, 0, out.data_ptr()),
                 (table.data_ptr(), 2, 4097, 0, out.data_ptr()), (table.data_ptr(), 2, 3, -1, out.data_ptr()),
                 (None, 2, 3, 0, out.data_ptr()), (table.data_ptr(), 2, 3, 0, None),
                 (table.data_ptr() + 4, 2, 3, 0, out.data_ptr()), (table.data_ptr(), 2, 3, 0, out.data_ptr() + 4)):
        assert lib.ffs_offset_stats(*args, st) == -1, args
        assert lib.ffs_last_error().decode().startswith("ffs_offset_stats: ")
    assert lib.ffs_offset_stats(table.data_ptr(), 0, 3, 0, out.data_ptr(), st) == 0
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
        from ffsubsync_amd import _native
        from oracle import raster_oracle as ro

        keep, rows = [], []
        for i in E2E:
            ref, track = cases.sync_problems()[i]
            model = sc.model_sync(i)
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


def _stability_test(sel=slice(None), **kw):
    from ffsubsync_amd import stability

    rp, rl, rb, sp, sl, sb, hi, seeds = [c[sel] for c in _device_lists()]
    return stability.stability_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, cases.W, cases.K, 1,
                                          tol=sc.TOL, sub_hi=hi, seeds=seeds, **kw)


def _check_record(rec, want):
    for name in stm.FIELDS:
        assert rec[name] == want[name], (name, rec[name], want[name])


def test_stability_test_lists_equal_the_exact_reference():
    """Every (score, offset) of the table against ``exact_reference.candidate`` on the model's expanded half-sample (what
    ``stability_model.half_records`` holds), and the records against the model."""
    test = _stability_test()
    assert not test.status.any() and test.stats["careful_files"] == 0 and test.stats["chunks"] == 1
    solves = test.solves()
    assert solves.shape == (len(E2E), cases.K + 1)
    for row, i in enumerate(E2E):
        model = sc.model_sync(i)
        assert np.array_equal(solves[row]["score"], model["scores"]), i
        assert np.array_equal(solves[row]["offset"], model["offsets"]), i
        assert not solves[row]["flags"].any()
        _check_record(test.records[row], model["record"])


def test_a_file_alone_equals_the_file_inside_a_batch_and_chunks_change_nothing():
    whole = _stability_test()
    for row in (0, 3):
        alone = _stability_test(slice(row, row + 1))
        assert alone.records.tobytes() == whole.records[row:row + 1].tobytes()
        assert alone.solves().tobytes() == whole.solves()[row:row + 1].tobytes()
    parts = _stability_test(budget_bytes=1)  # one file per chunk
    assert parts.stats["chunks"] == len(E2E)
    assert parts.records.tobytes() == whole.records.tobytes() and parts.solves().tobytes() == whole.solves().tobytes()


def test_two_calls_queued_on_one_stream_equal_the_calls_made_apart():
    """``raw``: nothing is read back (records and status stay CUDA tensors), so two whole tests (lists, solves,
    reduction) queue behind each other on a side stream with no synchronisation in between."""
    import torch
    from ffsubsync_amd import _native

    apart = [_stability_test(slice(0, 2)), _stability_test(slice(2, 4))]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        first = _stability_test(slice(0, 2), raw=True)
        second = _stability_test(slice(2, 4), raw=True)
    for got in (first, second):
        assert got.records.is_cuda and got.status.is_cuda and got.table.is_cuda and got.stats["careful_files"] == 0
    stream.synchronize()
    for got, want in zip((first, second), apart):
        recs = got.records.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:2]
        assert recs.tobytes() == want.records.tobytes()
        assert got.table.cpu().numpy().tobytes() == want.table.cpu().numpy().tobytes()
        assert not got.status.cpu().numpy().any()


def test_stable_sync_equals_the_model_and_separates_the_classes():
    from ffsubsync_amd import stability

    problems, kinds = cases.sync_problems(), cases.sync_kinds()
    got = stability.stable_sync(problems, 60, tol=sc.TOL, min_share=sc.MIN_SHARE)
    assert len(got) == len(problems) == 12
    for i, (r, kind) in enumerate(zip(got, kinds)):
        model = sc.model_sync(i)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        _check_record(vars(r.record), model["record"])
        assert r.interval_samples == model["interval_samples"] and r.interval_seconds == (r.interval_samples[0] / 100.0, r.interval_samples[1] / 100.0)
        assert r.share_within == model["share_within"] and r.reasons == model["reasons"]
        assert r.stable is model["stable"] is (kind == "matched"), (i, kind, r.share_within)
    none = stability.stable_sync(problems[:1], 60)  # the shipped defaults: the interval alone, no verdict
    assert none[0].stable is None and none[0].reasons == [] and none[0].interval_samples == got[0].interval_samples
    assert none[0].record.tol == stability.DEFAULT_TOL


def test_the_careful_path_gives_the_fast_path_s_table():
    """``stability._careful`` (the redo of an AMBIGUOUS file: half-samples expanded and solved pair by pair through
    ``solve_pairs``) on one matched E2E file: its K + 1 records are the rows of the fast path's table.  (DESIGN 3.24 found
    no input that raises AMBIGUOUS on the run path, so the redo is called directly.)"""
    from ffsubsync_amd import stability

    fast = _stability_test().solves()
    rp, rl, rb, sp, sl, sb, hi, seeds = _device_lists()
    recs = stability._careful((int(rp[0]), int(rb[0]), int(rl[0]), 0.0, 1.0), (int(sp[0]), int(sb[0]), int(sl[0]), 0.0, float(hi[0])),
                              int(seeds[0]), cases.K, 1, cases.W)
    assert recs.dtype == fast.dtype and recs.shape == (cases.K + 1,)
    assert np.array_equal(recs["score"], fast[0]["score"]) and np.array_equal(recs["offset"], fast[0]["offset"])
