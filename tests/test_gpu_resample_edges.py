"""The shuffled-cue and half-sample paths where their own GPU tests do not look: keys that no random
seed reaches, positions and ``ones`` at the ends of int32, list calls queued faster than their descriptor uploads
complete, inputs written and outputs read by neighbours on the same stream, and the end-to-end wrappers on files and
tracks of a handful of cues.  The cases are tests/resample_edge_cases.py's (held to what they name by
tests/test_resample_edge_cases_host.py); the ``Call`` layouts are those of tests/test_gpu_surrogate.py and
tests/test_gpu_stability.py (blocks at 8-byte alignment only, poison in every gap).  Expected values come from
tests/surrogate_model.py, tests/stability_model.py and tests/exact_reference.py, never from a device run; every
comparison is exact (``null_mean`` / ``null_std`` as tests/test_gpu_surrogate.py compares them).  Need a real MI355X."""
import math

import numpy as np
import pytest

import resample_edge_cases as rc
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm
import test_gpu_stability as tst
import test_gpu_surrogate as tsu

pytestmark = pytest.mark.gpu
_memo = {}


def _block(pos, length, spare=0):
    return sm.encode(pos, length, len(pos) + 1 + spare)


def _out_words(call, v, s):
    """The int32 words of output block (v, s) of a ``Call``, from the device."""
    cap = int(call.caps[v])
    o = int(call.out_off[v]) + s * (16 + 8 * cap)
    return call.out[o:o + 16 + 8 * cap].cpu().numpy().view(np.int32)


def _queue(call):
    """The call of a ``Call`` on the current stream, nothing waited for."""
    from ffsubsync_amd import _native

    fn = _native.surrogate_lists if isinstance(call, tsu.Call) else _native.subsample_lists
    fn(call.ptrs, call.n_bound, call.seeds, call.out_off, call.caps, call.k, call.b, call.out, call.status)


# ---- 1. crafted keys -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_units", sorted({c[1] for c in rc.SURROGATE_CASES}))
def test_surrogate_keys_equal_to_the_padding_word_and_to_zero(block_units):
    """Every crafted case of one block size as the vectors of one call (a call takes one block size): the key 0xFFFFFFFF,
    which the sort cannot tell from its padding, and the key 0, on the first, a middle, the last and the short last block."""
    picked = [(i, c) for i, c in enumerate(rc.SURROGATE_CASES) if c[1] == block_units]
    lists = [rc.crafted_list("surrogate", i) for i, _ in picked]
    call = tsu.Call([_block(p, n, spare=j % 3) for j, (p, n) in enumerate(lists)], [p.size + (0, 2, 6)[j % 3] for j, (p, _) in enumerate(lists)],
                    [rc.surrogate_seed(c) for _, c in picked], rc.SURROGATE_K, block_units).run()
    call.check()
    assert not call.want_status()[:-2].any()
    for v, ((_, (units, block, s, b, key)), (pos, _)) in enumerate(zip(picked, lists)):
        # on the device's output: the units of the last block sit at the place cases.short_block_place names
        nb = rc.n_blocks_of(units, block)
        seed = int(call.seeds[v])
        place, tail = cases.short_block_place(seed, s, units, block), units - (nb - 1) * block
        if b == nb - 1:
            assert place == (nb - 1 if key == rc.PAD_KEY else 0)
        got = _out_words(call, v, s)
        assert int(got[0]) == pos.size
        out = got[4:4 + 2 * pos.size:2].astype(np.int64)
        first = place * block  # (every block in front of the last one's place is a full one)
        src = (nb - 1) * block
        assert np.array_equal(np.diff(out)[2 * first:2 * (first + tail)], np.diff(pos)[2 * src:2 * (src + tail)]), (v, place)


@pytest.mark.parametrize("block_runs", sorted({c[1] for c in rc.STABILITY_CASES}))
def test_half_sample_keys_on_either_side_of_the_keep_bit(block_runs):
    """Keys 0x7FFFFFFF and 0x80000000 on a middle block and on the last block: ``key >> 31`` decides, and flips."""
    picked = [(i, c) for i, c in enumerate(rc.STABILITY_CASES) if c[1] == block_runs]
    lists = [rc.crafted_list("stability", i) for i, _ in picked]
    call = tst.Call([_block(p, n, spare=j % 3) for j, (p, n) in enumerate(lists)], [p.size + (0, 2, 6)[j % 3] for j, (p, _) in enumerate(lists)],
                    [rc.stability_seed(c) for _, c in picked], rc.STABILITY_K, block_runs).run()
    call.check()
    assert not call.want_status()[:-2].any()
    for v, ((_, (runs, block, s, b, key)), (pos, _)) in enumerate(zip(picked, lists)):
        got = _out_words(call, v, s)
        out = got[4:4 + 2 * int(got[0]):2].tolist()
        want_kept = (key == rc.KEEP_BIT) == (s % 2 == 0)
        assert (int(pos[2 * b * block]) in out) == want_kept, (v, s, b, hex(key))


# ---- 2. large positions --------------------------------------------------------------------------------------------------
def _large_call(cls, block):
    lists = [rc.large_lists()[name] for name in ("a", "a3", "b", "c", "c3")]
    blocks = [_block(p, n, spare=j % 3) for j, (p, n) in enumerate(lists)]
    bound = [p.size + (0, 2, 6)[j % 3] for j, (p, _) in enumerate(lists)]
    return cls(blocks, bound, [7, 0xFFFFFFFF, 12345, 0, 99], rc.LARGE_K, block)


@pytest.mark.parametrize("block_units", rc.LARGE_BLOCKS)
def test_surrogates_of_lists_that_end_at_int32_max(block_units):
    """len = 2^31 - 1: shifts of ``pos`` of up to nearly 2^31 either way, ``ones`` above 2^30 (the packed (span, ones)
    scan), a unit that spans nearly the whole vector.  Images against the model; nothing is expanded to samples."""
    call = _large_call(tsu.Call, block_units).run()
    call.check()
    assert not call.want_status()[:-2].any()
    for v, name in enumerate(("a", "a3", "b", "c", "c3")):  # ``ones`` counted from the positions, not read from a header
        ones = rc.ones_of(rc.large_lists()[name][0])
        for s in range(rc.LARGE_K):
            got = _out_words(call, v, s)
            n = int(got[0])
            assert int(got[1]) == ones and tuple(got[4 + 2 * n:6 + 2 * n]) == (rc.INT32_MAX, ones) and int(got[3 + 2 * n]) == ones
    for v in (3, 4):  # (the surrogates of the 2 050-run lists are not the inputs)
        n = int(call.blocks[v][0])
        assert all(not np.array_equal(_out_words(call, v, s)[4:4 + 2 * n], call.blocks[v][4:4 + 2 * n]) for s in range(rc.LARGE_K))


@pytest.mark.parametrize("block_runs", rc.LARGE_BLOCKS)
def test_half_samples_of_lists_that_end_at_int32_max(block_runs):
    call = _large_call(tst.Call, block_runs).run()
    call.check()
    assert not call.want_status()[:-2].any()
    for v in range(5):  # complementary members: their ``ones`` add up to the input's, above 2^30 for list (b)
        total = [int(_out_words(call, v, s)[1]) for s in (0, 1)]
        assert sum(total) == int(call.blocks[v][1])


# ---- 3. queued list calls ------------------------------------------------------------------------------------------------
SEQ_RUNS = (66, 10, 301)  # runs of the three vectors of every call of a sequence


def _sequence_call(j):
    """Call j of a sequence: surrogate and half-sample calls alternate.  Safety rule of tests/stream_cases.py: the calls of
    a sequence have identical list sizes, bounds, capacities, offsets, K and B (so the two ``Call`` layouts are the same)
    and differ only in seeds and contents -- mixed-up descriptors would give wrong bytes inside the same buffers, never
    an access outside them."""
    rng = np.random.RandomState(500 + j)
    lists = [cases.random_list(rng, m - 1, kind=v % 4) for v, m in enumerate(SEQ_RUNS)]
    cls = tsu.Call if j % 2 == 0 else tst.Call
    return cls([_block(p, n, spare=1) for p, n in lists], [p.size + 2 for p, _ in lists], rng.randint(0, 2 ** 32, 3, dtype=np.uint64), 3, 2)


def _same_shapes(calls):
    first = calls[0]
    for c in calls[1:]:
        assert c.in_off == first.in_off and np.array_equal(c.out_off, first.out_off) and np.array_equal(c.caps, first.caps)
        assert c.out_bytes == first.out_bytes and np.array_equal(c.n_bound, first.n_bound) and (c.k, c.b) == (first.k, first.b)
        assert not np.array_equal(c.seeds, first.seeds) and not np.array_equal(c.in_host, first.in_host)


def test_six_list_calls_queued_behind_a_fill_on_one_stream():
    """Six calls that alternate ``ffs_surrogate_lists`` and ``ffs_subsample_lists`` on one side stream with no host
    synchronisation between them: the two pinned descriptor buffers are handed out three times each, so a buffer is
    rewritten while the stream still holds copies out of it unless ``stage_acquire`` waits for them.  A device fill of
    2 GiB, eight times over, is queued first so that the uploads are still pending when the host writes the next table.
    The fill only makes a race more likely: the verdict is the images, every call against its own model, and does not
    depend on how long the fill takes."""
    import torch

    calls = [_sequence_call(j) for j in range(6)]
    _same_shapes(calls)
    ballast = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the inputs are uploaded, the outputs poisoned, nothing pending
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for i in range(8):
            ballast.fill_(i)
        for call in calls:
            _queue(call)
    stream.synchronize()
    for call in calls:
        call.check()
    del ballast


def test_three_list_calls_each_on_two_streams_at_once():
    """The same sequence, calls 0, 2, 4 on one side stream and 1, 3, 5 on another, issued alternately by one host thread:
    the staging buffers (thread-local, shared by both streams) go from a call on one stream to a call on the other."""
    import torch

    calls = [_sequence_call(10 + j) for j in range(6)]
    _same_shapes(calls)
    ballast = [torch.empty(1 << 30, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j, s in enumerate(streams):
        with torch.cuda.stream(s):
            for i in range(4):
                ballast[j].fill_(i)
    for j, call in enumerate(calls):
        with torch.cuda.stream(streams[j % 2]):
            _queue(call)
    for s in streams:
        s.synchronize()
    for call in calls:
        call.check()
    del ballast


# ---- 4. late inputs and late readers ---------------------------------------------------------------------------------------
def _packed(v01):
    import torch

    packed = np.packbits(np.asarray(v01, np.uint8), bitorder="little").tobytes().ljust((len(v01) + 31) // 32 * 4, b"\0")
    return torch.from_numpy(np.frombuffer(packed, np.int32).copy()).cuda()


@pytest.mark.parametrize("export", ["surrogate", "subsample"])
def test_a_list_written_just_before_and_an_output_read_just_after(export):
    """On a side stream, no host wait in between: ``ffs_runs_from_bits`` writes the input list into a poisoned block, the
    list export reads it, ``ffs_runs_to_bits`` reads output block 1."""
    import torch
    from ffsubsync_amd import _native

    rng = np.random.RandomState(44)
    pos, length = cases.random_list(rng, 140, kind=1)
    n, k, b, seed = pos.size, 3, 2, 0xC0FFEE
    words = _packed(sm.expand(pos, length))
    cap_in, cap_out = n + 2, n + 1
    inp = torch.full((4 + 2 * cap_in,), -1, dtype=torch.int32, device="cuda")
    stride = 16 + 8 * cap_out
    out = torch.full((k * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    status = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    bits = torch.full((_native.packed_words(length),), -1, dtype=torch.int32, device="cuda")
    fn = _native.surrogate_lists if export == "surrogate" else _native.subsample_lists
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _native.runs_from_bits(words, length, cap=cap_in, out=inp)
        fn(np.array([inp.data_ptr()], np.uint64), [n], [seed], [0], [cap_out], k, b, out, status)
        _native.runs_to_bits(out[stride:2 * stride].view(torch.int32), length, out=bits)
    stream.synchronize()
    model = (lambda s: sm.surrogate(pos, seed, s, b)) if export == "surrogate" else (lambda s: stm.subsample(pos, seed, s, b))
    want = np.full(k * stride, 0xAB, np.uint8)
    for s in range(k):
        w = sm.encode(model(s), length, cap_out).view(np.uint8)
        want[s * stride:s * stride + w.size] = w
    assert np.array_equal(out.cpu().numpy(), want) and int(status.cpu()[0]) == 0
    assert np.array_equal(inp.cpu().numpy()[:4 + 2 * (n + 1)], sm.encode(pos, length, cap_in))
    got_bits = _native.unpack_bits(bits, length).cpu().numpy()
    assert np.array_equal(got_bits, sm.expand(model(1), length)) and not np.array_equal(got_bits, sm.expand(pos, length))


def _late_table(files):
    """The record table of ``files`` copied from pinned memory by an asynchronous copy on the current stream."""
    import torch

    host = np.concatenate(files)
    pinned = torch.from_numpy(host.view(np.uint8).copy()).pin_memory()
    table = torch.full((pinned.numel() + 24,), 0xFF, dtype=torch.uint8, device="cuda")
    return host, pinned, table


def test_null_stats_of_a_table_that_a_copy_on_the_stream_has_just_filled():
    import torch
    from ffsubsync_amd import _native

    k = 65
    files = tsu._stats_files(k)
    host, pinned, table = _late_table(files)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        table[:pinned.numel()].copy_(pinned, non_blocking=True)
        out = _native.null_stats(table, len(files), k)
    stream.synchronize()
    got = out.cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:len(files)]
    for f, (rec, g) in enumerate(zip(files, got)):
        want = sm.stats(rec["score"], rec["flags"])
        for name in ("n_null", "n_ge", "n_gt", "flags"):
            assert int(g[name]) == want[name], (f, name, int(g[name]), want[name])
        for name in ("real_score", "null_min", "null_max"):
            assert tsu._same_bits(float(g[name]), want[name]), (f, name, float(g[name]), want[name])
        for name in ("null_mean", "null_std"):  # (fixed-order sums against numpy's pairwise sums, as test_null_stats_equal_the_model)
            assert math.isclose(float(g[name]), want[name], rel_tol=1e-12, abs_tol=0.0), (f, name, float(g[name]), want[name])
    assert np.array_equal(table.cpu().numpy()[:pinned.numel()], host.view(np.uint8))


def test_offset_stats_of_a_table_that_a_copy_on_the_stream_has_just_filled():
    import torch
    from ffsubsync_amd import _native

    k, tol = 65, 5
    files = tst._stats_files(k)
    host, pinned, table = _late_table(files)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        table[:pinned.numel()].copy_(pinned, non_blocking=True)
        out = _native.offset_stats(table, len(files), k, tol)
    stream.synchronize()
    got = out.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:len(files)]
    for f, (rec, g) in enumerate(zip(files, got)):
        _, row = tst._want_record(rec, tol)
        assert g.tobytes() == row.tobytes(), f
    assert np.array_equal(table.cpu().numpy()[:pinned.numel()], host.view(np.uint8))


# ---- 5. tiny files end to end --------------------------------------------------------------------------------------------
def _tiny_lists():
    """The seven tiny files as device-resident lists: the references through ``ffs_runs_from_bits``, the subtitles as the
    model's words (``sm.encode``).  Columns of ``null_test_lists``' arguments."""
    if "tiny" not in _memo:
        import torch
        from ffsubsync_amd import _native

        keep, rows = [], []
        for i, (ref_len, ref_lv, _, sub_len, sub_lv, seed, _) in enumerate(rc.TINY_FILES):
            ref, pos, _ = rc.tiny_file(i)
            n_ref = sm.boundaries(ref).size
            ref_block = _native.runs_from_bits(_packed(ref), ref_len, cap=n_ref + 2)
            sub_block = torch.from_numpy(sm.encode(pos, sub_len, pos.size + 1)).cuda()
            keep.append((ref_block, sub_block))
            rows.append((ref_block.data_ptr(), ref_len, n_ref, sub_block.data_ptr(), sub_len, pos.size, ref_lv[0], ref_lv[1],
                         sub_lv[0], sub_lv[1], seed))
        torch.cuda.synchronize()
        _memo["tiny"] = (keep, [np.array(c) for c in zip(*rows)])
    return _memo["tiny"][1]


def _tiny_null(block, k, **kw):
    from ffsubsync_amd import surrogate

    rp, rl, rb, sp, sl, sb, rlo, rhi, slo, shi, seeds = _tiny_lists()
    return surrogate.null_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, rc.TINY_W, k, block, ref_lo=rlo,
                                     ref_hi=rhi, sub_lo=slo, sub_hi=shi, seeds=seeds, **kw)


def _tiny_half(block, k, **kw):
    from ffsubsync_amd import stability

    rp, rl, rb, sp, sl, sb, rlo, rhi, slo, shi, seeds = _tiny_lists()
    return stability.stability_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, rc.TINY_W, k, block,
                                          tol=rc.TINY_TOL, ref_lo=rlo, ref_hi=rhi, sub_lo=slo, sub_hi=shi, seeds=seeds, **kw)


def _two_file_budget(k):
    """``budget_bytes`` that holds the blocks of exactly two files: chunks of 2, 2, 2 and 1."""
    return 2 * k * (16 + 8 * (max(f[2] for f in rc.TINY_FILES) * 2 + 1))


def _check_null_table(solves, records, block, k):
    n = len(rc.TINY_FILES)
    assert solves.shape == (n, k + 1)
    for i in range(n):
        sc, fl = rc.tiny_model(i, block)["null"]
        half = rc.tiny_model(i, block)["half"]
        assert np.array_equal(solves[i]["score"], sc[:k + 1]), (i, solves[i]["score"], sc[:k + 1])
        assert np.array_equal(solves[i]["flags"], fl[:k + 1]), (i, solves[i]["flags"])
        assert int(solves[i][0]["offset"]) == int(half[1][0]), i  # (the real solve: the half-sample model's record 0)
        tsu._check_record(records[i], rc.tiny_null_record(i, block, k))


def _check_half_table(solves, records, block, k):
    n = len(rc.TINY_FILES)
    assert solves.shape == (n, k + 1)
    for i in range(n):
        sc, off, fl = rc.tiny_model(i, block)["half"]
        assert np.array_equal(solves[i]["score"], sc[:k + 1]), (i, solves[i]["score"], sc[:k + 1])
        assert np.array_equal(solves[i]["offset"], off[:k + 1]), (i, solves[i]["offset"], off[:k + 1])
        assert np.array_equal(solves[i]["flags"], fl[:k + 1]), (i, solves[i]["flags"])
        tst._check_record(records[i], rc.tiny_half_record(i, block, k))


@pytest.mark.parametrize("block_units", rc.TINY_BLOCKS)
def test_null_test_lists_on_files_of_a_handful_of_cues(block_units):
    """Subtitles of 0, 1, 2, 3, 9 and 40 runs, lengths, bounds and levels that differ from file to file, block sizes up to
    larger than every list, K = 1, 2, 5, 6: every score and flag of the table and every record against the model; then
    the same in chunks of 2, 2, 2 and 1 files, byte for byte the unchunked call."""
    for k in rc.TINY_K:
        test = _tiny_null(block_units, k)
        assert not test.status.any() and test.stats["chunks"] == 1 and test.stats["careful_files"] == 0
        _check_null_table(test.solves(), test.records, block_units, k)
        parts = _tiny_null(block_units, k, budget_bytes=_two_file_budget(k))
        assert parts.stats["chunks"] == 4 and parts.stats["careful_files"] == 0 and not parts.status.any()
        assert parts.records.tobytes() == test.records.tobytes() and parts.solves().tobytes() == test.solves().tobytes()


@pytest.mark.parametrize("block_runs", rc.TINY_BLOCKS)
def test_stability_test_lists_on_files_of_a_handful_of_cues(block_runs):
    """The same files through the half-samples: a silent subtitle and every half-sample that keeps nothing go through
    ``align_batch`` as empty boundary lists, where every lag's score is the reference's alone and the exact tie rule
    names the offset; K = 1 has no pair, K = 5 a last half-sample without a partner."""
    for k in rc.TINY_K:
        test = _tiny_half(block_runs, k)
        assert not test.status.any() and test.stats["chunks"] == 1 and test.stats["careful_files"] == 0
        _check_half_table(test.solves(), test.records, block_runs, k)
        parts = _tiny_half(block_runs, k, budget_bytes=_two_file_budget(k))
        assert parts.stats["chunks"] == 4 and parts.stats["careful_files"] == 0 and not parts.status.any()
        assert parts.records.tobytes() == test.records.tobytes() and parts.solves().tobytes() == test.solves().tobytes()


def test_tiny_files_queued_twice_on_a_side_stream_with_nothing_read_back():
    """``raw=True``: two whole null tests and two whole stability tests (lists, solves, reduction; in chunks, so several
    list calls each) queue behind each other on a side stream; after one synchronisation every table and record is the
    model's."""
    import torch
    from ffsubsync_amd import _native

    block, n = 2, len(rc.TINY_FILES)
    _tiny_lists()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got = [(_tiny_null(block, 5, raw=True, budget_bytes=_two_file_budget(5)), _tiny_half(block, 6, raw=True, budget_bytes=_two_file_budget(6)))
               for _ in range(2)]
    stream.synchronize()
    for null, half in got:
        assert null.records.is_cuda and half.records.is_cuda and null.stats["chunks"] == half.stats["chunks"] == 4
        assert not null.status.cpu().numpy().any() and not half.status.cpu().numpy().any()
        solves = null.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * 6].reshape(n, 6)
        _check_null_table(solves, null.records.cpu().numpy().view(_native.NULL_RESULT_DTYPE)[:n], block, 5)
        solves = half.table.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:n * 7].reshape(n, 7)
        _check_half_table(solves, half.records.cpu().numpy().view(_native.STABILITY_RESULT_DTYPE)[:n], block, 6)


# ---- 6. tiny tracks ------------------------------------------------------------------------------------------------------
def test_null_sync_on_tracks_of_one_to_nine_cues():
    from ffsubsync_amd import surrogate

    got = surrogate.null_sync(list(rc.track_problems()), rc.TRACK_SECONDS, n_surrogates=rc.TRACK_K, block_units=1, seed=rc.TRACK_SEED,
                              min_z=rc.TRACK_MIN_Z)
    assert len(got) == len(rc.TRACK_CUES)
    for i, r in enumerate(got):
        model = rc.track_null_model(i)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        tsu._check_record(vars(r.null), model["record"])
        assert r.p == model["p"] and r.trusted == model["trusted"], i
        assert r.z == model["z"] or math.isclose(r.z, model["z"], rel_tol=1e-9), i  # (from null_mean / null_std)
        assert r.reasons == model["reasons"], (i, r.reasons, model["reasons"])


def test_stable_sync_on_tracks_of_one_to_nine_cues():
    from ffsubsync_amd import stability

    got = stability.stable_sync(list(rc.track_problems()), rc.TRACK_SECONDS, n_subsamples=rc.TRACK_K, block_runs=1, seed=rc.TRACK_SEED,
                                tol=rc.TRACK_TOL, min_share=rc.TRACK_MIN_SHARE)
    assert len(got) == len(rc.TRACK_CUES)
    for i, r in enumerate(got):
        model = rc.track_stable_model(i)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        tst._check_record(vars(r.record), model["record"])
        assert r.interval_samples == model["interval_samples"] and r.share_within == model["share_within"], i
        assert r.stable is model["stable"] and r.reasons == model["reasons"], (i, r.reasons, model["reasons"])
