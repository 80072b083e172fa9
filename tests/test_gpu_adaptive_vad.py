"""The adaptive energy VAD (ffsubsync_amd.adaptive_vad) against the numpy / integer model of
tests/adaptive_vad_model.py, bit for bit everywhere: k_vad_levels on the buffers of ingest_reference.energy_cases under five
edge tables, k_vad_level_hist around its launch geometry, k_vad_pick_threshold on a table of histograms written by the
test, k_vad_level_labels, the two whole-file entries and PCMSpeechTransformer(vad="adaptive").  Outputs of many cases sit
side by side in one buffer with sentinel bytes between them and are read back once.
tests/test_adaptive_vad_host.py asserts, on the same builders, that no frame is within rounding of an edge and that no
histogram of the pick table is decided by rounding.  The rule has no upstream counterpart: the model is the reference."""
import io

import numpy as np
import pytest

import adaptive_vad_model as am
import ingest_reference as ir
from oracle import vad_oracle as vo

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
LEVEL_OFFSETS = (0, 1, 3)   # byte offsets of a case's level bytes from an 8-byte boundary: the 8-byte store and the byte loop


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def native(torch):
    from ffsubsync_amd import _native

    return _native.load(), _native


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream(torch, native):
    return native[1].current_stream_ptr(torch)


@pytest.fixture(scope="module")
def tables(torch):
    host = am.edge_tables()
    return host, {name: _dev(torch, e) for name, e in host.items()}


@pytest.fixture(scope="module")
def grid_stride(torch):
    """ir.grid_stride_pcm() and its model levels under the default table (computed once, shared)."""
    pcm = ir.grid_stride_pcm()
    return pcm, am.frame_levels(pcm, ir.GRID_STRIDE_FRAME_LEN, am.default_edges())


# ---- k_vad_levels --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("frame_len", ir.FRAME_LENS)
def test_frame_level_sweep(torch, native, tables, frame_len):
    """ffs_vad_levels through the C ABI on every case of ingest_reference.energy_cases (vector widths of 1 .. 64 lanes,
    the element loop for odd lengths, lengths above 512 and unaligned bases, start offsets of 0, 1, 3 and 8 samples, every
    residue of the frame count mod 8, tails of none, one and frame_len - 1 samples, frames exactly at, one below and one
    above a decade edge, full-scale frames) under every edge table (default, 1, 64, 65 and 255 edges), the level bytes
    written 0, 1 and 3 bytes behind an 8-byte boundary; nothing is written behind the last frame.  On the default table
    level_labels(levels, 100) in packed form equals ffs_vad_energy_bits(pcm, 50.0) byte for byte."""
    lib, _native = native
    stream = _stream(torch, native)
    host_tables, dev_tables = tables
    cases = list(ir.energy_cases(frame_len))
    jobs, pos, bpos = [], 0, 0
    for ci, c in enumerate(cases):
        nf = -(-c["n_samples"] // frame_len)
        for ti, name in enumerate(host_tables):
            pos = (pos + 7) // 8 * 8 + LEVEL_OFFSETS[(ci + ti) % 3]
            jobs.append((c, name, pos, nf, bpos if name == "default" else None))
            pos += nf + 8
            if name == "default":
                bpos += (nf + 7) // 8 + 8
    out = torch.full((pos + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 8 == 0
    bits_new = torch.full((bpos,), SENTINEL, dtype=torch.uint8, device="cuda")
    bits_old = torch.full((bpos,), SENTINEL, dtype=torch.uint8, device="cuda")
    uploaded = {}
    for c, name, at, nf, bat in jobs:
        if id(c["buffer"]) not in uploaded:
            uploaded[id(c["buffer"])] = _dev(torch, c["buffer"])
        pcm = uploaded[id(c["buffer"])][c["offset"]:]
        _native.check(lib.ffs_vad_levels(pcm.data_ptr(), c["n_samples"], frame_len, dev_tables[name].data_ptr(),
                                         host_tables[name].size, out.data_ptr() + at, stream))
        if bat is not None:
            _native.check(lib.ffs_vad_level_labels(out.data_ptr() + at, nf, None, 100, 0.0, None, bits_new.data_ptr() + bat, stream))
            _native.check(lib.ffs_vad_energy_bits(pcm.data_ptr(), c["n_samples"], frame_len, 50.0, bits_old.data_ptr() + bat, stream))
    host = out.cpu().numpy()
    covered = np.zeros(host.size, bool)
    sums = {}
    for c, name, at, nf, _ in jobs:
        key = (id(c["buffer"]), c["offset"], c["n_samples"])
        if key not in sums:
            sums[key] = ir.frame_sums(ir.case_pcm(c), frame_len)
        want = am.levels_of_sums(*sums[key], host_tables[name])
        what = (frame_len, name, c["offset"], c["n_samples"], at % 8)
        assert want.size == nf and np.array_equal(host[at:at + nf], want), what
        covered[at:at + nf] = True
    assert np.all(host[~covered] == SENTINEL)
    assert torch.equal(bits_new, bits_old) and bool((bits_new != SENTINEL).any())


def test_frame_levels_grid_stride_trip(torch, native, grid_stride):
    """More than 524 288 frames: the waves of k_vad_levels' capped grid take a second trip, on the vector path and (one
    sample into the allocation) on the element path.  level_labels takes its second trip on the same levels."""
    from ffsubsync_amd import _native, adaptive_vad

    pcm, want = grid_stride
    fl = ir.GRID_STRIDE_FRAME_LEN
    for off in (0, 1):
        dev = _dev(torch, np.concatenate([np.full(8 + off, 32767, np.int16), pcm, np.full(64, -32768, np.int16)]))
        dev = dev[8 + off: 8 + off + pcm.size]
        out = torch.full((want.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        got = adaptive_vad.frame_levels(dev, fl, out=out)
        host = out.cpu().numpy()
        assert got.numel() == want.size and np.array_equal(host[:want.size], want) and np.all(host[want.size:] == SENTINEL), off
    words, nf = _native.vad_energy_bits(dev, fl, 50.0)
    raster = adaptive_vad.level_labels(got, 100, packed=True)
    assert raster.packed and raster.n == nf == want.size and torch.equal(raster.bits, words)
    labels = adaptive_vad.level_labels(got, 100, 0.1)
    assert np.array_equal(labels.cpu().numpy().view(np.uint32), ir.expected_f32(want >= 100, 0.1).view(np.uint32))


def test_chunked_sweep_equals_the_one_call_sweep(torch, native, tables):
    """Three chunks at first_frame offsets that are not multiples of 8 (37, 78) into one level vector."""
    from ffsubsync_amd import adaptive_vad

    fl = 160
    pcm, _ = vo.synth_pcm(fl * 111 + 77, seed=9, frame=fl)
    dev = _dev(torch, pcm)
    whole = adaptive_vad.frame_levels(dev, fl)
    nf = whole.numel()
    assert nf == 112
    out = torch.full((nf + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    for f0, f1 in ((0, 37), (37, 78), (78, nf)):
        adaptive_vad.frame_levels(dev[f0 * fl:min(f1 * fl, pcm.size)], fl, out=out[f0:])
    host = out.cpu().numpy()
    assert np.array_equal(host[:nf], am.frame_levels(pcm, fl, am.default_edges())) and np.all(host[nf:] == SENTINEL)
    assert torch.equal(out[:nf], whole)
    # a caller's own table, from host numbers and as a device tensor
    host_tables, dev_tables = tables
    for name in ("65", "255"):
        want = am.frame_levels(pcm, fl, host_tables[name])
        assert np.array_equal(adaptive_vad.frame_levels(dev, fl, host_tables[name]).cpu().numpy(), want)
        assert np.array_equal(adaptive_vad.frame_levels(dev, fl, dev_tables[name]).cpu().numpy(), want)


# ---- k_vad_level_hist ------------------------------------------------------------------------------------------------


def test_level_histogram(torch, native):
    """Frame counts 0 / 1 / 15 / 16 / 17, am.HIST_IDLE (a second workgroup with no work), am.HIST_TWO_TRIPS (every
    workgroup of the capped grid takes more than one trip), at bases 0, 1 and 5 bytes off a 16-byte boundary; n_bins 192,
    256 and 2; a second call on the same buffer overwrites it; nothing is written behind the n_bins counts."""
    lib, _native = native
    stream = _stream(torch, native)
    rng = np.random.RandomState(11)
    pool = rng.randint(0, 192, size=am.HIST_TWO_TRIPS + 64).astype(np.uint8)
    pool[:4096] = np.arange(4096) % 192   # every bin occupied
    wide = rng.randint(0, 256, size=5000).astype(np.uint8)
    two = rng.randint(0, 2, size=5000).astype(np.uint8)
    dev = {"pool": _dev(torch, pool), "wide": _dev(torch, wide), "two": _dev(torch, two)}
    host = {"pool": pool, "wide": wide, "two": two}
    jobs = [("pool", base, n, 192) for n in am.HIST_COUNTS for base in (0, 1, 5)]
    jobs += [("wide", 0, 5000, 256), ("wide", 3, 4997, 256), ("two", 7, 4993, 2), ("pool", 16, 100, 192)]
    slot = 256 + 8
    out = torch.full((len(jobs) * slot,), -1515870811, dtype=torch.int32, device="cuda")   # 0xA5A5A5A5
    for j, (src, base, n, n_bins) in enumerate(jobs):
        assert (dev[src].data_ptr() + base) % 16 == base % 16
        _native.check(lib.ffs_vad_level_hist(dev[src].data_ptr() + base if n else None, n, n_bins, out.data_ptr() + 4 * j * slot, stream))
    got = out.cpu().numpy().view(np.uint32).reshape(len(jobs), slot)
    for j, (src, base, n, n_bins) in enumerate(jobs):
        want = am.level_hist(host[src][base:base + n], n_bins)
        assert np.array_equal(got[j, :n_bins], want) and int(got[j, :n_bins].sum()) == n, (src, base, n, n_bins)
        assert np.all(got[j, n_bins:] == 0xA5A5A5A5), (src, base, n, n_bins)
    # the second call overwrites: the last slot again with other frames
    j = len(jobs) - 1
    _native.check(lib.ffs_vad_level_hist(dev["pool"].data_ptr() + 200, 4097, 192, out.data_ptr() + 4 * j * slot, stream))
    again = out.cpu().numpy().view(np.uint32).reshape(len(jobs), slot)[j]
    assert np.array_equal(again[:192], am.level_hist(pool[200:200 + 4097], 192)) and np.all(again[192:] == 0xA5A5A5A5)
    # a level byte of n_bins or more is counted nowhere
    from ffsubsync_amd import adaptive_vad

    h = adaptive_vad.level_hist(dev["wide"], 100).cpu().numpy()
    assert np.array_equal(h, am.level_hist(wide, 100)) and h.sum() == int((wide < 100).sum())


# ---- k_vad_pick_threshold ----------------------------------------------------------------------------------------------


def test_pick_threshold_table(torch, native):
    """Every histogram of am.pick_cases(), many per launch (one launch per parameter set): two spikes, the symmetric
    plateau, FLAT, EMPTY, totals of exactly 2^23 and 2^23 + 1, both clamps, the FLOOR count exactly at need and one short,
    n_bins 2 and 256.  Every field of every record, eta bit for bit; nothing behind the last record."""
    lib, _native = native
    stream = _stream(torch, native)
    groups = {}
    for name, h, kw in am.pick_cases():
        groups.setdefault((h.size, tuple(sorted(kw.items()))), []).append((name, h))
    seen = 0
    for (n_bins, kw), members in groups.items():
        kw = dict(kw)
        full = dict(rule=am.OTSU, lo_bin=20, t_min=21, t_max=n_bins - 1, fallback_bin=100, floor_ppm=50000, margin_bins=12)
        full.update(kw)
        hist = _dev(torch, np.stack([h for _, h in members]).astype(np.uint32).view(np.int32))
        out = torch.full((len(members) * 48 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        _native.check(lib.ffs_vad_pick_threshold(hist.data_ptr(), len(members), n_bins, full["rule"], full["lo_bin"], full["t_min"],
                                                 full["t_max"], full["fallback_bin"], full["floor_ppm"], full["margin_bins"],
                                                 out.data_ptr(), stream))
        raw = out.cpu().numpy()
        rows = raw[:len(members) * 48].view(_native.VAD_THRESHOLD_DTYPE)
        assert np.all(raw[len(members) * 48:] == SENTINEL)
        for (name, h), row in zip(members, rows):
            want = am.pick(h, **full)
            got = tuple(int(row[f]) for f in am.FIELDS[:-1]) + (int(row["eta"].view(np.uint64)),)
            assert got == am.record_tuple(want), (name, got, want)
            seen += 1
    assert seen == len(am.pick_cases())


def test_pick_threshold_wrapper_and_device_threshold(torch, native):
    """pick_threshold on one histogram and on a stack; the record tensor handed to level_labels as the threshold."""
    from ffsubsync_amd import adaptive_vad

    cases = [(n, h) for n, h, kw in am.pick_cases() if h.size == 192 and not kw]
    stack = _dev(torch, np.stack([h for _, h in cases]).view(np.int32))
    recs = adaptive_vad.pick_threshold(stack, "otsu", lo_bin=20, floor_ppm=50000, margin_bins=12)
    one = adaptive_vad.pick_threshold(stack[0], "otsu", lo_bin=20, floor_ppm=50000, margin_bins=12)
    assert isinstance(recs, list) and len(recs) == len(cases) and one == recs[0]
    for (name, h), rec in zip(cases, recs):
        want = am.pick(h)
        assert [getattr(rec, f) for f in am.FIELDS] == [want[f] for f in am.FIELDS], name
    floor = adaptive_vad.pick_threshold(stack[0], "FLOOR ", lo_bin=20, floor_ppm=50000, margin_bins=12)
    assert floor.threshold_bin == am.pick(cases[0][1], rule=am.FLOOR)["threshold_bin"]


# ---- k_vad_level_labels ------------------------------------------------------------------------------------------------


def test_level_labels(torch, native):
    """n = 1 / 7 / 8 / 9 / 63 / 64 / 65 / 300; thresholds 0 (all speech), 192 (none), 256 and one in between; the threshold
    from a record on the device and from the host value; both output forms in one call and each alone; labels float32
    cannot hold; the unused high bits of the last byte 0; sentinels intact."""
    lib, _native = native
    stream = _stream(torch, native)
    rng = np.random.RandomState(12)
    levels = rng.randint(0, 192, size=400).astype(np.uint8)
    levels[:16] = [0, 191, 100, 99, 101, 100, 0, 191, 100, 99, 1, 2, 100, 100, 99, 191]
    dev = _dev(torch, levels)
    records = np.zeros(3, _native.VAD_THRESHOLD_DTYPE)
    records["threshold_bin"] = [100, 0, 192]
    records["flags"] = 77   # a reader that takes the wrong field sees it
    rec_dev = _dev(torch, records.view(np.uint8))
    jobs = []
    for n in (1, 7, 8, 9, 63, 64, 65, 300):
        for k, (thr_dev, thr) in enumerate(((None, 100), (None, 0), (None, 192), (None, 256), (0, 100), (1, 0), (2, 192))):
            jobs.append((n, (n + k) % 5, thr_dev, thr, (0.1, 0.0, -1.0, 0.7)[k % 4], ("both", "labels", "bits")[(n + k) % 3]))
    f_slot, b_slot = 300 + 4, 38 + 8
    f_out = torch.full((len(jobs) * f_slot,), -7.0, dtype=torch.float32, device="cuda")
    b_out = torch.full((len(jobs) * b_slot,), SENTINEL, dtype=torch.uint8, device="cuda")
    for j, (n, off, thr_dev, thr, label, form) in enumerate(jobs):
        _native.check(lib.ffs_vad_level_labels(
            dev.data_ptr() + off, n, None if thr_dev is None else rec_dev.data_ptr() + 48 * thr_dev, thr if thr_dev is None else -5, label,
            f_out.data_ptr() + 4 * j * f_slot if form != "bits" else None, b_out.data_ptr() + j * b_slot if form != "labels" else None,
            stream))
    f_host, b_host = f_out.cpu().numpy().reshape(len(jobs), f_slot), b_out.cpu().numpy().reshape(len(jobs), b_slot)
    for j, (n, off, thr_dev, thr, label, form) in enumerate(jobs):
        speech = am.speech(levels[off:off + n], thr)
        assert speech.all() if thr == 0 else not speech.any() if thr >= 192 else True
        nb = (n + 7) // 8
        nf_written, nb_written = (n if form != "bits" else 0), (nb if form != "labels" else 0)
        if form != "bits":
            assert np.array_equal(f_host[j, :n].view(np.uint32), ir.expected_f32(speech, label).view(np.uint32)), jobs[j]
        if form != "labels":
            assert np.array_equal(b_host[j, :nb], ir.expected_bits(speech)), jobs[j]
        assert np.all(f_host[j, nf_written:] == -7.0) and np.all(b_host[j, nb_written:] == SENTINEL), jobs[j]


# ---- end to end ----------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def stream_source(torch):
    src = ir.stream_source()
    return src, torch.from_numpy(src).pin_memory(), {}


def _shipped():
    """The package's shipped defaults as arguments of the model's pick."""
    from ffsubsync_amd import adaptive_vad as av

    return dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, fallback_bin=100,
                floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)


def _model(cache, src, n, frame_rate):
    if frame_rate not in cache:
        cache[frame_rate] = am.detect(src[:n], vo.frame_len(100, frame_rate), **_shipped())
    return cache[frame_rate]


def _same_record(rec, want):
    return [getattr(rec, f) for f in am.FIELDS[:-1]] == [want[f] for f in am.FIELDS[:-1]] and \
        np.float64(rec.eta).view(np.uint64) == np.float64(want["eta"]).view(np.uint64)


@pytest.mark.parametrize("frame_rate", ir.STREAM_RATES)
def test_whole_file_entries_equal_the_model(torch, stream_source, frame_rate):
    """detect_device_adaptive and detect_pinned_stream_adaptive (five whole 100 s buffers and a short last one that is not
    a multiple of the frame length) with the shipped defaults: the model's labels and record, fp32 and packed."""
    from ffsubsync_amd import adaptive_vad

    src, pinned, cache = stream_source
    n = ir.stream_samples(frame_rate)
    speech, want, _ = _model(cache, src, n, frame_rate)
    assert 0 < speech.sum() < speech.size and not want["flags"]
    dev = pinned[:n].cuda()
    for labels, rec in (adaptive_vad.detect_device_adaptive(dev, 100, frame_rate, 0.1),
                        adaptive_vad.detect_pinned_stream_adaptive(pinned[:n], 100, frame_rate, 0.1)):
        assert _same_record(rec, want), (rec, want)
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy().view(np.uint32), ir.expected_f32(speech, 0.1).view(np.uint32))
    for raster, rec in (adaptive_vad.detect_device_adaptive(dev, 100, frame_rate, 0.1, packed=True),
                        adaptive_vad.detect_pinned_stream_adaptive(pinned[:n], 100, frame_rate, 0.1, packed=True)):
        assert _same_record(rec, want) and raster.packed and raster.n == speech.size and (raster.lo, raster.hi) == (0.1, 1.0)
        words, bits = raster.bits.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
        assert np.array_equal(words[:bits.size], bits) and not words[bits.size:].any()
    assert adaptive_vad.threshold_db(rec) == pytest.approx(10.0 * np.log10(am.default_edges()[want["threshold_bin"] - 1]), rel=1e-12)


def test_whole_file_entries_on_a_side_stream(torch, stream_source):
    """Both entries and the four calls queued by hand on a non-default stream with no synchronisation between them, the
    floor rule and a caller's parameters, the results consumed on that stream."""
    from ffsubsync_amd import adaptive_vad

    src, pinned, _ = stream_source
    rate, fl = 16000, 160
    n = 3 * fl * 10000 + 777
    args = dict(lo_bin=20, t_min=30, t_max=150, fallback_bin=90, floor_ppm=100000, margin_bins=20)
    speech, want, levels = am.detect(src[1000:1000 + n], fl, rule=am.FLOOR, **args)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = pinned[1000:1000 + n].cuda(non_blocking=True)
        a, rec_a = adaptive_vad.detect_pinned_stream_adaptive(pinned[1000:1000 + n], 100, rate, -1.0, rule="floor", **args)
        b, rec_b = adaptive_vad.detect_device_adaptive(dev, 100, rate, -1.0, rule="floor", **args)
        lv = adaptive_vad.frame_levels(dev, fl)
        raw = adaptive_vad.pick_threshold_device(adaptive_vad.level_hist(lv), "floor", **args)
        c = adaptive_vad.level_labels(lv, raw, -1.0)
        taken = [t.clone() for t in (a, b, c, lv)]
    side.synchronize()
    assert _same_record(rec_a, want) and _same_record(rec_b, want) and 0 < speech.sum() < speech.size
    for t in taken[:3]:
        assert np.array_equal(t.cpu().numpy().view(np.uint32), ir.expected_f32(speech, -1.0).view(np.uint32))
    assert np.array_equal(taken[3].cpu().numpy(), levels)


def test_speech_transformer_adaptive_returns_the_label_itself_in_float64(torch, stream_source):
    """PCMSpeechTransformer(vad="adaptive") from an array, from bytes and from a file object: float64, exactly
    non_speech_label where the frame is not speech, one threshold for the whole stream (two chunks and a short tail)."""
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer

    src, _, _ = stream_source
    pcm = src[: 480 * 12000 + 77]
    speech, want, _ = am.detect(pcm, 480, **_shipped())
    for label, source in ((0.1, pcm), (0.7, pcm.tobytes()), (0.1, io.BytesIO(pcm.tobytes()))):
        t = PCMSpeechTransformer("adaptive", 100, 48000, non_speech_label=label).fit(source)
        got = t.transform()
        assert got.dtype == np.float64 and np.array_equal(got, np.where(speech, 1.0, label)), label
        assert set(np.unique(got)) == {label, 1.0} and _same_record(t.vad_threshold_, want)
    with pytest.raises(ValueError, match="Unable to detect speech"):
        PCMSpeechTransformer("adaptive", 100, 48000).fit(b"")


def test_quiet_file_keeps_its_labels(torch):
    """The point of the feature on the device: a file scaled down by 30 dB (integer-exact: speech x 32 -> x 1) keeps
    the adaptive labels, and the fixed 50 dB rule finds nothing in it."""
    from ffsubsync_amd import _native, adaptive_vad

    fl, files = am.gain_files()
    loud, quiet = files[0], files[-30]
    a, rec_a = adaptive_vad.detect_device_adaptive(_dev(torch, loud), 100, 100 * fl, 0.0)
    b, rec_b = adaptive_vad.detect_device_adaptive(_dev(torch, quiet), 100, 100 * fl, 0.0)
    assert torch.equal(a, b) and 0 < float(a.sum()) < a.numel() and not (rec_a.flags or rec_b.flags)
    assert float(_native.vad_energy(_dev(torch, quiet), fl, 50.0, 0.0).sum()) == 0.0


# ---- refusals ------------------------------------------------------------------------------------------------------


def test_refusals_of_each_export(torch, native):
    am.check_refusals(native[0])
