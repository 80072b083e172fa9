"""The ingest kernels -- everything between decoded PCM and the vector the aligner reads -- against the plain exact
references of tests/ingest_reference.py, over frame lengths, alignments, tails, thresholds, labels and edges instead
of one point of each: k_vad_energy (both output forms), detect_pinned_stream, both tokenizer kernels, k_speech_bounds
and fit_boundaries, k_pack_bits, k_scatter_segments and assemble_sparse_reference.

Equality is bit for bit everywhere except the tokenizer at labels float32 cannot hold, whose bound
(cm + 1) * 2^-23 is derived in ingest_reference.token_bound.  tests/test_ingest_reference_host.py asserts, on the same
builders, that no frame of the energy sweep is ambiguous and that every branch of the kernels is visited.
VAD parity with auditok itself stays unpinned: the expected values are restatements and exact arithmetic."""
import numpy as np
import pytest

import ingest_reference as ir
from oracle import vad_oracle as vo

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_equal(a, b):
    """float32 arrays equal bit for bit (tells -0.0 from 0.0, and NaNs by payload)."""
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- k_vad_energy ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("frame_len", ir.FRAME_LENS)
def test_frame_energy_sweep(torch, frame_len):
    """ffs_vad_energy / ffs_vad_energy_bits through the C ABI on every case of ingest_reference.energy_cases: vector
    widths of 1 .. 64 lanes, the element loop in 1 .. 10 rounds, start offsets of 0, 1, 3 and 8 samples, every residue
    of the frame count mod 8 with tails of none, one and frame_len - 1 samples, thresholds of 0 .. 90 dB with frames
    exactly at, one below and one above the threshold, full-scale frames, labels float32 cannot hold.  fp32 labels
    equal float32(label) / 1.0 bit for bit; the packed form equals packbits with the unused bits of the last byte 0;
    neither writes behind its last frame (sentinels)."""
    from ffsubsync_amd import _native

    lib, stream = _native.load(), _native.current_stream_ptr(torch)
    cases = list(ir.energy_cases(frame_len))
    # the outputs of all cases side by side in two device buffers (sentinels between them), read back once
    f_at, b_at, nf_total, nb_total = [], [], 0, 0
    for c in cases:
        nf = -(-c["n_samples"] // frame_len)
        f_at.append(nf_total)
        b_at.append(nb_total)
        nf_total += nf + 4
        nb_total += (nf + 7) // 8 + 8
    f_out = torch.full((nf_total,), -7.0, dtype=torch.float32, device="cuda")
    b_out = torch.full((nb_total,), SENTINEL, dtype=torch.uint8, device="cuda")
    uploaded = {}
    for c, fo, bo in zip(cases, f_at, b_at):
        if id(c["buffer"]) not in uploaded:
            uploaded[id(c["buffer"])] = _dev(torch, c["buffer"])
        pcm = uploaded[id(c["buffer"])][c["offset"]:]
        assert pcm.data_ptr() % 16 == (2 * c["offset"]) % 16
        _native.check(lib.ffs_vad_energy(pcm.data_ptr(), c["n_samples"], frame_len, c["threshold"], c["label"],
                                         f_out.data_ptr() + 4 * fo, stream))
        _native.check(lib.ffs_vad_energy_bits(pcm.data_ptr(), c["n_samples"], frame_len, c["threshold"],
                                              b_out.data_ptr() + bo, stream))
    f_host, b_host = f_out.cpu().numpy(), b_out.cpu().numpy()
    for c, fo, bo in zip(cases, f_at, b_at):
        speech, _ = ir.energy_labels(ir.case_pcm(c), frame_len, c["threshold"])
        nf, nb = speech.size, (speech.size + 7) // 8
        what = (frame_len, c["threshold"], c["offset"], c["n_samples"], c["label"])
        assert _bits_equal(f_host[fo:fo + nf], ir.expected_f32(speech, c["label"])), what
        assert np.all(f_host[fo + nf:fo + nf + 4] == -7.0), what
        assert np.array_equal(b_host[bo:bo + nb], ir.expected_bits(speech)), what
        assert np.all(b_host[bo + nb:bo + nb + 8] == SENTINEL), what


def test_frame_energy_grid_stride_trip(torch):
    """More than 524 288 frames: the waves of k_vad_energy's capped grid take a second trip.  Both output forms."""
    from ffsubsync_amd import _native

    pcm, fl = ir.grid_stride_pcm(), ir.GRID_STRIDE_FRAME_LEN
    speech, _ = ir.energy_labels(pcm, fl, 50.0)
    for off in (0, 1):   # the vector path and the element path
        dev = _dev(torch, np.concatenate([np.full(8 + off, 32767, np.int16), pcm, np.full(64, -32768, np.int16)]))
        dev = dev[8 + off: 8 + off + pcm.size]
        got = _native.vad_energy(dev, fl, 50.0, 0.1).cpu().numpy()
        assert _bits_equal(got, ir.expected_f32(speech, 0.1)), off
        nb = (speech.size + 7) // 8
        out = torch.full((nb + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        _, nf = _native.vad_energy_bits(dev, fl, 50.0, out=out)
        host = out.cpu().numpy()
        assert nf == speech.size and np.array_equal(host[:nb], ir.expected_bits(speech)), off
        assert np.all(host[nb:] == SENTINEL), off


# ---- detect_pinned_stream and the detectors ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def stream_source(torch):
    src = ir.stream_source()
    return src, torch.from_numpy(src).pin_memory()


@pytest.mark.parametrize("frame_rate", ir.STREAM_RATES)
def test_detect_pinned_stream_equals_the_chunk_loop(torch, stream_source, frame_rate):
    """Five whole 100 s buffers (each of the function's two staging buffers is reused twice) and a short last one that
    is not a multiple of the frame length, against vo.chunked_detect, bit for bit, fp32 and packed."""
    from ffsubsync_amd.speech_transformers import detect_pinned_stream

    src, pinned = stream_source
    n = ir.stream_samples(frame_rate)
    want = vo.chunked_detect(src[:n], 100, frame_rate, non_speech_label=0.1)
    speech = want == 1.0
    got = detect_pinned_stream(pinned[:n], 100, frame_rate, 0.1)
    assert got.is_cuda and _bits_equal(got.cpu().numpy(), ir.expected_f32(speech, 0.1))
    raster = detect_pinned_stream(pinned[:n], 100, frame_rate, 0.1, packed=True)
    assert raster.packed and raster.n == want.size and (raster.lo, raster.hi) == (0.1, 1.0)
    words, bits = raster.bits.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
    assert words.size == (want.size + 31) // 32 * 4
    assert np.array_equal(words[:bits.size], bits) and not words[bits.size:].any()
    assert np.array_equal(np.asarray(raster), want)


def test_detect_pinned_stream_reuses_a_callers_staging_on_a_side_stream(torch, stream_source):
    """A caller's staging buffers and copy stream reused for three files of different length back to back, issued from
    a non-default stream with no synchronisation in between, the results consumed on that stream."""
    from ffsubsync_amd.speech_transformers import detect_pinned_stream

    src, pinned = stream_source
    rate, fl = 16000, 160
    chunk = fl * 10000
    files = [(0, ir.stream_samples(rate), 0.1, False), (1000, 3 * chunk + 777, -1.0, True), (37, 2 * chunk + 1, 0.7, False),
             (5, chunk - 3, 0.0, True)]
    staging = ([torch.empty(chunk, dtype=torch.int16, device="cuda") for _ in range(2)], torch.cuda.Stream())
    side = torch.cuda.Stream()
    taken = []
    with torch.cuda.stream(side):
        for o, n, label, packed in files:
            out = detect_pinned_stream(pinned[o:o + n], 100, rate, label, staging=staging, packed=packed)
            taken.append((out.bits if packed else out).clone())   # consumed on the issuing stream
    side.synchronize()
    for (o, n, label, packed), got in zip(files, taken):
        want = vo.chunked_detect(src[o:o + n], 100, rate, non_speech_label=label)
        speech = want == 1.0
        if packed:
            words, bits = got.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
            assert np.array_equal(words[:bits.size], bits) and not words[bits.size:].any(), (o, n)
        else:
            assert _bits_equal(got.cpu().numpy(), ir.expected_f32(speech, label)), (o, n)


def test_detectors_return_the_label_itself_in_float64(torch, stream_source):
    """The reference's detector factory returns exactly non_speech_label (speech_transformers.py:133-150), not its
    float32 rounding: 0.1 and 0.7 (which is above 0.5) through the detector closure and the pipelined chunk loop."""
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer, _make_energy_detector

    src, _ = stream_source
    pcm = src[: 480 * 12000 + 77]
    for label in (0.1, 0.7):
        got = _make_energy_detector(100, 48000, label)(pcm[:4800000].tobytes())
        want = vo.detect_fast(pcm[:4800000], non_speech_label=label)
        assert got.dtype == np.float64 and np.array_equal(got, want), label
        assert set(np.unique(got)) == {label, 1.0}
    t = PCMSpeechTransformer("energy", 100, 48000, non_speech_label=0.1).fit(pcm)
    want = vo.chunked_detect(pcm, non_speech_label=0.1)
    assert t.transform().dtype == np.float64 and np.array_equal(t.transform(), want)


# ---- tokenizer ---------------------------------------------------------------------------------------------------


def test_tokenizer_at_labels_float32_cannot_hold(torch):
    """The existing validity patterns and parameter cases on chunks served by each kernel.  Dyadic labels: the float64
    restatement bit for bit.  Labels float32 cannot hold: within the derived bound (cm + 1) * 2^-23 of the float64
    restatement -- and, what the header states, equal to float32(clip(cp + cm (float64(float32(l)) - 1), 0, 1)) bit
    for bit, from either kernel."""
    from ffsubsync_amd import _native

    labels = ir.DYADIC_LABELS + ir.NON_DYADIC_LABELS
    served = {False: 0, True: 0}
    for valid, case in ir.token_inputs():
        dev = _dev(torch, valid.astype(np.float32))
        for chunk in ir.TOKEN_CHUNKS:
            want, cp, cm = ir.tokenize_f64(valid, labels, chunk, case)
            served[ir.serial_kernel_serves(valid.size, chunk, case)] += 1
            for label in labels:
                got = _native.vad_tokenize(dev, chunk, *case, label).cpu().numpy()
                what = (valid.size, case, chunk, label)
                if label in ir.DYADIC_LABELS:
                    assert np.array_equal(got.astype(np.float64), want[label]), what
                err = np.abs(got.astype(np.float64) - want[label])
                worst = float(np.max(err / ir.token_bound(cm)))
                assert worst <= 1.0, what + (worst,)
                assert _bits_equal(got, ir.token_model(cp, cm, label)), what
    assert served[False] and served[True]


def test_both_tokenizer_kernels_on_identical_input(torch):
    """min_length = 0 selects the workgroup kernel and min_length = -1 the serial one, with the same meaning
    (len >= min_length always holds): outputs identical bit for bit, for every label."""
    from ffsubsync_amd import _native

    rng = np.random.RandomState(5)
    labels = ir.DYADIC_LABELS + ir.NON_DYADIC_LABELS
    shapes = [(1, 10000), (64, 10000), (257, 997), (3000, 997), (10000, 997), (10000, 10000), (28672, 28672)]
    for n, chunk in shapes:
        valid = ir.validity_pattern(rng, n)
        dev = _dev(torch, valid.astype(np.float32))
        for j, (mx, msil) in enumerate(((500, 25), (7, 0), (40, 30), (3, -1))):
            for label in (labels if j == 0 and chunk <= 10000 else labels[2:5]):
                scan = _native.vad_tokenize(dev, chunk, 0, mx, msil, label)
                serial = _native.vad_tokenize(dev, chunk, -1, mx, msil, label)
                assert torch.equal(scan.view(torch.int32), serial.view(torch.int32)), (n, chunk, mx, msil, label)


def test_auditok_detector_at_30_frames_per_second(torch):
    """_make_auditok_detector at sample_rate 30 against vo._Tokenizer(0.2 * 30, 150, 0.25 * 30) with the floats left as
    floats: a silence counter reaches 7.5 at 8 frames, so the wrapper's ceil is the point (the input tells 8 from 7,
    see the host test); frame_len is 1600 there -- the element path in four rounds."""
    from ffsubsync_amd.speech_transformers import _make_auditok_detector

    pcm, _ = ir.auditok30_pcm()
    sample_rate, frame_rate = ir.AUDITOK30
    speech, _ = ir.energy_labels(pcm, vo.frame_len(sample_rate, frame_rate), 50.0)
    tokens = vo._Tokenizer(0.2 * sample_rate, int(5 * sample_rate), 0.25 * sample_rate).tokenize(speech)
    for label in (0.0, -1.0):
        got = _make_auditok_detector(sample_rate, frame_rate, label)(pcm.tobytes())
        assert got.dtype == np.float64 and np.array_equal(got, ir.rasterise_tokens(speech.size, tokens, label)), label


# ---- k_speech_bounds / fit_boundaries ----------------------------------------------------------------------------------


@pytest.mark.parametrize("n", ir.BOUNDS_LENGTHS)
def test_speech_bounds(torch, n):
    """Lengths around the wave, the block and the grid (131 072 threads: the grid-stride trip starts there); no speech,
    all speech, single speech frames at both ends, in the middle and at index 131 072; 0.5 and its float32 neighbours,
    NaN and infinities.  Expected: np.nonzero(x > 0.5) on the float32 array."""
    from ffsubsync_amd import _native

    for name, x in ir.bounds_patterns(n):
        assert _native.speech_bounds(_dev(torch, x)) == ir.fit_boundaries(x), (n, name)


def test_fit_boundaries_compares_in_the_callers_precision(torch):
    """speech_transformers.py:310-317 compares the caller's array with 0.5: a float64 value just above 0.5 is speech
    although it rounds to float32(0.5).  Host arrays, CUDA tensors and DeviceRaster levels."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.speech_transformers import ComputeSpeechFrameBoundariesMixin as Mixin
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    just_above = float(np.nextafter(0.5, 1.0))
    x = np.full(1000, 0.5)
    x[17], x[400], x[900], x[950], x[960] = just_above, 1.0, 0.5 + 2.0 ** -30, np.nextafter(0.5, 0.0), np.nan
    assert ir.fit_boundaries(x) == (17, 900) and ir.fit_boundaries(x.astype(np.float32)) == (400, 400)
    for frames in (x, x.tolist(), torch.from_numpy(x).cuda()):
        m = Mixin().fit_boundaries(frames)
        assert (m.start_frame_, m.end_frame_, m.num_frames) == (17, 900, 883), type(frames)
    for frames in (x.astype(np.float32), torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(x).cuda().half()):
        m = Mixin().fit_boundaries(frames)
        assert (m.start_frame_, m.end_frame_) == (400, 400), type(frames)
    z = Mixin().fit_boundaries(np.full(100, 0.5))
    assert z.start_frame_ is None and z.end_frame_ is None and z.num_frames is None
    bits = np.zeros(1000, np.uint8)
    bits[[17, 900]] = 1
    dev = _dev(torch, bits)
    for lo, hi in ((0.0, just_above), (0.5, just_above), (0.0, 0.5), (just_above, 0.5), (0.25, 1.0)):
        for raster in (DeviceRaster(dev, lo, hi), DeviceRaster(_native.pack_bits(dev), lo, hi, 1000)):
            want = ir.fit_boundaries(np.asarray(raster))
            m = Mixin().fit_boundaries(raster)
            assert (m.start_frame_, m.end_frame_) == want, (lo, hi, raster.packed)
    assert ir.fit_boundaries(np.asarray(DeviceRaster(dev, 0.0, just_above))) == (17, 900)
    assert ir.fit_boundaries(np.asarray(DeviceRaster(dev, just_above, 0.5))) == (0, 999)


# ---- k_pack_bits ---------------------------------------------------------------------------------------------------

PACK_LENGTHS = (1, 31, 32, 33, 8191, 8192, 8193, 3 * 8192 + 31)   # around a word and around a block (256 words)


def test_pack_bits_bytes(torch):
    """U8 sources with values 0, 1, 2, 128, 255 at source offsets 0-3; the unused bits of the last word are 0."""
    from ffsubsync_amd import _native

    rng = np.random.RandomState(2)
    values = np.array([0, 1, 2, 128, 255], np.uint8)
    for n in PACK_LENGTHS:
        buf = values[rng.choice(5, n + 3, p=[0.6, 0.1, 0.1, 0.1, 0.1])]
        dev = _dev(torch, buf)
        for off in range(4):
            got = _native.pack_bits(dev[off:off + n]).view(torch.uint8).cpu().numpy()
            assert np.array_equal(got, ir.pack_bits(buf[off:off + n])), (n, off)


def test_pack_bits_floats_against_the_double_threshold(torch):
    """bit = (x > threshold) with the threshold a double: samples at float32(threshold) and its float32 neighbours on
    both sides, NaN and infinities, thresholds float32 cannot hold.  Expected: the float64 comparison."""
    from ffsubsync_amd import _native

    rng = np.random.RandomState(3)
    for thr in (0.5, 0.1, 0.48, -0.25, 0.0):
        t = np.float32(thr)
        up, down = np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))
        values = np.array([t, up, down, np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf)),
                           np.nan, np.inf, -np.inf, 0.0, 1.0, -1.0], np.float32)
        for n in PACK_LENGTHS:
            x = values[rng.choice(values.size, n)]
            if n >= values.size:
                x[: values.size] = values
            got = _native.pack_bits(_dev(torch, x), thr).view(torch.uint8).cpu().numpy()
            assert np.array_equal(got, ir.pack_bits(x, thr)), (thr, n)
    # a threshold beyond float32's range, and a NaN threshold
    x = np.array([np.inf, 3.4e38, -np.inf, np.nan, 0.0], np.float32)
    for thr in (1e300, -1e300, float("nan"), float("inf")):
        got = _native.pack_bits(_dev(torch, x), thr).view(torch.uint8).cpu().numpy()
        assert np.array_equal(got, ir.pack_bits(x, thr)), thr


def test_pack_bits_grid_stride_trip(torch):
    """2^29 + 12 345 bytes generated on the device (0.5 GB): k_pack_bits' capped grid (65 536 blocks x 256 words x 32
    samples = 2^29) takes a second trip.  Checked against a torch packing of the same tensor."""
    from ffsubsync_amd import _native

    n = 2 ** 29 + 12345
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    x = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    x = x * (x > 150)
    words = _native.pack_bits(x)
    assert words.numel() == (n + 31) // 32
    flags = torch.cat([x != 0, torch.zeros(-n % 32, dtype=torch.bool, device="cuda")]).view(-1, 8).to(torch.uint8)
    del x
    want = flags[:, 0].clone()
    for k in range(1, 8):
        want |= flags[:, k] << k
    assert want.numel() == 4 * words.numel() and 0.3 < float(flags[-100000:].float().mean()) < 0.5
    assert torch.equal(words.view(torch.uint8), want)


# ---- k_scatter_segments / assemble_sparse_reference ------------------------------------------------------------------------


def _scatter_cases():
    """(name, segment lengths, destination starts, out_len): windows that do not overlap inside [0, out_len)."""
    rng = np.random.RandomState(4)
    for count in (0, 1, 31, 32, 33, 70):
        lens = rng.randint(0, 40, count)
        lens[::7] = 0
        lens[1::5] = 1
        gaps = rng.randint(0, 6, count)
        dst = np.cumsum(gaps + np.concatenate([[0], lens[:-1]])) if count else np.zeros(0, int)
        out_len = int(dst[-1] + lens[-1] // 2 + 1) if count else 50   # the last window is clipped
        yield "%d windows" % count, lens, dst, out_len
    yield "long window", np.array([5, 300000, 9]), np.array([0, 10, 300020]), 300025
    yield "long window clipped", np.array([300000, 3]), np.array([7, 0]), 262144 + 300
    out_len = 1000
    yield "at the end", np.array([5, 4, 6, 2, 1]), np.array([out_len - 1, out_len, out_len + 10, 10, 0]), out_len
    yield "out_len 1", np.array([1, 3, 0, 2]), np.array([0, 1, 0, 5]), 1
    yield "out_len 1, clipped", np.array([4]), np.array([0]), 1


def _segments(rng, lens):
    return [rng.choice(np.array([0.0, 0.25, 1.0, -1.0, 0.1], np.float32), int(n)) for n in lens]


def test_scatter_segments_through_the_c_abi(torch):
    """0, 1, 31, 32, 33 and 70 windows (SCATTER_MAX = 32 per launch); lengths 0, 1 and 300 000 (beyond the 262 144
    threads of a launch); windows that start at out_len - 1, at out_len and beyond; a non-zero src_off; out_len 1.
    Expected: the reference's loop."""
    from ffsubsync_amd import _native

    rng = np.random.RandomState(6)
    for name, lens, dst, out_len in _scatter_cases():
        segs = _segments(rng, lens)
        parts, src_off, pos = [np.full(5, 9.0, np.float32)], [], 5
        for s in segs:   # the windows' labels with junk in front of, between and behind them
            src_off.append(pos)
            parts += [s, np.full(3, 9.0, np.float32)]
            pos += s.size + 3
        labels = _dev(torch, np.concatenate(parts))
        got = _native.scatter_segments(labels, np.array(src_off, np.int64), dst, lens, out_len).cpu().numpy()
        assert _bits_equal(got, ir.scatter(segs, dst, out_len).astype(np.float32)), name


def test_assemble_sparse_reference_orders_overlapping_windows(torch):
    """The same window sets through assemble_sparse_reference, and chains of overlaps (A meets B, B meets C, A does not
    meet C) given in every order: the later window wins, as in the reference's loop."""
    import itertools

    from ffsubsync_amd.speech_transformers import assemble_sparse_reference

    rng = np.random.RandomState(8)

    def check(name, segs, dst, out_len):
        want = ir.scatter(segs, dst, out_len).astype(np.float32)
        tensors = [_dev(torch, s) for s in segs]
        if not np.any(want > 0):
            with pytest.raises(ValueError, match="Unable to detect speech in any sampled segment"):
                assemble_sparse_reference(tensors, [float(d) for d in dst], float(out_len - 2), 1)
            return
        got = assemble_sparse_reference(tensors, [float(d) for d in dst], float(out_len - 2), 1).cpu().numpy()
        assert _bits_equal(got, want), name

    for name, lens, dst, out_len in _scatter_cases():
        if out_len >= 2:   # out_len = int(total_duration * sample_rate) + 2
            check(name, _segments(rng, lens), dst, out_len)
    chain = [(100, 100), (180, 120), (290, 110), (395, 30), (50, 10)]   # (start, length): A-B, B-C, C-D overlap
    for order in itertools.permutations(range(len(chain))):
        dst = np.array([chain[i][0] for i in order])
        segs = [np.full(chain[i][1], float(i + 1) / 8, np.float32) for i in order]
        check("chain %s" % (order,), segs, dst, 420)
    # many windows, each overlapping its neighbours, shuffled: more runs than one launch holds windows
    starts = rng.permutation(70) * 10
    segs = [rng.choice(np.array([0.0, 0.25, 1.0], np.float32), 25) for _ in starts]
    check("70 overlapping", segs, starts, 700)
