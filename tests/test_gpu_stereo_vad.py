"""The centre-channel VAD (ffs_vad_stereo_levels, ffs_vad_centre_gate, adaptive_vad.stereo_levels / centre_gate /
detect_*_centre, PCMSpeechTransformer(vad="centre" / "centre_steady")) against tests/stereo_vad_model.py,
bit for bit: levels, gated levels, every field of the record and every guard byte around the caller's outputs.  Many
cases share one buffer with sentinels between them and are read back once.  The rule has no upstream counterpart: the
model is the only reference (tests/test_stereo_vad_host.py pins its identities and the conditions on these inputs)."""
import io

import numpy as np
import pytest

import adaptive_vad_model as am
import ingest_reference as ir
import steady_gate_model as gm
import stereo_vad_model as sm

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def native(torch):
    from ffsubsync_amd import _native

    return _native.load(), _native


@pytest.fixture(scope="module")
def tables(torch):
    host = am.edge_tables()
    return host, {name: torch.from_numpy(e).cuda() for name, e in host.items()}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the sweep ---------------------------------------------------------------------------------------------------------


def test_vector_path_limits_are_the_kernels_constants(native):
    """The largest frame length of the vector path and one vector more, by the kernel's constants: both are swept below."""
    _native = native[1]
    assert sm.MAX_FRAME_VEC == _native.VAD_STEREO_MAX_FRAME_VEC == 512 and sm.ONE_VECTOR_MORE == sm.MAX_FRAME_VEC + 4 == 516
    assert {1, 3, 4, 5, 160, 480, 512, 516, sm.MAX_FRAME_VEC, sm.ONE_VECTOR_MORE} == set(sm.FRAME_LENS)


@pytest.mark.parametrize("frame_len", sm.FRAME_LENS)
def test_sweep_against_the_model(torch, native, tables, frame_len):
    """sm.sweep_cases: the PCM 0, 2, 4 and 8 bytes behind a 16-byte boundary, 0, 1 and 40 .. 47 whole frames, tails of
    none, one pair and frame_len - 1 pairs, each output 0, 1 and 3 bytes behind an 8-byte boundary, tables of 1, 64, 65,
    255 and the default 191 edges; the pool holds frames exactly at, one below and one above a decade edge in M and in S,
    and the three full-scale frames.  One output buffer, sentinels between the slots, one read-back."""
    lib, _native = native
    host_tables, dev_tables = tables
    bufs = sm.sweep_buffers(frame_len)
    cases = list(sm.sweep_cases(frame_len))
    # every offset's buffer at a 16-byte boundary of one allocation
    at, pos = {}, 0
    for off, b in bufs.items():
        at[off] = pos
        pos += (b.size + 7) // 8 * 8
    host = np.zeros(pos, np.int16)
    for off, b in bufs.items():
        host[at[off]:at[off] + b.size] = b
    pcm = _dev(torch, host)
    assert pcm.data_ptr() % 16 == 0
    opos = 0
    for c in cases:
        n_frames = -(-c["n_pairs"] // frame_len)
        opos = (opos + 7) // 8 * 8 + 8
        c["mid_at"] = opos + c["mid_off"]
        opos = (c["mid_at"] + n_frames + 7) // 8 * 8 + 8
        c["side_at"] = opos + c["side_off"]
        opos = c["side_at"] + n_frames
    out = torch.full((opos + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 8 == 0
    stream = _native.current_stream_ptr(torch)
    for c in cases:
        e = dev_tables[c["table"]]
        n = c["n_pairs"]
        _native.check(lib.ffs_vad_stereo_levels(pcm.data_ptr() + 2 * (at[c["offset"]] + c["offset"]), n, frame_len, e.data_ptr(),
                                                int(e.numel()), out.data_ptr() + c["mid_at"] if n else None,
                                                out.data_ptr() + c["side_at"] if n else None, stream))
    got = out.cpu().numpy()
    covered = np.zeros(got.size, bool)
    for c in cases:
        mid, side = sm.stereo_levels(sm.case_pcm(bufs, c), frame_len, host_tables[c["table"]])
        what = (frame_len, c["offset"], c["n_pairs"], c["table"], c["mid_off"], c["side_off"])
        assert np.array_equal(got[c["mid_at"]:c["mid_at"] + mid.size], mid), what
        assert np.array_equal(got[c["side_at"]:c["side_at"] + side.size], side), what
        covered[c["mid_at"]:c["mid_at"] + mid.size] = covered[c["side_at"]:c["side_at"] + side.size] = True
    assert np.all(got[~covered] == SENTINEL)
    assert np.array_equal(pcm.cpu().numpy(), host)


def test_grid_stride_second_trip(torch, native, tables):
    """More frames of 4 pairs than one trip of the capped grid covers (under 9 MB), a short last frame."""
    lib, _native = native
    host = sm.grid_stride_pcm()
    n_pairs, fl = host.size // 2, sm.GRID_STRIDE_FRAME_LEN
    n_frames = -(-n_pairs // fl)
    assert n_frames == sm.GRID_STRIDE_FRAMES > sm.SWEEP_GRID_FRAMES
    pcm = _dev(torch, host)
    out = torch.full((2 * (n_frames + 16),), SENTINEL, dtype=torch.uint8, device="cuda")
    e = tables[1]["64"]
    _native.check(lib.ffs_vad_stereo_levels(pcm.data_ptr(), n_pairs, fl, e.data_ptr(), 64, out.data_ptr() + 8,
                                            out.data_ptr() + n_frames + 24, _native.current_stream_ptr(torch)))
    got = out.cpu().numpy()
    mid, side = sm.stereo_levels(host, fl, tables[0]["64"])
    assert np.array_equal(got[8:8 + n_frames], mid) and np.array_equal(got[n_frames + 24:2 * n_frames + 24], side)
    assert np.all(got[:8] == SENTINEL) and np.all(got[8 + n_frames:n_frames + 24] == SENTINEL) and np.all(got[2 * n_frames + 24:] == SENTINEL)
    assert len(np.unique(mid)) > 5 and len(np.unique(side)) > 5


def test_dual_mono_equals_the_mono_sweep_on_the_device(torch, native, tables):
    """L == R: mid is ffs_vad_levels of one channel byte for byte, side is all zero -- both paths, full-scale frames."""
    from ffsubsync_amd import adaptive_vad as av

    for fl in (5, 160, 480, 516):
        mono = ir.energy_pool(fl, 50.0).ravel()[:-3]
        dev = _dev(torch, mono)
        want = av.frame_levels(dev, fl)
        mid, side = av.stereo_levels(_dev(torch, sm.dual_mono(mono)), fl)
        assert torch.equal(mid, want) and not bool(side.any()) and int(want.max()) > 150, fl
    with pytest.raises(ValueError, match="not interleaved"):
        av.stereo_levels(dev[:7], 4)
    mid, side = av.stereo_levels(dev[:0], 4)
    assert mid.numel() == side.numel() == 0
    outs = (torch.full((20,), SENTINEL, dtype=torch.uint8, device="cuda"), torch.full((20,), SENTINEL, dtype=torch.uint8, device="cuda"))
    m2, s2 = av.stereo_levels(_dev(torch, sm.dual_mono(mono[:50])), 5, tables[1]["65"], out=(outs[0][3:], outs[1][1:]))
    assert np.array_equal(m2.cpu().numpy(), am.frame_levels(mono[:50], 5, tables[0]["65"])) and m2.numel() == 10 and not bool(s2.any())
    assert bool((outs[0][13:] == SENTINEL).all()) and bool((outs[0][:3] == SENTINEL).all()) and bool((outs[1][11:] == SENTINEL).all())
    with pytest.raises(ValueError, match="out: need 10 level bytes"):
        av.stereo_levels(_dev(torch, sm.dual_mono(mono[:50])), 5, out=(outs[0][:9], outs[1]))


# ---- the centre gate ---------------------------------------------------------------------------------------------------


class Batch:
    """Calls of ffs_vad_centre_gate side by side: mid and side at chosen byte offsets, outputs in slots with guards, the
    records 56 bytes apart; check() reads everything back once and compares with the model."""

    def __init__(self, torch, native):
        self.torch, (self.lib, self._native) = torch, native
        self.jobs = []

    def add(self, name, mid, side, t, c, mid_off=0, side_off=0, out=True, thr_dev=False):
        self.jobs.append(dict(name=name, mid=np.asarray(mid, np.uint8), side=np.asarray(side, np.uint8), t=t, c=c, mid_off=mid_off,
                              side_off=side_off, out=out, thr_dev=thr_dev))

    def run(self, stream=None, repeat_with=None):
        torch, _native = self.torch, self._native
        stream = _native.current_stream_ptr(torch) if stream is None else stream
        ipos = opos = 0
        for j in self.jobs:
            n = j["mid"].size
            ipos = (ipos + 15) // 16 * 16 + j["mid_off"]
            j["mat"] = ipos
            ipos = (ipos + n + 15) // 16 * 16 + j["side_off"]
            j["sat"] = ipos
            ipos += n
            j["oat"] = opos + 8
            opos += n + 8
        host = np.full(ipos + 16, 77, np.uint8)
        for j in self.jobs:
            host[j["mat"]:j["mat"] + j["mid"].size] = j["mid"]
            host[j["sat"]:j["sat"] + j["side"].size] = j["side"]
        self.host = host
        self.inputs = _dev(torch, host)
        self.out = torch.full((opos + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.records = torch.full((len(self.jobs) * 56 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.thr = [self._thresholds()]
        for k, j in enumerate(self.jobs):
            self._call(k, j, stream)
        if repeat_with is not None:   # the same record and output again, with other parameters: everything is overwritten
            for j in self.jobs:
                j.update(repeat_with(j))
            self.thr.append(self._thresholds())   # (the first table stays alive: its readers may still be queued)
            for k, j in enumerate(self.jobs):
                self._call(k, j, stream)
        return self

    def _thresholds(self):
        thr = np.zeros(len(self.jobs), self._native.VAD_THRESHOLD_DTYPE)
        thr["threshold_bin"] = [j["t"] for j in self.jobs]
        thr["flags"] = 77   # a reader that takes the wrong field sees it
        return _dev(self.torch, thr.view(np.uint8))

    def _call(self, k, j, stream):
        n = j["mid"].size
        base = self.inputs.data_ptr()
        self._native.check(self.lib.ffs_vad_centre_gate(
            base + j["mat"] if n else None, base + j["sat"] if n else None, n, self.thr[-1].data_ptr() + 48 * k if j["thr_dev"] else None,
            -5 if j["thr_dev"] else j["t"], j["c"], self.out.data_ptr() + j["oat"] if j["out"] else None,
            self.records.data_ptr() + 56 * k, stream))

    def check(self):
        _native = self._native
        o_host, r_host = self.out.cpu().numpy(), self.records.cpu().numpy()
        assert np.array_equal(self.inputs.cpu().numpy(), self.host)
        covered = np.zeros(o_host.size, bool)
        for k, j in enumerate(self.jobs):
            n = j["mid"].size
            want_out, want = sm.centre_gate(j["mid"], j["side"], j["t"], j["c"])
            what = (j["name"], n, j["t"], j["c"], j["mid_off"], j["side_off"], j["out"], j["thr_dev"])
            row = r_host[56 * k:56 * k + 48].view(_native.VAD_CENTRE_DTYPE)[0]
            assert tuple(int(row[f]) for f in sm.FIELDS) == sm.record_tuple(want), (what, row, want)
            assert np.all(r_host[56 * k + 48:56 * k + 56] == SENTINEL), what
            if j["out"]:
                assert np.array_equal(o_host[j["oat"]:j["oat"] + n], want_out), what
                covered[j["oat"]:j["oat"] + n] = True
        assert np.all(o_host[~covered] == SENTINEL)
        return self


def test_gate_sizes_alignments_thresholds_and_a_second_call(torch, native):
    """n = 0, 1, 63, 64, 65 and one more than a trip of the capped grid with mid and side 0, 1 and 3 bytes behind a 16-byte
    boundary, the threshold from the host and from a record on the device, out NULL for every fourth; then every call
    again over the same record and output with other parameters."""
    rng = np.random.RandomState(33)
    b = Batch(torch, native)
    k = 0
    for n in sm.GATE_LENGTHS:
        for mo in sm.GATE_OFFSETS:
            for so in sm.GATE_OFFSETS:
                if n > 65 and (mo + so) % 3:   # the long one at three of the nine offset pairs
                    continue
                mid, side = sm.random_levels(rng, n) if n else (np.zeros(0, np.uint8),) * 2
                b.add("size", mid, side, (100, 0, 1, 256, 130)[k % 5], (12, 0, 1, 255, 30)[k % 5 if k % 2 else (k // 5) % 5], mo, so,
                      out=bool(k % 4), thr_dev=bool(k % 2))
                k += 1
    assert sm.GATE_LENGTHS[-1] > native[1].VAD_CENTRE_GRID_FRAMES
    b.run(repeat_with=lambda j: dict(t=(j["t"] + 7) % 257, c=(j["c"] + 9) % 256, thr_dev=not j["thr_dev"])).check()


def test_gate_case_table(torch, native):
    """sm.gate_cases(): t = 0, 1 and 256, c = 0, 1 and 255, contrast exactly c and c - 1, side above mid, no active
    frame, every active frame rejected, dual mono, a negative sum of contrasts; host and device thresholds."""
    b = Batch(torch, native)
    for k, (name, mid, side, t, c) in enumerate(sm.gate_cases()):
        b.add(name, mid, side, t, c, sm.GATE_OFFSETS[k % 3], sm.GATE_OFFSETS[(k // 3) % 3], thr_dev=bool(k % 2))
    b.run().check()


def test_gate_from_a_pick_record_on_a_side_stream_behind_an_upload(torch, native):
    """Levels uploaded, histogram, pick and centre gate queued on a side stream with nothing between them: the threshold
    comes from the pick's record on the device; the wrapper with an int, a ThresholdRecord and the device record; then
    ffs_vad_level_labels and the steady-run gate on the output see what the model says they see."""
    from ffsubsync_amd import _native, adaptive_vad as av

    rng = np.random.RandomState(34)
    mid, side = sm.random_levels(rng, 5000)
    thr = am.pick(am.level_hist(mid, 192), rule=am.OTSU, lo_bin=0, t_min=1)
    t, c = thr["threshold_bin"], 10
    want_out, want = sm.centre_gate(mid, side, t, c)
    pm, ps = torch.from_numpy(mid).pin_memory(), torch.from_numpy(side).pin_memory()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dm, ds = pm.cuda(non_blocking=True), ps.cuda(non_blocking=True)
        raw = av.pick_threshold_device(av.level_hist(dm), lo_bin=0)
        outs = [av.centre_gate(dm, ds, raw, c), av.centre_gate(dm, ds, t, c), av.centre_gate(dm, ds, av.record_of(np.array(
            [tuple(thr[f] for f in am.FIELDS)], _native.VAD_THRESHOLD_DTYPE)[0]), c)]
        labels = av.level_labels(outs[0][0], raw, 0.0)
        gated, _ = av.steady_gate(outs[0][0], raw, 0, 40, 0.0)
        into = torch.full((5016,), SENTINEL, dtype=torch.uint8, device="cuda")
        o4, r4 = av.centre_gate(dm, ds, raw, c, out=into[5:])
    stream.synchronize()
    for k, (o, r) in enumerate(outs + [(o4, r4)]):
        rec = av.centre_record_of(r.cpu().numpy().view(_native.VAD_CENTRE_DTYPE)[0])
        assert [getattr(rec, f) for f in sm.FIELDS] == [want[f] for f in sm.FIELDS], k
        assert np.array_equal(o.cpu().numpy(), want_out), k
    assert bool((into[:5] == SENTINEL).all()) and bool((into[5005:] == SENTINEL).all())
    kept = (mid.astype(int) >= t) & (mid.astype(int) - side.astype(int) >= c)
    assert np.array_equal(labels.cpu().numpy() != 0, kept) and want["n_kept"] == int(kept.sum()) and 0 < kept.sum() < (mid >= t).sum()
    assert np.array_equal(gated.cpu().numpy() != 0, gm.gate_vectorised(want_out, t, 0, 40)[0])
    with pytest.raises(ValueError, match="must not overlap"):
        av.centre_gate(dm, ds, t, c, out=dm)
    with pytest.raises(ValueError, match="side: need 5000 level bytes"):
        av.centre_gate(dm, ds[:-1], t, c)


def test_refusals_of_both_exports(torch, native):
    sm.check_refusals(native[0])


# ---- whole-file entries --------------------------------------------------------------------------------------------------


def _shipped():
    from ffsubsync_amd import adaptive_vad as av

    return dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, fallback_bin=100,
                floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)


@pytest.fixture(scope="module")
def stereo():
    """sm.stereo_file() with the model's results at FILE_CONTRAST (plain and behind the steady-run gate) and at the
    shipped default, computed once and shared."""
    from ffsubsync_amd import adaptive_vad as av

    pcm = sm.stereo_file()
    at = {}
    for c in (sm.FILE_CONTRAST, av.DEFAULT_MIN_CONTRAST_BINS):
        at[c] = dict(plain=sm.detect(pcm, 160, c, **_shipped())[:4], steady=sm.detect(pcm, 160, c, steady=(0, 1000), **_shipped())[:4])
    speech = at[sm.FILE_CONTRAST]["plain"][0]
    (w0, w1), (b0, b1) = sm.WIDE, sm.BED_BURST
    assert not speech[w0:w1].any() and speech[b0:b1].all()   # the wide stretch is gone, the burst over the bed is kept
    return pcm, at


def _same(rec, want, fields):
    return [getattr(rec, f) for f in fields if f != "reserved"] == [want[f] for f in fields if f != "reserved"]


def _same_threshold(rec, want):
    return _same(rec, want, am.FIELDS[:-1]) and np.float64(rec.eta).view(np.uint64) == np.float64(want["eta"]).view(np.uint64)


def test_whole_file_entries_equal_the_model(torch, stereo):
    """detect_device_centre and detect_pinned_stream_centre, plain and steady, fp32 and packed: the model's labels and
    all records; the wide stretch is gone and the burst over the bed is kept."""
    from ffsubsync_amd import adaptive_vad as av

    pcm, at = stereo
    pinned = torch.from_numpy(pcm).pin_memory()
    dev = pinned.cuda()
    c = sm.FILE_CONTRAST
    for steady in (False, True):
        speech, thr, centre, gate = at[c]["steady" if steady else "plain"]
        for packed in (False, True):
            for res in (av.detect_device_centre(dev, 100, 16000, 0.1, packed=packed, min_contrast_bins=c, steady=steady),
                        av.detect_pinned_stream_centre(pinned, 100, 16000, 0.1, packed=packed, min_contrast_bins=c, steady=steady)):
                assert len(res) == (4 if steady else 3) and _same_threshold(res[1], thr) and _same(res[2], centre, sm.FIELDS), res[1:]
                assert not steady or _same(res[3], gate, gm.FIELDS)
                if packed:
                    words, bits = res[0].bits.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
                    assert res[0].packed and res[0].n == speech.size and np.array_equal(words[:bits.size], bits) and not words[bits.size:].any()
                else:
                    assert np.array_equal(res[0].cpu().numpy().view(np.uint32), ir.expected_f32(speech, 0.1).view(np.uint32))
    speech0, thr0, centre0, _ = at[av.DEFAULT_MIN_CONTRAST_BINS]["plain"]
    labels, rec, crec = av.detect_device_centre(dev, 100, 16000, 0.0)   # the shipped default
    assert _same_threshold(rec, thr0) and _same(crec, centre0, sm.FIELDS) and np.array_equal(labels.cpu().numpy() != 0, speech0)
    assert av.assess_centre(crec) == [] and len(av.assess_centre(av.centre_record_of(
        np.array([sm.record_tuple(at[c]["plain"][2])], av._native.VAD_CENTRE_DTYPE)[0]), 0.1)) == 1
    # a dual-mono file: the mono path's labels byte for byte, and the flag
    mono = np.ascontiguousarray(pcm[0::2])
    want = av.detect_device_adaptive(torch.from_numpy(mono).cuda(), 100, 16000, 0.1)
    got = av.detect_device_centre(torch.from_numpy(sm.dual_mono(mono)).cuda(), 100, 16000, 0.1)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2].flags == sm.MONO and "dual mono" in av.assess_centre(got[2])[0]


def test_speech_transformer_centre_and_centre_steady(torch, stereo):
    """PCMSpeechTransformer(vad="centre") and "centre_steady" from bytes and from a file object, at the shipped default
    and with the contrast in the name: float64 with exactly non_speech_label, all records kept; a trailing incomplete
    pair is dropped."""
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer
    from ffsubsync_amd import adaptive_vad as av

    pcm, at = stereo
    blob = pcm.tobytes()
    for vad, c, steady in (("centre", av.DEFAULT_MIN_CONTRAST_BINS, False), ("centre_steady", av.DEFAULT_MIN_CONTRAST_BINS, True),
                           ("centre:%d" % sm.FILE_CONTRAST, sm.FILE_CONTRAST, False), ("centre_steady:%d" % sm.FILE_CONTRAST, sm.FILE_CONTRAST, True)):
        speech, thr, centre, gate = at[c]["steady" if steady else "plain"]
        for label, source in ((0.1, blob + b"\x01\x02\x03"), (0.7, io.BytesIO(blob))):
            t = PCMSpeechTransformer(vad, 100, 16000, non_speech_label=label).fit(source)
            got = t.transform()
            assert got.dtype == np.float64 and np.array_equal(got, np.where(speech, 1.0, label)), (vad, label)
            assert _same_threshold(t.vad_threshold_, thr) and _same(t.vad_centre_, centre, sm.FIELDS), vad
            assert (t.vad_gate_ is None) == (not steady) and (not steady or _same(t.vad_gate_, gate, gm.FIELDS)), vad
    (w0, w1), (b0, b1) = sm.WIDE, sm.BED_BURST
    assert (got[w0:w1] == 0.7).all() and (got[b0:b1] == 1.0).all()
    mono = PCMSpeechTransformer("adaptive", 100, 16000).fit(np.ascontiguousarray(pcm[0::2]).tobytes())
    assert mono.vad_centre_ is None and (mono.transform()[w0:w1] == 1.0).all()
    with pytest.raises(ValueError, match="Unable to detect speech"):
        PCMSpeechTransformer("centre", 100, 16000).fit(b"")


def test_streams_longer_than_one_buffer(torch):
    """25 003 frames of 4 pairs: the pinned entry sweeps two whole 10 000-frame buffers and a part of a third, the
    transformer reads as many chunks from bytes and from a file object; the model's labels and records, both gates."""
    from ffsubsync_amd import adaptive_vad as av
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer, WINDOWS_PER_BUFFER, frames_per_window

    pcm = sm.stream_pcm()
    rate, frame_rate = sm.STREAM_RATES
    assert frames_per_window(rate, frame_rate) == sm.STREAM_FRAME_LEN and sm.STREAM_FRAMES > 2 * WINDOWS_PER_BUFFER
    c = 6
    speech, thr, centre, gate, mid, side = sm.detect(pcm, sm.STREAM_FRAME_LEN, c, steady=(0, 100), **_shipped())
    plain = sm.detect(pcm, sm.STREAM_FRAME_LEN, c, **_shipped())[0]
    default_run, _, _, default_gate, _, _ = sm.detect(pcm, sm.STREAM_FRAME_LEN, c, steady=(0, av.default_max_run(rate)), **_shipped())
    assert speech.size == sm.STREAM_FRAMES and 0 < speech.sum() < plain.sum() < (mid >= thr["threshold_bin"]).sum() and gate["n_rejected"] > 0
    pinned = torch.from_numpy(pcm).pin_memory()
    labels, rec, crec, grec = av.detect_pinned_stream_centre(pinned, rate, frame_rate, 0.0, min_contrast_bins=c, steady=True, max_run=100)
    assert _same_threshold(rec, thr) and _same(crec, centre, sm.FIELDS) and _same(grec, gate, gm.FIELDS)
    assert np.array_equal(labels.cpu().numpy() != 0, speech)
    labels, rec, crec = av.detect_pinned_stream_centre(pinned, rate, frame_rate, 0.0, min_contrast_bins=c)
    assert _same(crec, centre, sm.FIELDS) and np.array_equal(labels.cpu().numpy() != 0, plain)
    for vad, want in (("centre_steady:%d" % c, default_run), ("centre:%d" % c, plain)):
        for source in (pcm.tobytes(), io.BytesIO(pcm.tobytes())):
            t = PCMSpeechTransformer(vad, rate, frame_rate).fit(source)
            assert np.array_equal(t.transform() != 0, want) and _same(t.vad_centre_, centre, sm.FIELDS) and _same_threshold(t.vad_threshold_, thr), vad
    steady_t = PCMSpeechTransformer("centre_steady:%d" % c, rate, frame_rate).fit(pcm.tobytes())
    assert _same(steady_t.vad_gate_, default_gate, gm.FIELDS)


def test_centre_raster_feeds_quality_sync_without_a_host_look(torch, stereo):
    """The packed raster of the file goes straight into quality_sync; the answer is the one the model's labels give."""
    from ffsubsync_amd import adaptive_vad as av, quality

    pcm, at = stereo
    speech = at[sm.FILE_CONTRAST]["steady"][0]
    edges = np.flatnonzero(np.diff(speech.astype(np.int8), prepend=0, append=0))
    a, b = edges[0::2], edges[1::2]
    keep = a >= 150
    track = ((a[keep] - 150) * 10000).astype(np.int64), ((b[keep] - 150) * 10000).astype(np.int64), np.zeros(int(keep.sum()), np.uint8)
    raster = av.detect_device_centre(torch.from_numpy(pcm).cuda(), 100, 16000, 0.0, packed=True, min_contrast_bins=sm.FILE_CONTRAST,
                                     steady=True)[0]
    got = quality.quality_sync([(raster, track)], 4)[0]
    want = quality.quality_sync([(speech.astype(float), track)], 4)[0]
    assert (got.ratio_index, got.ratio, got.offset) == (want.ratio_index, want.ratio, want.offset) and abs(got.offset) == 150
    assert np.float64(got.score).view(np.uint64) == np.float64(want.score).view(np.uint64)
    assert got.quality == want.quality and got.reasons == want.reasons
