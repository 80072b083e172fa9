"""The steady-run gate (ffs_vad_steady_gate, adaptive_vad.steady_gate) against tests/steady_gate_model.py,
bit for bit: labels, packed bits, every field of the record and every guard byte around the caller's outputs.  Many
cases share one output buffer with sentinels between them and are read back once.  The rule has no upstream
counterpart: the model is the reference (tests/test_steady_gate_host.py pins its three forms against each other)."""
import io

import numpy as np
import pytest

import adaptive_vad_model as am
import ingest_reference as ir
import steady_gate_model as gm

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
F_GUARD = -7.0
T = gm.TILE


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


class Batch:
    """Calls of ffs_vad_steady_gate side by side: levels at a chosen byte offset behind an 8-byte boundary, outputs in
    slots with guards, one workspace per call; check() reads everything back once and compares with the model."""

    def __init__(self, torch, native):
        self.torch, (self.lib, self._native) = torch, native
        self.jobs = []

    def add(self, name, levels, t, dip, max_run, label=0.0, form="both", offset=0, thr_dev=False):
        self.jobs.append(dict(name=name, levels=np.asarray(levels, np.uint8), t=t, dip=dip, max_run=max_run, label=label, form=form,
                              offset=offset, thr_dev=thr_dev))

    def run(self, stream=None, repeat_with=None):
        torch, lib, _native = self.torch, self.lib, self._native
        stream = _native.current_stream_ptr(torch) if stream is None else stream
        lpos = fpos = bpos = 0
        for j in self.jobs:
            n = j["levels"].size
            lpos = (lpos + 15) // 16 * 16 + j["offset"]
            j.update(lat=lpos, fat=fpos, bat=bpos)
            lpos += n + 8
            fpos += n + 4
            bpos += (n + 7) // 8 + 8
        host = np.full(lpos + 16, 77, np.uint8)
        for j in self.jobs:
            host[j["lat"]:j["lat"] + j["levels"].size] = j["levels"]
        self.levels = _dev(torch, host)
        assert self.levels.data_ptr() % 16 == 0
        self.f_out = torch.full((fpos + 4,), F_GUARD, dtype=torch.float32, device="cuda")
        self.b_out = torch.full((bpos + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.records = torch.full((len(self.jobs) * 56 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        thr = np.zeros(len(self.jobs), _native.VAD_THRESHOLD_DTYPE)
        thr["threshold_bin"] = [j["t"] for j in self.jobs]
        thr["flags"] = 77   # a reader that takes the wrong field sees it
        self.thr = _dev(torch, thr.view(np.uint8))
        self.ws = []
        for k, j in enumerate(self.jobs):
            self._call(k, j, stream)
        if repeat_with is not None:   # the same outputs again, with other parameters: everything is overwritten
            for k, j in enumerate(self.jobs):
                j.update(repeat_with(j))
                self._call(k, j, stream)
        return self

    def _call(self, k, j, stream):
        torch, lib, _native = self.torch, self.lib, self._native
        n = j["levels"].size
        need = int(lib.ffs_vad_steady_gate_workspace_bytes(n))
        assert need == gm.workspace_bytes(n)
        ws = torch.full((need + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ws.append((ws, need))
        _native.check(lib.ffs_vad_steady_gate(
            self.levels.data_ptr() + j["lat"] if n else None, n, self.thr.data_ptr() + 48 * k if j["thr_dev"] else None,
            -5 if j["thr_dev"] else j["t"], j["dip"], j["max_run"], j["label"],
            self.f_out.data_ptr() + 4 * j["fat"] if j["form"] in ("both", "labels") else None,
            self.b_out.data_ptr() + j["bat"] if j["form"] in ("both", "bits") else None,
            self.records.data_ptr() + 56 * k, ws.data_ptr(), need, stream))

    def check(self):
        _native = self._native
        f_host, b_host, r_host = self.f_out.cpu().numpy(), self.b_out.cpu().numpy(), self.records.cpu().numpy()
        assert np.all(self.levels.cpu().numpy()[-8:] == 77)
        f_cov, b_cov = np.zeros(f_host.size, bool), np.zeros(b_host.size, bool)
        for k, j in enumerate(self.jobs):
            n = j["levels"].size
            speech, want = gm.gate_vectorised(j["levels"], j["t"], j["dip"], j["max_run"])
            what = (j["name"], n, j["t"], j["dip"], j["max_run"], j["form"], j["offset"])
            row = r_host[56 * k:56 * k + 48].view(_native.VAD_GATE_DTYPE)[0]
            assert tuple(int(row[f]) for f in gm.FIELDS) == gm.record_tuple(want), (what, row, want)
            assert np.all(r_host[56 * k + 48:56 * k + 56] == SENTINEL), what
            if j["form"] in ("both", "labels"):
                got = f_host[j["fat"]:j["fat"] + n]
                assert np.array_equal(got.view(np.uint32), ir.expected_f32(speech, j["label"]).view(np.uint32)), what
                f_cov[j["fat"]:j["fat"] + n] = True
            if j["form"] in ("both", "bits"):
                nb = (n + 7) // 8
                assert np.array_equal(b_host[j["bat"]:j["bat"] + nb], ir.expected_bits(speech)), what
                b_cov[j["bat"]:j["bat"] + nb] = True
        assert np.all(f_host[~f_cov] == F_GUARD) and np.all(b_host[~b_cov] == SENTINEL)
        for ws, need in self.ws:   # nothing behind the workspace the export asked for
            assert np.all(ws[need:].cpu().numpy() == SENTINEL)
        return self


def test_lengths_alignments_and_output_forms(torch, native):
    """n = 0, 1, 7, 8, 9, 15, 16, 17, GATE_TILE - 1, GATE_TILE, GATE_TILE + 1 with the levels 0, 1 and 3 bytes behind a
    16-byte boundary (the 16-byte loads and the byte loop), both outputs, each alone and neither, the threshold from the
    host and from a record on the device, labels float32 cannot hold; then the same outputs again with other parameters."""
    rng = np.random.RandomState(3)
    b = Batch(torch, native)
    k = 0
    for n in gm.LENGTHS:
        for off in gm.OFFSETS:
            lv = gm.random_levels(rng, n, 0.2) if n else np.zeros(0, np.uint8)
            b.add("length", lv, 100, (0, 10)[k % 2], (3, 9, 40)[k % 3], (0.1, 0.0, -1.0, 0.7)[k % 4],
                  ("both", "labels", "bits", "none")[(k + k // 4) % 4], off, thr_dev=bool(k % 2))
            k += 1
    b.run(repeat_with=lambda j: dict(dip=10 - j["dip"], max_run=j["max_run"] + 2, label=0.3, thr_dev=not j["thr_dev"])).check()


def test_stretches_against_tile_edges_limits_thresholds_and_dips(torch, native):
    """gm.stretch_cases(): a rise on a tile's last frame with the fall on the next one's first, a stretch through three
    tiles without a setter, files that start active, end inside a stretch, hold only keep or only active frames,
    trailing keep frames on both sides of a tile edge, stretches of exactly max_run and one more, max_run = 1, dips of 0,
    t - 1, t and 255, t = 0 and 256, random files; each at a levels offset of 0, 1 or 3."""
    b = Batch(torch, native)
    for k, (name, lv, t, dip, max_run) in enumerate(gm.stretch_cases()):
        b.add(name, lv, t, dip, max_run, (0.0, 0.25)[k % 2], "both", gm.OFFSETS[k % 3], thr_dev=bool(k % 2))
    b.run().check()


def test_carry_scan_over_more_than_a_wave_and_more_than_a_trip_of_tiles(torch, native):
    """65 and 257 tiles plus 17 frames with one stretch carried through all but five tiles, at a limit that rejects it
    and at exactly its length; the packed form only (the labels of a million frames add nothing)."""
    b = Batch(torch, native)
    for tiles, lv, t, dip, max_run in gm.scan_cases():
        b.add("scan %d" % tiles, lv, t, dip, max_run, 0.0, "bits", 0, thr_dev=tiles == 65)
    b.run().check()
    assert [j["levels"].size for j in b.jobs] == [65 * T + 17] * 2 + [257 * T + 17] * 2


def test_side_stream_behind_an_upload(torch, native):
    """The levels are uploaded and the gate queued on a side stream with nothing between them; the wrapper, with an int,
    a ThresholdRecord and the device record as the threshold."""
    from ffsubsync_amd import _native, adaptive_vad as av

    name, lv, t, dip, max_run = gm.stretch_cases()[-1]
    speech, want = gm.gate_vectorised(lv, t, dip, max_run)
    pinned = torch.from_numpy(lv).pin_memory()
    rec = np.zeros(1, _native.VAD_THRESHOLD_DTYPE)
    rec["threshold_bin"] = t
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = pinned.cuda(non_blocking=True)
        thr = torch.from_numpy(rec.view(np.uint8)).pin_memory().cuda(non_blocking=True)
        outs = [av.steady_gate(dev, t, dip, max_run, 0.5), av.steady_gate(dev, av.record_of(rec[0]), dip, max_run, 0.5),
                av.steady_gate(dev, thr, dip, max_run, 0.5), av.steady_gate(dev, thr, dip, max_run, 0.5, packed=True)]
        taken = [(a.bits.clone() if hasattr(a, "bits") else a.clone(), r.clone()) for a, r in outs]
    side.synchronize()
    for k, (labels, raw) in enumerate(taken):
        got = av.gate_record_of(raw.cpu().numpy().view(_native.VAD_GATE_DTYPE)[0])
        assert [getattr(got, f) for f in gm.FIELDS if f != "reserved"] == [want[f] for f in gm.FIELDS if f != "reserved"], k
        if k < 3:
            assert np.array_equal(labels.cpu().numpy().view(np.uint32), ir.expected_f32(speech, 0.5).view(np.uint32)), k
        else:
            words, bits = labels.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
            assert np.array_equal(words[:bits.size], bits) and not words[bits.size:].any()
    raster = outs[3][0]
    assert raster.packed and raster.n == lv.size and (raster.lo, raster.hi) == (0.5, 1.0)
    # max_run >= n: byte for byte the plain labels
    plain = av.level_labels(dev, t, 0.5)
    assert torch.equal(av.steady_gate(dev, t, 0, lv.size, 0.5)[0], plain) and torch.equal(av.steady_gate(dev, t, 90, lv.size, 0.5)[0], plain)


def test_too_long_path_is_the_plain_labels(torch, native):
    """2^23 + 1 frames of zeros with four active ones: the gate is skipped (max_run = 2 would drop them), the outputs are
    ffs_vad_level_labels' byte for byte, the record holds n_frames and the flag, and no workspace is asked for."""
    lib, _native = native
    n = gm.MAX_FRAMES + 1
    assert lib.ffs_vad_steady_gate_workspace_bytes(n) == 0
    dev = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dev[T - 2:T + 2] = 200
    nb = (n + 7) // 8
    bits = torch.full((nb + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    plain = torch.full((nb + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    record = torch.full((56,), SENTINEL, dtype=torch.uint8, device="cuda")
    stream = _native.current_stream_ptr(torch)
    _native.check(lib.ffs_vad_steady_gate(dev.data_ptr(), n, None, 100, 0, 2, 0.0, None, bits.data_ptr(), record.data_ptr(), None, 0, stream))
    _native.check(lib.ffs_vad_level_labels(dev.data_ptr(), n, None, 100, 0.0, None, plain.data_ptr(), stream))
    assert torch.equal(bits, plain) and int(bits[:nb].to(torch.int32).sum()) == 0xC0 + 0x03
    raw = record.cpu().numpy()
    want = gm.record(100, 0, n, too_long=True)
    assert tuple(int(raw[:48].view(_native.VAD_GATE_DTYPE)[0][f]) for f in gm.FIELDS) == gm.record_tuple(want)
    assert np.all(raw[48:] == SENTINEL)


def test_refusals_of_both_exports(torch, native):
    gm.check_refusals(native[0])


# ---- whole-file entries ----------------------------------------------------------------------------------------------


def _shipped():
    from ffsubsync_amd import adaptive_vad as av

    return dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, fallback_bin=100,
                floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)


@pytest.fixture(scope="module")
def tone():
    """gm.tone_file() with the model's pick, plain labels, gated labels and gate record (computed once, shared)."""
    pcm, (m0, m1) = gm.tone_file()
    plain, thr, levels = am.detect(pcm, 160, **_shipped())
    speech, gate = gm.gate_vectorised(levels, thr["threshold_bin"], 0, 1000)
    assert not thr["flags"] and plain[m0:m1].all() and not speech[m0 - 30:m1].any()   # the tone, and the burst that abuts it
    assert gate["n_rejected"] == 1 and gate["longest_run"] == m1 - m0 + 30 and 0 < speech.sum() == plain.sum() - (m1 - m0 + 30)
    return pcm, speech, thr, gate


def _same_gate(rec, want):
    return [getattr(rec, f) for f in gm.FIELDS if f != "reserved"] == [want[f] for f in gm.FIELDS if f != "reserved"]


def _same_threshold(rec, want):
    return [getattr(rec, f) for f in am.FIELDS[:-1]] == [want[f] for f in am.FIELDS[:-1]] and \
        np.float64(rec.eta).view(np.uint64) == np.float64(want["eta"]).view(np.uint64)


def test_whole_file_entries_equal_the_model(torch, tone):
    """detect_device_gated and detect_pinned_stream_gated on a file of speech bursts with pauses and one 14 s tone: the
    model's labels, fp32 and packed, and both records; a caller's max_run and dip_bins reach the gate."""
    from ffsubsync_amd import adaptive_vad as av

    pcm, speech, thr, gate = tone
    pinned = torch.from_numpy(pcm).pin_memory()
    dev = pinned.cuda()
    for labels, rec, grec in (av.detect_device_gated(dev, 100, 16000, 0.1), av.detect_pinned_stream_gated(pinned, 100, 16000, 0.1)):
        assert _same_threshold(rec, thr) and _same_gate(grec, gate), (rec, grec)
        assert labels.is_cuda and np.array_equal(labels.cpu().numpy().view(np.uint32), ir.expected_f32(speech, 0.1).view(np.uint32))
    for raster, rec, grec in (av.detect_device_gated(dev, 100, 16000, 0.1, packed=True),
                              av.detect_pinned_stream_gated(pinned, 100, 16000, 0.1, packed=True)):
        assert _same_threshold(rec, thr) and _same_gate(grec, gate) and raster.packed and raster.n == speech.size
        words, bits = raster.bits.view(torch.uint8).cpu().numpy(), ir.expected_bits(speech)
        assert np.array_equal(words[:bits.size], bits) and not words[bits.size:].any()
    assert av.assess_gate(grec) == [] and len(av.assess_gate(grec, 0.1)) == 1
    levels = am.frame_levels(pcm, 160, am.default_edges())
    want, wrec = gm.gate_vectorised(levels, thr["threshold_bin"], 5, 120)
    labels, _, grec = av.detect_device_gated(dev, 100, 16000, 0.0, dip_bins=5, max_run=120)
    assert _same_gate(grec, wrec) and np.array_equal(labels.cpu().numpy() != 0, want) and wrec["n_rejected"] > 1


def test_speech_transformer_gated(torch, tone):
    """PCMSpeechTransformer(vad="gated") from bytes and from a file object: float64 with exactly non_speech_label, both
    records kept; "adaptive" still labels the tone."""
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer

    pcm, speech, thr, gate = tone
    for label, source in ((0.1, pcm.tobytes()), (0.7, io.BytesIO(pcm.tobytes()))):
        t = PCMSpeechTransformer("gated", 100, 16000, non_speech_label=label).fit(source)
        got = t.transform()
        assert got.dtype == np.float64 and np.array_equal(got, np.where(speech, 1.0, label)), label
        assert set(np.unique(got)) == {label, 1.0} and _same_threshold(t.vad_threshold_, thr) and _same_gate(t.vad_gate_, gate)
    plain = PCMSpeechTransformer("adaptive", 100, 16000).fit(pcm.tobytes())
    assert plain.vad_gate_ is None and (plain.transform()[1500:2900] == 1.0).all() and (got[1500:2900] == 0.7).all()
    with pytest.raises(ValueError, match="Unable to detect speech"):
        PCMSpeechTransformer("gated", 100, 16000).fit(b"")


def test_gated_raster_feeds_quality_sync_without_a_host_look(torch, tone):
    """The packed gated raster of the file goes straight into quality_sync; the answer is the one the model's labels give."""
    from ffsubsync_amd import adaptive_vad as av, quality

    pcm, speech, thr, gate = tone
    edges = np.flatnonzero(np.diff(speech.astype(np.int8), prepend=0, append=0))
    a, b = edges[0::2], edges[1::2]
    keep = a >= 150
    track = ((a[keep] - 150) * 10000).astype(np.int64), ((b[keep] - 150) * 10000).astype(np.int64), np.zeros(int(keep.sum()), np.uint8)
    raster, _, _ = av.detect_device_gated(torch.from_numpy(pcm).cuda(), 100, 16000, 0.0, packed=True)
    got = quality.quality_sync([(raster, track)], 4)[0]
    want = quality.quality_sync([(speech.astype(float), track)], 4)[0]
    assert (got.ratio_index, got.ratio, got.offset) == (want.ratio_index, want.ratio, want.offset) and abs(got.offset) == 150
    assert np.float64(got.score).view(np.uint64) == np.float64(want.score).view(np.uint64)
    assert got.quality == want.quality and got.reasons == want.reasons
