"""CPU checks of tests/ingest_reference.py: the references against oracle/vad_oracle.py, and the conditions that
tests/test_gpu_ingest.py relies on, asserted on that module's own inputs (both import their builders from
ingest_reference) so that they cannot rot: no frame is ambiguous, every branch of k_vad_energy and both tokenizer
kernels are visited, the derived tokenizer bound holds for the models.  Parity with auditok stays unpinned."""
import math
from collections import Counter

import numpy as np
import pytest

import ingest_reference as ir
from oracle import vad_oracle as vo


def _oracle(pcm, frame_len, thr, fast=True):
    f = vo.detect_fast if fast else vo.detect
    return f(pcm, 1, frame_len, non_speech_label=0.0, threshold_db=thr) == 1.0   # frame_len(1, fl) == fl


def test_frame_sums_and_boundary_frames_are_exact():
    """boundary_frame hits 10^k n + delta exactly, and on those frames the oracle's 10*log10(sum/n) >= thr rule and
    the integer rule agree (k = 0..9, delta = -1, 0, 1, frame lengths 1 .. 4800)."""
    built = 0
    for fl in ir.FRAME_LENS:
        assert vo.frame_len(1, fl) == fl
        for k in range(10):
            for delta in (-1, 0, 1):
                frame = ir.boundary_frame(fl, k, delta)
                if frame is None:
                    continue
                built += 1
                sums, counts = ir.frame_sums(frame, fl)
                assert sums.tolist() == [10 ** k * fl + delta] and counts.tolist() == [fl]
                speech, dist = ir.energy_labels(frame, fl, 10.0 * k)
                assert speech.tolist() == [delta >= 0] and dist == math.inf
                assert _oracle(frame, fl, 10.0 * k, fast=False).tolist() == [delta >= 0]
                assert _oracle(frame, fl, 10.0 * k).tolist() == [delta >= 0]
    assert built >= 350
    assert ir.boundary_frame(1, 0, 1) is None and ir.boundary_frame(1, 9, 0) is None   # 2 and 10^9 are not squares
    assert ir.boundary_frame(480, 5, 0).dtype == np.int16
    # a short tail frame is a frame of its own length
    sums, counts = ir.frame_sums(np.array([3, -4, 5], np.int16), 2)
    assert sums.tolist() == [25, 25] and counts.tolist() == [2, 1]


def test_vector_path_restates_the_dispatch_rule():
    assert ir.vector_path(480, 0, 0, 4 * 480) == ir.VECTOR
    assert ir.vector_path(480, 16, 0, 4 * 480) == ir.VECTOR
    assert ir.vector_path(480, 0, 0, 4 * 480 - 1) == ir.ELEMENT_TAIL
    assert ir.vector_path(480, 0, 4, 7 * 480) == ir.ELEMENT_TAIL
    assert ir.vector_path(480, 2, 0, 4 * 480) == ir.ELEMENT_UNALIGNED
    assert ir.vector_path(512, 0, 0, 4 * 512) == ir.VECTOR
    assert ir.vector_path(441, 0, 0, 4 * 441) == ir.ELEMENT_ODD
    assert ir.vector_path(520, 0, 0, 4 * 520) == ir.ELEMENT_ROUNDS
    assert ir.vector_path(4800, 0, 0, 4 * 4800) == ir.ELEMENT_ROUNDS


def test_energy_cases_are_unambiguous_cover_every_branch_and_match_the_oracle():
    """On every input of the GPU sweep: energy_labels == vo.detect == vo.detect_fast; no frame within 1e-9 of a
    non-decade threshold (so fp64 rounding cannot move a label: the share of ambiguous frames is zero); every branch
    class of k_vad_energy holds at least 16 speech and 16 non-speech frames; every threshold meets every offset, and
    every (threshold, label) pair occurs; boundary and full-scale frames are served by the vector and the element path."""
    per_class = {c: Counter() for c in ir.BRANCH_CLASSES}
    pairs, thr_off, n_cases = set(), set(), 0
    for fl in ir.FRAME_LENS:
        frame_counts = set()
        for case in ir.energy_cases(fl):
            n_cases += 1
            pcm, thr, n = ir.case_pcm(case), case["threshold"], case["n_samples"]
            assert pcm.size == n and pcm.dtype == np.int16
            speech, dist = ir.energy_labels(pcm, fl, thr)
            if ir.decade(thr) is None:
                assert dist > 1e-9, (fl, thr, dist)
            else:
                assert dist == math.inf
            assert np.array_equal(speech, _oracle(pcm, fl, thr)), (fl, thr, case["offset"], n)
            if n_cases % 7 == 0:
                assert np.array_equal(speech, _oracle(pcm, fl, thr, fast=False)), (fl, thr, case["offset"], n)
            # what lies behind the slice is loud: a kernel that reads past n_samples changes the last label
            behind = case["buffer"][case["offset"] + n:]
            assert behind.size >= ir.GUARD_SAMPLES and np.abs(behind[-ir.GUARD_SAMPLES:].astype(int)).min() >= 32767
            n_frames = speech.size
            frame_counts.add(n_frames % 8)
            for f in range(n_frames):
                cls = ir.vector_path(fl, 2 * case["offset"], f - f % 4, n)
                per_class[cls][bool(speech[f])] += 1
            pairs.add((thr, case["label"]))
            thr_off.add((thr, case["offset"]))
        assert frame_counts == set(range(8)), fl
    assert n_cases >= 17 * 4 * 8 * 2
    for cls, count in per_class.items():
        assert count[True] >= 16 and count[False] >= 16, (cls, count)
    assert pairs == {(t, l) for t in ir.THRESHOLDS for l in ir.ENERGY_LABELS}
    assert thr_off == {(t, o) for t in ir.THRESHOLDS for o in ir.START_OFFSETS}


def test_energy_pools_hold_the_boundary_and_full_scale_frames():
    for fl in ir.FRAME_LENS:
        for thr in ir.DECADE_THRESHOLDS:
            pool = ir.energy_pool(fl, thr)
            sums, _ = ir.frame_sums(pool.ravel(), fl)
            k = ir.decade(thr)
            for delta in (-1, 0, 1):
                if ir.boundary_frame(fl, k, delta) is not None:
                    assert np.count_nonzero(sums == 10 ** k * fl + delta) >= 2, (fl, thr, delta)
            assert np.count_nonzero(sums == fl * 2 ** 30) >= 2                       # all -32768
            assert np.count_nonzero(sums == fl * 32767 ** 2) >= (2 if fl > 1 else 1)  # all 32767
    # 4800 samples of -32768: 5.2e12, far beyond 32 bits -- the 64-bit accumulation across the element loop's rounds
    assert 4800 * 2 ** 30 > 5e12


def test_large_inputs_match_the_oracle():
    pcm = ir.grid_stride_pcm()
    assert pcm.dtype == np.int16 and pcm.size < 5_000_000 and pcm.size % ir.GRID_STRIDE_FRAME_LEN
    speech, _ = ir.energy_labels(pcm, ir.GRID_STRIDE_FRAME_LEN, 50.0)
    assert speech.size == ir.GRID_STRIDE_FRAMES > 524288 and 0.2 < speech.mean() < 0.6
    assert np.array_equal(speech, _oracle(pcm, ir.GRID_STRIDE_FRAME_LEN, 50.0))
    for rate in ir.STREAM_RATES:
        n, fl = ir.stream_samples(rate), vo.frame_len(100, rate)
        assert n // (fl * 10000) == ir.STREAM_BUFFERS and 0 < n % (fl * 10000) and (n % (fl * 10000)) % fl
    src = ir.stream_source()[: ir.stream_samples(16000)]
    want = vo.chunked_detect(src, 100, 16000, non_speech_label=0.1)
    speech, _ = ir.energy_labels(src, 160, 50.0)
    assert np.array_equal(want == 1.0, speech) and set(np.unique(want)) == {0.1, 1.0}


def test_token_markers_reproduce_the_restatement_and_the_bound_holds():
    """token_markers + the float64 marker arithmetic is vo.tokenize_chunk for dyadic labels, bit for bit; for labels
    float32 cannot hold, both float32 models (end marker formed in float32, or in float64 from the float32 label) stay
    within (cm + 1) * 2^-23 of the float64 restatement."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for trial in range(40):
        n = int(rng.choice([1, 7, 64, 500, 3000]))
        valid = ir.validity_pattern(rng, n)
        cp, cm = ir.token_markers(valid, 20.0, 500, 25.0)
        for label in ir.DYADIC_LABELS:
            want = vo.tokenize_chunk(valid, label)
            assert np.array_equal(np.clip(cp + cm * (label - 1.0), 0.0, 1.0), want)
            assert np.array_equal(ir.token_model(cp, cm, label).astype(float), want)
            assert np.array_equal(ir.token_model_f32_marker(cp, cm, label).astype(float), want)
            assert np.array_equal(ir.rasterise_tokens(n, ir.chunk_tokens(valid, (20.0, 500, 25.0)), label), want)
        for label in ir.NON_DYADIC_LABELS + (0.1 + 2.0 ** -30,):
            want = vo.tokenize_chunk(valid, label)
            for model in (ir.token_model, ir.token_model_f32_marker):
                err = np.abs(model(cp, cm, label).astype(np.float64) - want)
                assert np.all(err <= ir.token_bound(cm)), (trial, label, model.__name__)
                worst = max(worst, float(np.max(err / ir.token_bound(cm))))
    assert 0.0 < worst < 0.5


def test_token_inputs_visit_both_kernels_with_every_parameter_case():
    served = Counter()
    cases = set()
    for valid, case in ir.token_inputs():
        cases.add(case)
        for chunk in ir.TOKEN_CHUNKS:
            served[ir.serial_kernel_serves(valid.size, chunk, case)] += 1
            want, cp, cm = ir.tokenize_f64(valid, (0.0, 0.1), chunk, case)
            assert want[0.0].size == cp.size == cm.size == valid.size
            assert np.array_equal(np.clip(cp - cm.astype(float), 0.0, 1.0), want[0.0])
    assert cases == set(ir.TOKEN_CASES) and served[True] >= 3 and served[False] >= 20
    assert any(cm.max() >= 2 for cm in [ir.tokenize_f64(v, (0.0,), 10000, c)[2] for v, c in ir.token_inputs()])


def test_auditok30_case_turns_on_the_ceiling_of_the_silence_limit():
    """sample_rate 30: the tokenizer's limits are (6.0, 150, 7.5); a silence counter reaches 7.5 at 8 frames, so the
    integer limit that means the same is ceil(7.5) = 8, and the input tells 8 from 7."""
    pcm, valid = ir.auditok30_pcm()
    assert vo.frame_len(*ir.AUDITOK30) == 1600 and pcm.size % 1600
    speech, _ = ir.energy_labels(pcm, 1600, 50.0)
    assert np.array_equal(speech, valid) and np.array_equal(speech, _oracle(pcm, 1600, 50.0))
    as_floats = vo._Tokenizer(0.2 * 30, int(5 * 30), 0.25 * 30).tokenize(speech)
    assert (0.2 * 30, 0.25 * 30) == (6.0, 7.5)
    assert as_floats == vo._Tokenizer(6, 150, 8).tokenize(speech)
    assert as_floats != vo._Tokenizer(6, 150, 7).tokenize(speech)


def test_host_loops():
    x = np.array([0.5, np.nextafter(0.5, 1.0), np.nan, 0.75, 0.5])
    assert ir.fit_boundaries(x) == (1, 3) and ir.fit_boundaries(x.astype(np.float32)) == (3, 3)
    assert ir.fit_boundaries(np.zeros(4)) == (None, None)
    f = np.array([0.1, np.nextafter(np.float32(0.1), np.float32(0)), np.nan, np.inf], np.float32)
    assert ir.pack_bits(f, 0.1).tolist() == [0b1001, 0, 0, 0]   # float32(0.1) is larger than 0.1
    assert ir.pack_bits(f, float(np.float32(0.1))).tolist() == [0b1000, 0, 0, 0]
    assert ir.pack_bits(np.array([0, 2, 0, 255] * 9, np.uint8)).tolist() == [0xAA, 0xAA, 0xAA, 0xAA, 0x0A, 0, 0, 0]
    got = ir.scatter([np.ones(5), np.full(4, 2.0), np.full(3, 3.0)], [2, 5, 9], 10)
    assert got.tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 2, 3]
    for n in (1, 257, 131073):
        for name, vec in ir.bounds_patterns(n):
            assert vec.dtype == np.float32 and vec.size == n, name
    names = [name for name, _ in ir.bounds_patterns(2 ** 20 + 5)]
    assert "second_trip" in names and len(names) == len(set(names)) == 12


@pytest.mark.parametrize("frame_len", [1, 8, 441, 4800])
def test_tails(frame_len):
    t = ir.tails(frame_len)
    assert 0 in t and all(0 <= x < frame_len for x in t)
    assert (1 in t) == (frame_len > 1) and (frame_len - 1 in t)
