"""The centre-channel VAD's model on the CPU (tests/stereo_vad_model.py): the identities of the contract
(L == R is the mono sweep, swapping the channels changes nothing, negating one swaps mid and side), the conditions on
the inputs tests/test_gpu_stereo_vad.py runs (no frame within rounding of an edge, the boundary and full-scale frames are
what they name), the record arithmetic and what follows from the rule, every host-side refusal of the exports and of the
Python layer with its message, and the shipped default against profiles/centre_gate_calibration.json by the script's
rule.  The rule has no upstream counterpart: the model is the only reference."""
import json
import os
import sys

import numpy as np
import pytest

import adaptive_vad_model as am
import steady_gate_model as gm
import stereo_vad_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _interleave(left, right):
    return np.stack([np.asarray(left, np.int16), np.asarray(right, np.int16)], axis=1).ravel()


def test_dual_mono_is_the_mono_sweep_byte_for_byte():
    """L == R: mid equals adaptive_vad_model.frame_levels of one channel for every table, side is all zero -- the gain
    files, and every pool of the mono sweep's frame lengths with their full-scale and boundary frames."""
    import ingest_reference as ir

    fl, files = am.gain_files()
    inputs = [(fl, pcm) for pcm in files.values()] + [(n, ir.energy_pool(n, 50.0).ravel()[:-3]) for n in (1, 7, 160, 480, 516)]
    for frame_len, mono in inputs:
        for name, edges in am.edge_tables().items():
            mid, side = sm.stereo_levels(sm.dual_mono(mono), frame_len, edges)
            assert np.array_equal(mid, am.frame_levels(mono, frame_len, edges)) and not side.any(), (frame_len, name)


def test_swapping_channels_changes_nothing_and_negating_one_swaps_mid_and_side():
    for frame_len in sm.FRAME_LENS:
        pool = sm.sweep_pool(frame_len)
        pcm = pool.ravel()[:-2 * (frame_len // 2)] if frame_len > 1 else pool.ravel()
        left, right = pcm[0::2], pcm[1::2]
        m, s, n = sm.stereo_sums(pcm, frame_len)
        m2, s2, n2 = sm.stereo_sums(_interleave(right, left), frame_len)
        assert np.array_equal(m, m2) and np.array_equal(s, s2) and np.array_equal(n, n2)
        ok = right != -32768   # -(-32768) is not an int16: those pairs are zeroed in both versions
        l0, r0 = np.where(ok, left, 0), np.where(ok, right, 0)
        a = sm.stereo_levels(_interleave(l0, r0), frame_len, am.default_edges())
        b = sm.stereo_levels(_interleave(l0, -r0), frame_len, am.default_edges())
        assert np.array_equal(a[0], b[1]) and np.array_equal(a[1], b[0]) and a[0].any() and a[1].any()


def test_sums_are_exact_at_full_scale():
    """All samples -32768: (L + R)^2 = 2^32 and 2 L R = 2^31 per pair; the mixed-sign pairs: (L - R)^2 = 65535^2."""
    for frame_len in (1, 5, 516):
        a, b, c = sm.extreme_frames(frame_len)
        m, s, n = sm.stereo_sums(np.concatenate([a, b, c]).astype(np.int16).ravel(), frame_len)
        assert [int(x) for x in m] == [frame_len << 32, frame_len, frame_len] and [int(x) for x in s] == [0, frame_len * 65535 ** 2] * 1 + [frame_len * 65535 ** 2]
        assert list(n) == [frame_len] * 3
    assert sm.stereo_sums(np.zeros(0, np.int16), 7)[2].size == 0


def test_no_frame_of_any_builder_lies_within_rounding_of_an_edge():
    """As adaptive_vad_model.edge_distance for the mono cases: the smallest relative distance of any M or S from any
    inexact edge is far above 2^-52, so fp64 rounding cannot move a level, on any slice the GPU test takes (a slice's
    short last frame included)."""
    tables = am.edge_tables()
    for frame_len in sm.FRAME_LENS:
        bufs = sm.sweep_buffers(frame_len)
        worst = np.inf
        for case in sm.sweep_cases(frame_len):
            worst = min(worst, sm.edge_distance(sm.case_pcm(bufs, case), frame_len, tables[case["table"]]))
        assert worst > 1e-12, (frame_len, worst)
    assert sm.edge_distance(sm.grid_stride_pcm(), sm.GRID_STRIDE_FRAME_LEN, tables["64"]) > 1e-12
    assert sm.edge_distance(sm.stereo_file(), 160, tables["default"]) > 1e-12
    assert sm.edge_distance(sm.stream_pcm(), sm.STREAM_FRAME_LEN, tables["default"]) > 1e-12


def test_the_sweep_cases_reach_what_they_name():
    """Every table holds the decades of DECADES exactly (or, "one", 10^5); a pool's boundary frames sit exactly at, one
    below and one above 10^k * 4 n in M and in S separately and take the levels that says; every (offset, count residue,
    tail kind, table) and every pair of output offsets occurs; the grid-stride case takes a second trip."""
    tables = am.edge_tables()
    for name, e in tables.items():
        assert name == "one" or all(float(10 ** k) in e for k in sm.DECADES)
    assert float(10 ** 5) in tables["one"] and 5 in sm.DECADES
    for frame_len in sm.FRAME_LENS:
        for which in ("mid", "side"):
            have = 0
            for k in sm.DECADES:
                lv = {}
                for d in (-1, 0, 1):
                    f = sm.boundary_frame(frame_len, k, d, which)
                    if f is None:   # no such frame: too few pairs for the sum (always at one pair: 4 * 10^k +- 1 is no square)
                        assert frame_len <= 5
                        continue
                    m, s, _ = sm.stereo_sums(f.ravel(), frame_len)
                    assert int((m if which == "mid" else s)[0]) == 10 ** k * 4 * frame_len + d and int((s if which == "mid" else m)[0]) <= frame_len
                    lv[d] = int(sm.stereo_levels(f.ravel(), frame_len, tables["default"])[which == "side"][0])
                    have += 1
                assert all(v == (20 * k - 1 if d < 0 else 20 * k) for d, v in lv.items())   # edges[20 k - 1] = 10^k is the (20 k)-th edge
            assert have >= {1: 1, 3: 4, 4: 8}.get(frame_len, 9), (frame_len, which, have)
    for frame_len in sm.FRAME_LENS:
        cases = list(sm.sweep_cases(frame_len))
        assert {c["offset"] for c in cases} == set(sm.START_OFFSETS)
        assert {(c["mid_off"], c["side_off"]) for c in cases} == {(a, b) for a in sm.OUT_OFFSETS for b in sm.OUT_OFFSETS}
        for t in sm.TABLES:
            mine = [c for c in cases if c["table"] == t]
            assert {c["offset"] for c in mine} == set(sm.START_OFFSETS)
            residues = {(c["n_pairs"] // frame_len) % 8 for c in mine if c["n_pairs"] >= 40 * frame_len}
            assert residues == set(range(8)) or (frame_len == 1 and len(residues) >= 4), (frame_len, t)   # one pair: a third of the cases
            assert {c["n_pairs"] % frame_len for c in mine} == set(sm.tails(frame_len))
        assert any(c["n_pairs"] == 0 for c in cases) and any(c["n_pairs"] == frame_len for c in cases)
    assert {480, 512, 516} <= set(sm.FRAME_LENS) and sm.MAX_FRAME_VEC == 512 and sm.ONE_VECTOR_MORE == 516
    assert sm.GRID_STRIDE_FRAMES > sm.SWEEP_GRID_FRAMES and sm.grid_stride_pcm().size == 2 * (4 * sm.GRID_STRIDE_FRAMES - 1)


def test_record_arithmetic():
    out, rec = sm.centre_gate([120, 120, 119, 131, 12, 11], [108, 109, 107, 120, 0, 0], 100, 12)
    assert list(out) == [120, 0, 119, 0, 12, 0]
    assert sm.record_tuple(rec) == (100, 0, 12, 120, 6, 4, 2, 12 + 11 + 12 + 11)
    out, rec = sm.centre_gate([100, 101, 150, 99], [255, 250, 140, 0], 100, 5)
    assert list(out) == [0, 0, 150, 99] and sm.record_tuple(rec) == (100, 0, 5, 255, 4, 3, 1, -155 - 149 + 10)
    assert sm.record_tuple(sm.centre_gate([120, 10], [0, 0], 100, 12)[1]) == (100, sm.MONO, 12, 0, 2, 1, 1, 120)
    assert sm.record_tuple(sm.centre_gate([120, 130], [115, 130], 100, 12)[1]) == (100, sm.ALL_REJECTED, 12, 130, 2, 2, 0, 5)
    assert sm.record_tuple(sm.centre_gate([], [], 100, 12)[1]) == (100, 0, 12, 0, 0, 0, 0, 0)
    assert sm.record_tuple(sm.centre_gate([5], [0], 256, 255)[1]) == (256, sm.MONO, 255, 0, 1, 0, 0, 0)
    named = {name: sm.centre_gate(m, s, t, c)[1] for name, m, s, t, c in sm.gate_cases()}
    assert named["no active frame"]["n_active"] == 0 and not named["no active frame"]["flags"]
    assert named["all active frames rejected"]["flags"] == sm.ALL_REJECTED and named["dual mono"]["flags"] == sm.MONO
    assert named["negative sum of contrasts"]["sum_contrast"] < 0 and named["t 256: nothing active"]["n_active"] == 0
    assert named["t 0: everything active"]["n_active"] == 700 and named["side above mid"]["n_kept"] == 0


def test_what_follows_from_the_rule():
    """ffs_vad_level_labels(out, t) labels exactly the kept frames (t >= 1); the steady-run gate sees a rejected frame as
    level 0; for L == R and c <= t the labels are the mono path's."""
    rng = np.random.RandomState(31)
    for k in range(20):
        mid, side = sm.random_levels(rng, 900)
        t, c = int(rng.randint(1, 200)), int(rng.randint(0, 60))
        out, rec = sm.centre_gate(mid, side, t, c)
        kept = (mid.astype(int) >= t) & (mid.astype(int) - side.astype(int) >= c)
        assert np.array_equal(am.speech(out, t), kept) and rec["n_kept"] == int(kept.sum())
        assert np.array_equal(out, np.where(mid.astype(int) - side.astype(int) >= c, mid, 0))
        zeroed = np.where(kept | (mid.astype(int) < t), out, 0)   # what the steady gate is given is what it would be given with zeros
        assert np.array_equal(gm.gate_vectorised(out, t, 0, 50)[0], gm.gate_vectorised(zeroed, t, 0, 50)[0])
    fl, files = am.gain_files()
    for g, mono in files.items():
        speech, thr, _ = am.detect(mono, fl, lo_bin=0, t_min=1)
        for c in (0, 1, thr["threshold_bin"]):
            got, thr2, centre, _, mid, side = sm.detect(sm.dual_mono(mono), fl, c, lo_bin=0, t_min=1)
            assert thr2 == thr and np.array_equal(got, speech) and centre["flags"] == sm.MONO and centre["n_kept"] == centre["n_active"], (g, c)


def test_whole_file_input_is_what_the_gpu_test_needs():
    """tests/test_gpu_stereo_vad.py's file: the plain labels hold the whole wide stretch, the centre gate at FILE_CONTRAST
    drops all of it and keeps the burst over the bed; with the steady-run gate behind it the labels stay."""
    from ffsubsync_amd import adaptive_vad as av

    pick = dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, fallback_bin=100,
                floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)
    pcm = sm.stereo_file()
    speech, thr, centre, _, mid, side = sm.detect(pcm, 160, sm.FILE_CONTRAST, **pick)
    plain = am.speech(mid, thr["threshold_bin"])
    (w0, w1), (b0, b1) = sm.WIDE, sm.BED_BURST
    assert not thr["flags"] and not centre["flags"] and plain[w0:w1].all() and not speech[w0:w1].any()
    assert plain[b0:b1].all() and speech[b0:b1].all() and side[b0:b1].min() > side[:50].max()
    assert centre["n_active"] - centre["n_kept"] >= w1 - w0 and 0 < speech.sum() < plain.sum()
    steady, _, _, gate, _, _ = sm.detect(pcm, 160, sm.FILE_CONTRAST, steady=(0, 1000), **pick)
    assert np.array_equal(steady, speech) and gate["n_rejected"] == 0 and gate["n_stretches"] > 5
    # at the shipped default (a frame is rejected only when side exceeds mid) part of the wide stretch stays
    shipped = sm.detect(pcm, 160, av.DEFAULT_MIN_CONTRAST_BINS, **pick)[0]
    assert av.DEFAULT_MIN_CONTRAST_BINS < sm.FILE_CONTRAST and 0 < shipped[w0:w1].sum() < w1 - w0 and shipped[b0:b1].all()


def test_refusals_of_the_exports_need_no_device():
    from ffsubsync_amd import _native

    assert _native.VAD_CENTRE_DTYPE.names == sm.FIELDS and _native.VAD_CENTRE_BYTES == 48
    assert (_native.VAD_CENTRE_MONO, _native.VAD_CENTRE_ALL_REJECTED) == (sm.MONO, sm.ALL_REJECTED)
    assert _native.VAD_STEREO_MAX_FRAME_VEC == sm.MAX_FRAME_VEC and _native.VAD_CENTRE_GRID_FRAMES == sm.GATE_GRID_FRAMES
    sm.check_refusals(_native.load())
    for name in ("ffs_vad_stereo_levels", "ffs_vad_centre_gate"):
        assert name in _native.EXPORTED_SYMBOLS and not name.endswith("_batch")


def test_python_checks_come_before_any_native_call():
    """Every host-side refusal of the Python layer with its message: CPU tensors stand in, nothing reaches the library."""
    import torch

    from ffsubsync_amd import adaptive_vad as av

    tensors = dict(pcm=torch.zeros(640, dtype=torch.int16), mid=torch.zeros(4, dtype=torch.uint8), side=torch.zeros(4, dtype=torch.uint8))
    for call, fragment in sm.python_refusals(av, tensors):
        with pytest.raises(ValueError) as err:
            call()
        assert fragment in str(err.value), (fragment, str(err.value))
    rec = av.CentreRecord(100, 0, 12, 90, 1000, 400, 300, 9000)
    assert av.assess_centre(rec) == [] and len(av.assess_centre(rec, 0.2)) == 1 and av.assess_centre(rec, 0.25) == []
    assert "dual mono" in av.assess_centre(av.CentreRecord(100, sm.MONO, 12, 0, 10, 4, 4, 400))[0]
    assert "all 7 active frames" in av.assess_centre(av.CentreRecord(100, sm.ALL_REJECTED, 12, 130, 10, 7, 0, 3))[0]
    row = np.zeros(1, __import__("ffsubsync_amd")._native.VAD_CENTRE_DTYPE)[0]
    row["sum_contrast"], row["max_side"] = -5, 7
    got = av.centre_record_of(row)
    assert (got.sum_contrast, got.max_side, got.n_frames) == (-5, 7, 0)


def test_transformer_names_do_not_collide():
    """Neither new vad name holds a substring an earlier branch tests for."""
    for name in ("centre", "centre_steady"):
        assert not any(s in name for s in ("gated", "adaptive", "energy", "fused", "webrtc", "auditok", "silero"))


def test_default_is_what_the_calibration_derives():
    """profiles/centre_gate_calibration.json: every figure recomputed with the model from the counts it keeps,
    the recommendation re-derived by the script's rule, and the shipped default equal to it."""
    from ffsubsync_amd import adaptive_vad as av

    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    try:
        import centre_gate_calibrate as cal
    finally:
        sys.path.pop(0)
    doc = json.load(open(os.path.join(ROOT, "profiles", "centre_gate_calibration.json")))
    assert doc["candidates"] == list(cal.CANDIDATES) == [0, 6, 12, 18, 24] and doc["keeps"] == cal.KEEPS == 0.99
    assert doc["rhos"] == [0.0, 0.5, 0.9, 1.0] and doc["beds_db"] == [-20, -10] and doc["gains_db"] == [0, -10, -20, -30, -40]
    assert {f["cell"] for f in doc["files"]} == {cal.cell_name(c) for c in cal.CELLS}
    files = cal.with_figures(doc["files"])   # the JSON keeps the counts; every figure is computed again by the model
    assert cal.recommend(files) == doc["shipped"]["min_contrast_bins"] == av.DEFAULT_MIN_CONTRAST_BINS
    assert cal.by_cell(files) == doc["by_cell"]
    assert all(sum(n for _, _, _, n in f["hist"]) == doc["duration"] * 100 for f in files)
    assert any(f["finds_speech"] for f in doc["files"])
