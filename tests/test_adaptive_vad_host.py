"""Host side of the adaptive energy VAD (ffsubsync_amd.adaptive_vad): the exports and the record against the
header, every ValueError before any native call, the library's own refusals, the wording of assess, the conditions on the
inputs of tests/test_gpu_adaptive_vad.py (no frame within rounding of an edge, no histogram decided by rounding), the
point of the feature on the model, and the shipped defaults recomputed from the committed calibration.  No device."""
import json
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import adaptive_vad_model as am
import ingest_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ffsubsync_amd.h")
CALIBRATION = os.path.join(ROOT, "profiles", "adaptive_vad_calibration.json")
EXPORTS = ("ffs_vad_levels", "ffs_vad_level_hist", "ffs_vad_pick_threshold", "ffs_vad_level_labels")


def test_exports_and_record_against_the_header():
    from ffsubsync_amd import _native, adaptive_vad

    text = open(HEADER).read()
    lib = _native.load()
    args = lambda name: [" ".join(a.split()[:-1]).replace("const ", "")
                         for a in re.search(r"int %s\(([^;]*)\);" % name, text).group(1).split(",")]
    for name in EXPORTS:
        assert name in _native.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert args(name)[-1] == "void*" and "plan" not in " ".join(args(name))  # stateless, a stream last
    assert args("ffs_vad_levels") == ["int16_t*", "int64_t", "int", "double*", "int", "uint8_t*", "void*"]
    assert args("ffs_vad_level_hist") == ["uint8_t*", "int64_t", "int", "uint32_t*", "void*"]
    assert args("ffs_vad_pick_threshold") == ["uint32_t*"] + ["int"] * 9 + ["ffs_vad_threshold*", "void*"]
    assert args("ffs_vad_level_labels") == ["uint8_t*", "int64_t", "int32_t*", "int", "float", "float*", "uint8_t*", "void*"]
    for name in EXPORTS:
        assert len(getattr(lib, name).argtypes) == len(args(name))
    body = re.search(r"typedef struct ffs_vad_threshold \{(.*?)\} ffs_vad_threshold;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(double|int32_t|int64_t)\s+([^;]+);", body):
        fields += [(n.strip(), {"double": "<f8", "int32_t": "<i4", "int64_t": "<i8"}[ctype]) for n in names.split(",")]
    dt = _native.VAD_THRESHOLD_DTYPE
    assert [(n, dt.fields[n][0].str) for n in dt.names] == fields and list(dt.names) == list(am.FIELDS)
    assert dt.names[0] == "threshold_bin" and dt.fields["threshold_bin"][1] == 0  # ffs_vad_level_labels reads it in place
    assert all(dt.fields[n][1] % dt.fields[n][0].itemsize == 0 for n in dt.names)
    size = int(re.search(r"sizeof\(ffs_vad_threshold\) == (\d+)", text).group(1))
    assert size == dt.itemsize == _native.VAD_THRESHOLD_BYTES == 48
    csrc = open(os.path.join(ROOT, "ffsubsync_amd", "csrc", "ffs_adaptive_vad.h")).read()
    assert "static_assert(sizeof(VadThreshold) == %d" % size in csrc
    for name in ("FALLBACK", "TOO_LONG", "EMPTY", "FLAT", "CLAMPED_LO", "CLAMPED_HI"):
        value = int(re.search(r"#define FFS_VAD_THR_%s (\d+)" % name, text).group(1))
        assert value == getattr(_native, "VAD_THR_" + name) == getattr(am, name)
    for name, model in (("OTSU", am.OTSU), ("FLOOR", am.FLOOR)):
        assert int(re.search(r"#define FFS_VAD_RULE_%s (\d+)" % name, text).group(1)) == getattr(_native, "VAD_RULE_" + name) == model
    assert _native.VAD_RULES == am.RULES
    for name, value in (("MAX_EDGES", 255), ("MAX_BINS", 256), ("MAX_FRAMES", 1 << 23)):
        assert int(re.search(r"#define FFS_VAD_%s (\d+)" % name, text).group(1)) == value == getattr(_native, "VAD_" + name) == getattr(am, name)
    assert adaptive_vad.MAX_FRAMES == 1 << 23 and adaptive_vad.DEFAULT_FALLBACK_BIN == 100
    # the launch geometry the model file states next to its histogram counts
    for name, value in (("HIST_MAX_BLOCKS", am.HIST_MAX_BLOCKS), ("HIST_THREADS", am.HIST_BYTES_PER_TRIP // 16)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), csrc)
    assert am.HIST_IDLE == 4097 and am.HIST_TWO_TRIPS > 2 * am.HIST_MAX_BLOCKS * am.HIST_BYTES_PER_TRIP


def test_the_library_refuses_bad_arguments_without_a_device():
    from ffsubsync_amd import _native

    am.check_refusals(_native.load())
    assert {name for name, _ in am.refusal_calls()} == set(EXPORTS)


def test_default_edges_hold_the_exact_decades():
    from ffsubsync_amd import adaptive_vad

    e = adaptive_vad.default_edges()
    assert e.dtype == np.float64 and e.size == 191 and np.array_equal(e, am.default_edges()) and np.all(np.diff(e) > 0)
    for j in range(9):
        assert e[19 + 20 * j] == float(10 ** (j + 1)), j
    assert e[99] == 1e5 and e[59] == 1e3
    assert adaptive_vad.threshold_db(adaptive_vad.ThresholdRecord(100, 0, 0, 0, 0, 0, 0, 0.0)) == 50.0
    assert adaptive_vad.threshold_db(adaptive_vad.ThresholdRecord(0, 0, 0, 0, 0, 0, 0, 0.0)) == -np.inf
    assert adaptive_vad.threshold_db(adaptive_vad.ThresholdRecord(192, 0, 0, 0, 0, 0, 0, 0.0)) == np.inf
    assert adaptive_vad.threshold_db(adaptive_vad.ThresholdRecord(1, 0, 0, 0, 0, 0, 0, 0.0), [1e3, 1e4]) == 30.0
    # for an ascending table level >= t is the fixed rule with threshold edges[t - 1]
    pcm = ir.energy_pool(160, 50.0).ravel()
    speech, _ = ir.energy_labels(pcm, 160, 50.0)
    assert np.array_equal(am.frame_levels(pcm, 160, e) >= 100, speech) and 0 < speech.sum() < speech.size
    for name, table in am.edge_tables().items():
        assert 1 <= table.size <= 255 and np.all(np.diff(table) > 0) and np.all(table > 0), name
    assert [t.size for t in am.edge_tables().values()] == [191, 1, 255, 64, 65]


@pytest.mark.parametrize("frame_len", ir.FRAME_LENS)
def test_no_frame_of_the_gpu_cases_is_within_rounding_of_an_edge(frame_len):
    """On every PCM case of the level sweep and under every edge table, no frame lies within 1e-12 relative of an edge
    that is not an exact decade (where the comparison is exact in integers): rounding cannot move a level.  And the
    cases do visit frames exactly at, one below and one above a decade edge."""
    every = np.unique(np.concatenate(list(am.edge_tables().values())))
    worst, seen = np.inf, set()
    at_edge = {-1: 0, 0: 0, 1: 0}
    for c in ir.energy_cases(frame_len):
        key = (id(c["buffer"]), c["offset"], c["n_samples"])
        if key in seen:
            continue
        seen.add(key)
        pcm = ir.case_pcm(c)
        worst = min(worst, am.edge_distance(pcm, frame_len, every))
        sums, counts = ir.frame_sums(pcm, frame_len)
        for k in range(10):
            for d in at_edge:
                at_edge[d] += int(np.sum(sums - 10 ** k * counts == d))
    assert worst > 1e-12, worst
    # (a frame of a few samples cannot be one above or below every decade: a sum of so few squares does not reach it)
    assert at_edge[0] and (frame_len < 16 or all(at_edge.values())), at_edge


def test_no_other_gpu_input_is_within_rounding_of_an_edge():
    e = am.default_edges()
    assert am.edge_distance(ir.grid_stride_pcm(), ir.GRID_STRIDE_FRAME_LEN, e) > 1e-12
    src = ir.stream_source()
    for rate in ir.STREAM_RATES:
        from oracle import vad_oracle as vo

        assert am.edge_distance(src[:ir.stream_samples(rate)], vo.frame_len(100, rate), e) > 1e-12, rate
    fl, files = am.gain_files()
    for pcm in files.values():
        assert am.edge_distance(pcm, fl, e) > 1e-12


def test_the_pick_table_is_never_decided_by_rounding():
    """For every histogram of the pick table the model's fp64 choice equals the maximiser in exact rational arithmetic,
    and no other candidate comes within 2^-50 of the maximum: a case where rounding decides is not in the table.  The
    same on random and adversarial histograms, to show such tables are the rule and not the exception."""
    names = set()
    for name, h, kw in am.pick_cases():
        names.add(name)
        lo = kw.get("lo_bin", 20)
        t, close = am.otsu_exact(h, lo)
        assert not close, name
        args = dict(kw, rule=am.OTSU, t_min=lo + 1, t_max=h.size - 1)
        rec = am.pick(h, **args)
        if sum(int(x) for x in h) > am.MAX_FRAMES:
            assert rec["flags"] == am.TOO_LONG | am.FALLBACK, name
        elif t is None:
            assert rec["flags"] & am.FALLBACK, name
        else:
            assert rec["threshold_bin"] == t and not rec["flags"], (name, rec, t)
            d, m = next((d, m) for tt, d, m in am.otsu_scores(h, lo) if tt == t)
            hh = [int(x) if b >= lo else 0 for b, x in enumerate(h)]
            N, S, Q = sum(hh), sum(b * x for b, x in enumerate(hh)), sum(b * b * x for b, x in enumerate(hh))
            exact = Fraction(d * d, m) / (N * Q - S * S)
            assert abs(Fraction(rec["eta"]) - exact) <= exact * Fraction(1, 1 << 50) and 0 < rec["eta"] <= 1.0, name
    assert len(names) == len(am.pick_cases())   # names are unique
    flags = [am.pick(h, **kw)["flags"] for _, h, kw in am.pick_cases()]
    for bit in (am.FALLBACK, am.TOO_LONG, am.EMPTY, am.FLAT, am.CLAMPED_LO, am.CLAMPED_HI):
        assert any(f & bit for f in flags), bit
    assert {h.size for _, h, _ in am.pick_cases()} >= {2, 256, 192}
    totals = {int(h.astype(np.int64).sum()) for _, h, _ in am.pick_cases()}
    assert {1 << 23, (1 << 23) + 1} <= totals
    rng = np.random.RandomState(3)
    for i in range(300):
        B = int(rng.choice([4, 17, 64, 192, 256]))
        if i % 3 == 0:   # adversarial: near-symmetric spikes
            h = np.zeros(B, np.int64)
            a = int(rng.randint(1, 1 << 20))
            h[[0, B - 1]] = [a, a + int(rng.randint(0, 3))]
            h[rng.randint(0, B)] += int(rng.randint(0, 3))
        else:
            h = rng.randint(0, int(rng.choice([3, 1000, 30000])), size=B).astype(np.int64)
        t, _ = am.otsu_exact(h, 0)
        rec = am.pick(h, lo_bin=0, t_min=1, fallback_bin=0)
        assert (rec["threshold_bin"] == t) if t is not None else bool(rec["flags"] & am.FALLBACK), (i, h)


def test_the_floor_rule_counts_exactly():
    cases = {name: (h, kw) for name, h, kw in am.pick_cases()}
    h, kw = cases["floor exactly at need"]
    assert am.pick(h, **kw)["floor_bin"] == 31 and am.pick(h, **kw)["threshold_bin"] == 31 + 12
    h, kw = cases["floor one short of need"]
    assert am.pick(h, **kw)["floor_bin"] == 60
    h, kw = cases["plateau"]
    assert am.pick(h, **kw)["threshold_bin"] == 1   # the lowest t of the plateau 1, 2, 3


def test_adaptive_labels_do_not_depend_on_the_gain():
    """Speech 30 dB above the floor at gains 0, -12 and -30 dB by integer-exact scaling: the adaptive labels are
    identical, the thresholds move with the gain, and the fixed 50 dB rule finds nothing at -30 dB."""
    from ffsubsync_amd import adaptive_vad as av

    fl, files = am.gain_files()
    args = dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1, floor_ppm=av.DEFAULT_FLOOR_PPM,
                margin_bins=av.DEFAULT_MARGIN_BINS)
    out = {g: am.detect(pcm, fl, **args) for g, pcm in files.items()}
    speech = out[0][0]
    assert 0.2 < speech.mean() < 0.6
    for g in (-12, -30):
        assert np.array_equal(out[g][0], speech) and not out[g][1]["flags"], g
    assert out[0][1]["threshold_bin"] > out[-12][1]["threshold_bin"] > out[-30][1]["threshold_bin"]
    fixed = {g: ir.energy_labels(pcm, fl, 50.0)[0] for g, pcm in files.items()}
    assert np.array_equal(fixed[0], speech) and not fixed[-30].any()
    for rule in (am.OTSU, am.FLOOR):   # either rule, and with the silence bin at 10 dB
        got = [am.detect(pcm, fl, rule=rule, lo_bin=0, t_min=1, floor_ppm=200000, margin_bins=10)[0] for pcm in files.values()]
        assert all(np.array_equal(g, speech) for g in got), rule


def test_every_bad_argument_raises_before_any_native_call():
    import torch

    from ffsubsync_amd import adaptive_vad as av

    cpu_pcm, cpu_levels = torch.zeros(320, dtype=torch.int16), torch.zeros(10, dtype=torch.uint8)
    hist = torch.zeros(192, dtype=torch.int32)
    with pytest.raises(ValueError, match="unknown rule 'mean'"):
        av.pick_threshold(hist, "mean")
    with pytest.raises(ValueError, match="unknown rule 3"):
        av.rule_code(3)
    for kw, match in ((dict(lo_bin=-1), "lo_bin=-1"), (dict(lo_bin=30, t_min=30), "t_min=30"), (dict(t_max=192), "t_max=192"),
                      (dict(t_min=50, t_max=49), "t_min=50"), (dict(fallback_bin=193), "fallback_bin=193"),
                      (dict(fallback_bin=-1), "fallback_bin=-1"), (dict(floor_ppm=-1), "floor_ppm=-1"),
                      (dict(floor_ppm=1000001), "floor_ppm=1000001"), (dict(margin_bins=-1), "margin_bins=-1"),
                      (dict(margin_bins=256), "margin_bins=256"), (dict(lo_bin=1.5), "lo_bin=1.5"),
                      (dict(margin_bins=2.0), "margin_bins=2.0"), (dict(t_max=True), "t_max=True")):
        with pytest.raises(ValueError, match=match):
            av.pick_threshold(hist, "otsu", **kw)
        with pytest.raises(ValueError, match=match):
            av.detect_device_adaptive(cpu_pcm, 100, 16000, 0.0, **kw)
        with pytest.raises(ValueError, match=match):
            av.detect_pinned_stream_adaptive(cpu_pcm, 100, 16000, 0.0, **kw)
    for bad in (torch.zeros(192, dtype=torch.int64), torch.zeros(2, 2, 192, dtype=torch.int32), np.zeros(192, np.int32)):
        with pytest.raises(ValueError, match="hist: need a contiguous int32 CUDA tensor"):
            av.pick_threshold(bad)
    with pytest.raises(ValueError, match="hist: need a contiguous int32 CUDA tensor"):
        av.pick_threshold(hist)   # right shape, not on a device
    with pytest.raises(ValueError, match="n_bins=1"):
        av.pick_threshold(torch.zeros(1, dtype=torch.int32))
    for edges, match in (([], "edges: need 1 to 255"), (np.ones(256), "edges: need 1 to 255"), (np.ones((2, 2)), "edges: need 1 to 255"),
                         ([1.0, 1.0], "strictly ascending"), ([2.0, 1.0], "strictly ascending"), ([0.0, 1.0], "positive finite"),
                         ([1.0, np.inf], "positive finite"), ([np.nan], "positive finite"), (["a"], "edges: need 1 to 255"),
                         (torch.ones(3), "a device table must be")):
        with pytest.raises(ValueError, match=match):
            av.frame_levels(cpu_pcm, 160, edges)
        with pytest.raises(ValueError, match=match):
            av.detect_device_adaptive(cpu_pcm, 100, 16000, 0.0, edges=edges)
    for fl in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="frame_len="):
            av.frame_levels(cpu_pcm, fl)
    for pcm in (cpu_pcm, np.zeros(10, np.int16), None):
        with pytest.raises(ValueError, match="pcm: need a contiguous int16 CUDA vector"):
            av.frame_levels(pcm, 160)
        with pytest.raises(ValueError, match="pcm: need a contiguous int16 CUDA vector"):
            av.detect_device_adaptive(pcm, 100, 16000, 0.0)
    for pcm in (np.zeros(10, np.int16), torch.zeros(10, dtype=torch.float32), torch.zeros(2, 5, dtype=torch.int16), None):
        with pytest.raises(ValueError, match="pcm: need a contiguous int16 CPU vector"):
            av.detect_pinned_stream_adaptive(pcm, 100, 16000, 0.0)
    for label in (float("nan"), float("inf"), None, "0", True):
        with pytest.raises(ValueError, match="non_speech_label="):
            av.detect_device_adaptive(cpu_pcm, 100, 16000, label)
        with pytest.raises(ValueError, match="non_speech_label="):
            av.level_labels(cpu_levels, 100, label)
    with pytest.raises(ValueError, match="sample_rate=100, frame_rate=10"):
        av.detect_device_adaptive(cpu_pcm, 100, 10, 0.0)
    with pytest.raises(ValueError, match="unknown parameter bogus"):
        av.detect_device_adaptive(cpu_pcm, 100, 16000, 0.0, bogus=1)
    with pytest.raises(ValueError, match="unknown rule 'mean'"):
        av.detect_pinned_stream_adaptive(cpu_pcm, 100, 16000, 0.0, rule="mean")
    for thr in (-1, 257, 1.5, None, True, "100"):
        with pytest.raises(ValueError, match="threshold="):
            av.level_labels(cpu_levels, thr)
    with pytest.raises(ValueError, match="a device threshold must be"):
        av.level_labels(cpu_levels, torch.zeros(1, dtype=torch.int32))
    for levels in (cpu_levels, np.zeros(4, np.uint8), None):
        with pytest.raises(ValueError, match="levels: need a contiguous uint8 CUDA vector"):
            av.level_labels(levels, 100)
        with pytest.raises(ValueError, match="levels: need a contiguous uint8 CUDA vector"):
            av.level_hist(levels)
    for n_bins in (1, 257, 2.5, True):
        with pytest.raises(ValueError, match="n_bins="):
            av.level_hist(cpu_levels, n_bins)
    with pytest.raises(ValueError, match="min_eta=2"):
        av.assess(av.ThresholdRecord(40, 0, 30, 90, 10, 10, 5, 0.9), 2)


def test_the_new_vad_name_changes_no_existing_one():
    from ffsubsync_amd.speech_transformers import PCMSpeechTransformer

    assert not any(s in "adaptive" for s in ("energy", "auditok", "webrtc", "fused", "silero"))
    t = PCMSpeechTransformer("adaptive")
    assert t.vad_threshold_ is None
    with pytest.raises(ValueError, match="unknown vad: adaptive"):
        t._make_detector()   # not behind the per-chunk factory seam: a threshold per chunk would be inconsistent


def test_assess_wording():
    from ffsubsync_amd import adaptive_vad as av

    R = av.ThresholdRecord
    assert av.assess(R(42, 0, 40, 96, 10700, 10700, 2800, 0.99)) == []
    assert av.assess(R(100, am.TOO_LONG | am.FALLBACK, 20, 255, (1 << 23) + 1, (1 << 23) + 1, 5, 0.0)) == [
        "too many frames for one histogram (8388609 > 8388608): fixed rule used"]
    assert av.assess(R(100, am.EMPTY | am.FALLBACK, -1, -1, 1004, 0, 0, 0.0)) == [
        "no frame at or above the silence bin (1004 frames): fixed rule used"]
    assert av.assess(R(100, am.FLAT | am.FALLBACK, 77, 77, 1234, 1234, 0, 0.0)) == [
        "all 1234 counted frames share level bin 77: fixed rule used"]
    assert av.assess(R(89, am.FLAT, 77, 77, 1234, 1234, 0, 0.0)) == ["all 1234 counted frames share level bin 77"]
    assert av.assess(R(40, am.CLAMPED_LO, 21, 23, 1200, 1200, 0, 0.78)) == ["threshold clamped up to bin 40"]
    assert av.assess(R(120, am.CLAMPED_HI, 100, 180, 900, 900, 400, 1.0)) == ["threshold clamped down to bin 120"]
    assert av.assess(R(170, am.FLAT | am.CLAMPED_HI, 150, 150, 9, 9, 0, 0.0)) == [
        "all 9 counted frames share level bin 150", "threshold clamped down to bin 170"]
    # eta is reported only against a bound the caller passes: the calibration ships none
    assert av.DEFAULT_MIN_ETA is None
    assert av.assess(R(42, 0, 40, 96, 10700, 10700, 2800, 0.31), 0.5) == ["levels do not split into two classes (eta 0.31 < 0.50)"]
    assert av.assess(R(42, 0, 40, 96, 10700, 10700, 2800, 0.5), 0.5) == []
    assert av.assess(R(100, am.EMPTY | am.FALLBACK, -1, -1, 4, 0, 0, 0.0), 0.5) == [
        "no frame at or above the silence bin (4 frames): fixed rule used"]
    # the model's records go through record_of unchanged
    from ffsubsync_amd import _native

    row = np.zeros(1, _native.VAD_THRESHOLD_DTYPE)
    for i, name in enumerate(am.FIELDS):
        row[name] = i + 1
    got = av.record_of(row[0])
    assert [getattr(got, name) for name in am.FIELDS] == list(range(1, 9)) and isinstance(got.eta, float) and isinstance(got.n_frames, int)


def test_the_defaults_follow_the_rules_from_the_committed_calibration():
    """The shipped rule, lo_bin, floor_ppm, margin_bins and eta bound recomputed from the class histograms of
    profiles/adaptive_vad_calibration.json by the rules of profiles/adaptive_vad_calibrate.py, and the figures the
    documents quote."""
    from ffsubsync_amd import adaptive_vad as av

    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    try:
        import adaptive_vad_calibrate as cal
    finally:
        sys.path.pop(0)
    data = json.load(open(CALIBRATION))
    files = data["files"]
    assert data["gains_db"] == [0, -10, -20, -30, -40] and data["durations"] == [600, 3600] and data["seeds"] == 6
    assert {(f["duration"], f["kind"], f["gain_db"]) for f in files} == {
        (d, k, g) for d in (600, 3600) for k in ("mixed", "no_speech") for g in data["gains_db"]}
    assert {f["silence"] for f in files} == {0.0, 0.12, 0.4} and len(files) == (6 + 3) * 2 * 5
    shipped = cal.derive(files)
    assert shipped == data["shipped"]
    assert av.DEFAULT_RULE == shipped["rule"] and av.DEFAULT_LO_BIN == shipped["lo_bin"]
    assert av.DEFAULT_FLOOR_PPM == shipped["floor_ppm"] and av.DEFAULT_MARGIN_BINS == shipped["margin_bins"]
    assert av.DEFAULT_MIN_ETA == shipped["min_eta"] and (shipped["min_eta"] is None) == (not shipped["separate"])
    # what the documents quote
    assert round(shipped["otsu_worst_error"]["0"], 3) == 0.196 and round(shipped["otsu_worst_error"]["20"], 3) == 0.252
    assert round(shipped["eta_good_min"], 2) == 0.76 and round(shipped["eta_no_speech_max"], 3) == 0.999
    worst = lambda lo, gains: max(cal.evaluate(cal.sparse_to_dense(f["class_hist"]), rule=am.OTSU, lo_bin=lo, t_min=lo + 1)[0]
                                  for f in files if f["kind"] == "mixed" and f["gain_db"] in gains)
    assert worst(1, (0, -10, -20, -30)) == 0.0 and worst(20, (0, -10, -20)) == 0.0 and worst(20, (-30,)) > 0.25
    by_gain = {r["gain_db"]: r for r in data["by_gain"]}
    assert by_gain[-30]["fixed"]["recall_min"] == 0.0 and by_gain[-40]["fixed"]["recall_min"] == 0.0
    assert by_gain[-20]["fixed"]["recall_min"] < 0.2 and by_gain[0]["fixed"]["recall_min"] == 1.0
    assert all(by_gain[g]["otsu"]["recall_min"] > 0.999 for g in by_gain)
    # an energy rule labels loud music as speech: wherever the speech is found, so is all of the music
    assert all(by_gain[g]["otsu"]["music_min"] == 1.0 for g in by_gain) and by_gain[0]["fixed"]["music_min"] == 1.0
