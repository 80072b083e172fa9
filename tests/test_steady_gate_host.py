"""The steady-run gate's model against itself on the CPU (tests/steady_gate_model.py): the sequential definition equals
the vectorised restatement and the kernels' tile / carry decomposition restated in Python, the three identities of the
contract hold, the refusals of the exports need no device, and the shipped defaults are what
profiles/steady_gate_calibration.json derives -- every figure of it recomputed from the model."""
import json
import os
import sys

import numpy as np

import steady_gate_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return np.array_equal(a[0], b[0]) and gm.record_tuple(a[1]) == gm.record_tuple(b[1])


def test_sequential_equals_vectorised_and_tiled_on_random_cases():
    """400 random small files over every class mix, thresholds, dips and limits; the tiled form with tiles of 8, 32 and 64
    frames and threads of 4 and 16, so stretches cross many tile and thread edges."""
    rng = np.random.RandomState(1)
    for k in range(400):
        n = int(rng.randint(0, 300))
        lv = gm.random_levels(rng, n, (0.5, 0.2, 0.05)[k % 3]) if n else np.zeros(0, np.uint8)
        t, dip, max_run = (100, 0, 256, 96, 121)[k % 5], (0, 10, 90, 255)[k % 4], int(rng.randint(1, 40))
        want = gm.gate_sequential(lv, t, dip, max_run)
        assert _same(want, gm.gate_vectorised(lv, t, dip, max_run)), (k, n, t, dip, max_run)
        tile, fpt = ((8, 4), (32, 16), (64, 4), (64, 16))[k % 4]
        assert _same(want, gm.gate_tiled(lv, t, dip, max_run, tile, fpt)), (k, n, t, dip, max_run, tile, fpt)


def test_sequential_equals_vectorised_and_tiled_on_the_case_table():
    """Every case the device test runs, at the kernels' own tile and thread widths."""
    for name, lv, t, dip, max_run in gm.stretch_cases():
        want = gm.gate_sequential(lv, t, dip, max_run)
        assert _same(want, gm.gate_vectorised(lv, t, dip, max_run)), name
        assert _same(want, gm.gate_tiled(lv, t, dip, max_run)), name
    tiles, lv, t, dip, max_run = gm.scan_cases()[1]
    want = gm.gate_vectorised(lv, t, dip, max_run)
    assert want[1]["longest_run"] == max_run == (tiles - 4) * gm.TILE and want[1]["n_rejected"] == 0
    assert _same(want, gm.gate_sequential(lv, t, dip, max_run))
    assert gm.gate_vectorised(lv, t, dip, max_run - 1)[1]["n_rejected"] == 1


def test_the_case_table_reaches_what_it_names():
    cases = {name: gm.gate_sequential(lv, t, dip, mr) + (lv,) for name, lv, t, dip, mr in gm.stretch_cases()}
    T = gm.TILE
    sp, rec, _ = cases["across three tiles of keep frames"]
    assert rec["n_stretches"] == 1 and rec["longest_run"] == 3 * T + 5 and sp.sum() == 5 and not rec["n_rejected"]
    assert cases["the same, one frame too long"][1]["n_rejected"] == 1 and not cases["the same, one frame too long"][0].any()
    assert cases["dip t: NO_QUIET"][1]["flags"] == gm.NO_QUIET and cases["dip t: NO_QUIET"][1]["n_stretches"] == 1
    rec = cases["dip one below t"][1]   # level 1 keeps the first stretch open, level 0 closes it
    assert rec["flags"] == 0 and rec["n_stretches"] == 2 and rec["longest_run"] == 50 and rec["n_kept"] == 50
    assert cases["t 0 too long: ALL_REJECTED"][1]["flags"] == gm.NO_QUIET | gm.ALL_REJECTED
    assert cases["trailing keep frames over the edge"][0].sum() == 10
    assert cases["trailing keep frames over the edge, one active frame too many"][0].sum() == 0
    assert cases["exactly max_run"][0].sum() == 100 and cases["max_run + 1"][0].sum() == 0
    assert cases["max_run 1"][0].sum() == 3 and cases["max_run 1 with keep frames inside"][0].sum() == 1
    assert cases["t 256: nothing active"][1]["n_active"] == 0


def test_identities_of_the_contract():
    rng = np.random.RandomState(2)
    for k in range(60):
        n = int(rng.randint(1, 600))
        lv = gm.random_levels(rng, n, (0.3, 0.05)[k % 2])
        t, max_run = 100, int(rng.randint(1, 80))
        plain = gm.classes(lv, t, 0)[0]
        # max_run >= n: the plain labels, whatever the dip
        for dip in (0, 10, 255):
            assert np.array_equal(gm.gate_sequential(lv, t, dip, n)[0], plain)
        # dip_bins = 0: the plain labels without the runs of ones longer than max_run
        assert np.array_equal(gm.gate_sequential(lv, t, 0, max_run)[0], gm.remove_long_runs(plain, max_run))
        # the kept set shrinks as dip_bins grows
        kept = [gm.gate_sequential(lv, t, dip, max_run)[0] for dip in (0, 4, 5, 10, 90, 100)]
        for small, large in zip(kept, kept[1:]):
            assert not (large & ~small).any()


def test_too_long_is_the_plain_labels():
    lv = np.zeros(gm.MAX_FRAMES + 1, np.uint8)
    lv[5:9] = 200
    for f in (gm.gate_sequential, gm.gate_vectorised, gm.gate_tiled):
        sp, rec = f(lv, 100, 0, 2)
        assert sp.sum() == 4 and rec["flags"] == gm.TOO_LONG and rec["n_frames"] == lv.size
        assert rec["n_active"] == rec["n_kept"] == rec["n_stretches"] == 0


def test_refusals_and_workspace_sizes_need_no_device():
    from ffsubsync_amd import _native

    assert _native.VAD_GATE_TILE == gm.TILE and _native.VAD_GATE_DTYPE.names == gm.FIELDS
    assert (_native.VAD_GATE_NO_QUIET, _native.VAD_GATE_ALL_REJECTED, _native.VAD_GATE_TOO_LONG) == (gm.NO_QUIET, gm.ALL_REJECTED, gm.TOO_LONG)
    gm.check_refusals(_native.load())


def test_python_checks_come_before_any_native_call():
    import pytest

    from ffsubsync_amd import adaptive_vad as av

    class Dev:   # passes for a CUDA vector up to the point where the arguments have been checked
        is_cuda = True

    for kw in (dict(dip_bins=-1), dict(dip_bins=256), dict(dip_bins=1.5), dict(max_run=0), dict(max_run=2 ** 31), dict(max_run=True),
               dict(non_speech_label=float("nan"))):
        with pytest.raises(ValueError):
            av.steady_gate(Dev(), 100, **kw)
    for thr in (-1, 257, 1.0, None):
        with pytest.raises(ValueError, match="threshold"):
            av.steady_gate(Dev(), thr)
    with pytest.raises(ValueError, match="levels"):
        av.steady_gate(np.zeros(4, np.uint8), 100)
    with pytest.raises(ValueError, match="max_run"):
        av.detect_device_gated(Dev(), 100, 16000, 0.0, max_run=0)
    with pytest.raises(ValueError, match="dip_bins"):
        av.detect_pinned_stream_gated(Dev(), 100, 16000, 0.0, dip_bins=300)
    with pytest.raises(ValueError, match="unknown parameter"):
        av.detect_device_gated(Dev(), 100, 16000, 0.0, bogus=1)
    rec = av.GateRecord(100, 0, 4, 1, 1500, 6000, 3000, 1500)
    assert av.assess_gate(rec) == [] and len(av.assess_gate(rec, 0.4)) == 1 and av.assess_gate(rec, 0.5) == []
    assert "longer than the limit" in av.assess_gate(av.GateRecord(100, gm.ALL_REJECTED, 1, 1, 3000, 6000, 3000, 0))[0]
    assert "plain labels" in av.assess_gate(av.GateRecord(100, gm.TOO_LONG, 0, 0, 0, gm.MAX_FRAMES + 1, 0, 0))[0]
    assert "close a stretch" in av.assess_gate(av.GateRecord(0, gm.NO_QUIET, 0, 0, 0, 10, 0, 0))[0]
    with pytest.raises(ValueError):
        av.assess_gate(rec, 1.5)


def test_defaults_are_what_the_calibration_derives():
    """profiles/steady_gate_calibration.json: every figure of its table recomputed with the model from the run-length
    coded class / band sequences it keeps, the recommendation re-derived by the script's rule, and the shipped defaults
    equal to it."""
    from ffsubsync_amd import adaptive_vad as av
    from ffsubsync_amd.constants import DEFAULT_MAX_SUBTITLE_SECONDS

    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    try:
        import steady_gate_calibrate as cal
    finally:
        sys.path.pop(0)
    doc = json.load(open(os.path.join(ROOT, "profiles", "steady_gate_calibration.json")))
    assert doc["max_run"] == av.DEFAULT_MAX_RUN == av.default_max_run(100) == DEFAULT_MAX_SUBTITLE_SECONDS * 100 == 1000
    assert doc["dips"] == list(cal.DIPS) and doc["dips"][0] == 0
    for f in doc["files"]:
        got = cal.figures(f["runs"], doc["max_run"])
        assert got == f["figures"], (f["seed"], f["gain_db"])
    assert cal.recommend(doc["files"]) == doc["shipped"]["dip_bins"] == av.DEFAULT_DIP_BINS
    assert cal.by_gain(doc["files"]) == doc["by_gain"]
    found = [f for f in doc["files"] if f["finds_speech"]]
    assert found and all(f["figures"]["0"]["music_before"] == 1.0 and f["figures"]["0"]["music_after"] == 0.0 for f in found)
