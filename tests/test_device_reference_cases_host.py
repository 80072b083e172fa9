"""The case table of tests/device_reference_cases.py holds what it names, so tests/test_gpu_device_references.py cannot be
vacuous: the forms carry the bits and the poison they promise, the lengths and densities are those the GPU tests are
there for, and the models' answers on the reused problems would change if a level, a pointer or a length mask were lost.
Host only (numpy models, the oracle and ``exact_reference``); no device, no library call."""
import numpy as np

import device_reference_cases as dc
import resample_edge_cases as rc
import stability_cases as sc
import surrogate_cases as cases


def _references():
    """[(name, 0/1 vector)] of every reference the GPU tests pass in a device form, the dense one left out."""
    out = [("sweep %d" % s, dc.bits_of(dc.sweep_problem(s).reference)) for s in dc.SWEEP_SEEDS]
    out += [("sync %d" % i, dc.bits_of(ref)) for i, (ref, _) in enumerate(cases.sync_problems())]
    out += [("track %d" % j, ref) for j, (ref, _) in enumerate(dc.track_problems())]
    out += [("tiny %d" % i, dc.bits_of(rc.tiny_file(i)[0])) for i in range(len(rc.TINY_FILES))]
    return out + [("silent", dc.silent_reference()), ("pcm", dc.pcm_speech())]


def test_the_levels_of_every_case_are_stated():
    assert dc.LEVELS == ((0.0, 1.0), (0.1, 1.0)) and dc.FORMS[0] == "host" and set(dc.SLICE_WORDS) == {"slice1", "slice3"}
    assert set(dc.SWEEP_LEVELS) == set(dc.SWEEP_RANGE) == set(dc.SWEEP_FORMS) == set(dc.SWEEP_SEEDS)
    assert set(dc.SWEEP_LEVELS.values()) == set(dc.LEVELS)
    for s in dc.SWEEP_SEEDS:  # every sweep call mixes the control with device forms, and every device form is in one
        assert "host" in dc.SWEEP_FORMS[s] and len(dc.SWEEP_FORMS[s]) >= 3
        lo, hi = dc.SWEEP_RANGE[s]
        assert lo < dc.sweep_problem(s).true_ratio < hi
    assert {f for s in dc.SWEEP_SEEDS for f in dc.SWEEP_FORMS[s]} == set(dc.FORMS)
    assert len(dc.TRACK_LEVELS) == len(dc.TRACK_FORMS) == len(dc.track_problems()) and set(dc.TRACK_LEVELS) == set(dc.LEVELS)
    assert set(dc.TRACK_FORMS) == {"slice1", "slice3", "bytes"} == set(dc.TINY_FORMS) and len(dc.TINY_FORMS) == len(rc.TINY_FILES)
    assert {(f, lv) for f, lv in zip(dc.TRACK_FORMS, dc.TRACK_LEVELS)} >= {(f, dc.LEVELS[1]) for f in ("slice1", "slice3", "bytes")}
    assert [f for f, _ in dc.DENSE_FORMS] == list(dc.DEVICE_FORMS) and {lv for _, lv in dc.DENSE_FORMS} == set(dc.LEVELS)
    assert dc.SILENT_LEVELS == (0.0, 1.0) and dc.PCM_LEVELS == (0.1, 1.0)
    for lv in dc.LEVELS:
        values = dc.host_values([0, 1, 1, 0], lv)
        assert values.dtype == np.float64 and values.tolist() == [lv[0], lv[1], lv[1], lv[0]]


def test_one_dense_reference_and_no_other():
    dense = dc.dense_reference()
    assert dc.boundaries(dense) >= dc.LIST_CAP and dc.boundaries(dense[:dc.DENSE_HEAD]) == 40000
    for name, v in _references():
        assert 0 < v.size and dc.boundaries(v) < dc.LIST_CAP, name
    assert not dc.silent_reference().any() and dc.boundaries(dc.silent_reference()) == 0


def test_the_length_residues_occur():
    lens = [ref.size for ref, _ in dc.track_problems()] + [dc.dense_reference().size]
    assert {0, 1, 31} <= {n % 32 for n in lens}
    # the reused tiny files and tracks alone do not supply them: that is why three tracks were added
    reused = [rc.tiny_file(i)[0].size for i in range(len(rc.TINY_FILES))] + [ref.size for ref, _ in rc.track_problems()]
    assert not {0, 1, 31} & {n % 32 for n in reused}
    assert [n % 32 for n in dc.RESIDUE_LENGTHS] == [0, 1, 31]
    # the three residues in a slice form, in the byte form and with the low level 0.1
    by_residue = {ref.size % 32: (f, lv) for (ref, _), f, lv in zip(dc.track_problems(), dc.TRACK_FORMS, dc.TRACK_LEVELS)}
    assert {by_residue[r][0] for r in (0, 1, 31)} == {"slice1", "slice3", "bytes"}
    assert by_residue[31][0] in dc.SLICE_WORDS  # poisoned bits behind the last sample of a word that is nearly full
    assert dc.dense_reference().size % 32 == 31


def test_the_sync_problems_cover_every_form_with_a_matched_and_a_wrong_file():
    kinds = cases.sync_kinds()
    assert len(kinds) == len(cases.sync_problems()) == 12
    seen = {(dc.sync_form(i), kinds[i]) for i in range(12)}
    assert seen == {(f, k) for f in dc.FORMS for k in ("matched", "wrong")}
    assert dc.sync_form(0) == "host" and [dc.sync_form(i) for i in range(6)] == list(dc.FORMS)


def test_every_slice_form_is_misaligned_poisoned_and_still_holds_the_vector():
    vectors = [v for _, v in _references()] + [dc.dense_reference()]
    for form, start in dc.SLICE_WORDS.items():
        assert (4 * start) % 16 in (4, 12)
        for v in vectors:
            buf, first = dc.slice_image(v, form)
            n, nw = v.size, dc.n_words(v.size)
            assert first == start and buf.dtype == np.uint32 and buf.size == start + nw + dc.GUARD_WORDS
            # every bit that is not a sample is set: the words in front and behind, and the last word's bits >= n
            assert (buf[:first] == 0xFFFFFFFF).all() and (buf[first + nw:] == 0xFFFFFFFF).all()
            bits = np.unpackbits(buf[first:first + nw].view(np.uint8), bitorder="little")
            assert bits.size == 32 * nw and bits[n:].all()
            # and a read with the length mask gives the vector
            assert np.array_equal(dc.unpack(buf[first:first + nw], n), v)
    assert {(4 * s) % 16 for s in dc.SLICE_WORDS.values()} == {4, 12}
    # the packed form is the clean control: zero bits behind the vector
    for v in vectors[:3] + vectors[-1:]:
        words = dc.packed_image(v)
        assert words.size == dc.n_words(v.size) and np.array_equal(dc.unpack(words, v.size), v)
        assert not np.unpackbits(words.view(np.uint8), bitorder="little")[v.size:].any()
    # a vector whose last word is partly used exists in a slice form with a zero sample in front of the poison: a reader
    # of the bits >= n would see a run that is not there
    assert any(v.size % 32 and not v[-1] for v in vectors)


def test_the_profile_answers_are_not_degenerate():
    changed = 0
    for s in dc.SWEEP_SEEDS:
        grids = [dc.exact_profile(s, lv) for lv in dc.LEVELS]
        assert np.array_equal(grids[0][0], grids[1][0]) and 5 <= grids[0][0].size <= 8
        changed += sum(a[1] != b[1] for a, b in zip(grids[0][1], grids[1][1]))
        assert len({o for o, _ in grids[0][1]}) > 1  # the offset depends on the ratio
    assert changed >= 1  # a dropped ``lo`` changes a score


def test_the_sweep_answers_are_not_degenerate():
    import exact_reference as er
    from oracle import raster_oracle as ro

    for s in dc.SWEEP_SEEDS:
        p, want = dc.sweep_problem(s), dc.model_sweep(s)
        assert len(want["report"]["peaks"]) >= 1 and want["offset"] != 0
        assert abs(want["ratio"] - p.true_ratio) <= want["step"] / 16 * (1 + 1e-9)
        assert 5 <= want["grid"].size <= 8 and want["fine"][0].size <= 3 * 33 + 7
        # the oracle's argmax at the answer is not decided by its FFT's rounding: the exact reference names the same lag
        sub = ro.rasterize(p.track[0], p.track[1], p.track[2], want["ratio"], 100, 0) != 0
        exact = er.candidate(dc.bits_of(p.reference), sub, dc.SWEEP_LEVELS[s], (0.0, min(1.0 / want["ratio"], 1.0)), dc.W)
        assert exact["offset"] == want["offset"] and exact["n_at_max"] == 1
        assert abs(exact["score"] - want["score"]) <= 1e-9 * abs(want["score"])


def test_the_sync_answers_are_not_degenerate():
    from ffsubsync_amd import surrogate

    for i, kind in enumerate(cases.sync_kinds()):
        if kind == "matched":
            assert cases.model_sync(i, surrogate.DEFAULT_MIN_Z)["offset"] != 0 and sc.model_sync(i)["offset"] != 0, i
    for j in range(len(dc.track_problems())):
        null, stable = dc.track_null_model(j), dc.track_stable_model(j)
        assert (null["ratio"], null["offset"], null["score"]) == (stable["ratio"], stable["offset"], stable["score"]), j
    # on the tiny tracks with the low level 0.1 the level decides a score: the model with (0, 1) gives another one
    import surrogate_model as sm

    moved = 0
    for j, lv in enumerate(dc.TRACK_LEVELS):
        if lv != dc.LEVELS[0]:
            ref, track = dc.track_problems()[j]
            plain = sm.null_sync(dc.host_values(ref, dc.LEVELS[0]), track, rc.TRACK_W, None, rc.TRACK_K, 1, rc.TRACK_SEED, j, rc.TRACK_MIN_Z)
            moved += plain["score"] != dc.track_null_model(j)["score"]
    assert moved >= 1
    # the reused tiny tracks with levels (0, 1): the levels argument of the models changes nothing there
    for j in range(len(rc.TRACK_CUES)):
        if dc.TRACK_LEVELS[j] == dc.LEVELS[0]:
            assert dc.track_null_model(j)["scores"].tolist() == rc.track_null_model(j)["scores"].tolist()
            assert dc.track_stable_model(j)["record"] == rc.track_stable_model(j)["record"]


def test_the_dense_and_silent_answers():
    grid = dc.small_grid(dc.DENSE_RANGE[0], dc.DENSE_RANGE[1], dc.DENSE_TOLERANCE)
    assert 8 <= grid.size <= 40
    for lv in dc.LEVELS:
        recs = dc.exact_records("dense", lv, tuple(grid.tolist()))
        assert all(f == 0 for _, _, f in recs) and len({s for _, s, _ in recs}) > 1
    a, b = (dc.exact_records("dense", lv, tuple(grid.tolist())) for lv in dc.LEVELS)
    assert any(x[1] != y[1] for x, y in zip(a, b))
    silent = dc.exact_records("silent", dc.SILENT_LEVELS, tuple(grid.tolist()))
    assert all(f == 0 for _, _, f in silent)
    # the model sweep of the silent reference: the oracle's argmax at the answer is the exact reference's, without a tie
    import sweep_model

    lo, hi = dc.DENSE_RANGE
    want = sweep_model.sweep(np.zeros(dc.silent_reference().size), dc.small_track(), dc.SMALL_W, lo=lo, hi=hi,
                             tolerance_samples=dc.DENSE_TOLERANCE, top_k=1)
    _answer_is_not_decided_by_rounding(want, dc.silent_reference(), dc.small_track(), dc.SILENT_LEVELS, dc.SMALL_W)


def _answer_is_not_decided_by_rounding(want, ref01, track, levels, w):
    import exact_reference as er
    from oracle import raster_oracle as ro

    sub = ro.rasterize(track[0], track[1], track[2], want["ratio"], 100, 0) != 0
    exact = er.candidate(ref01, sub, levels, (0.0, min(1.0 / want["ratio"], 1.0)), w)
    assert exact["offset"] == want["offset"] and exact["n_at_max"] == 1
    assert abs(exact["score"] - want["score"]) <= 1e-9 * abs(want["score"])


def test_the_golden_section_files():
    from ffsubsync_amd.constants import candidate_ratios
    import sweep_model

    assert [float(r) for r in candidate_ratios()] == [float(r) for r in sweep_model.SEVEN]  # (ratio_index means the same)
    files = dc.gss_files()
    assert len(files) == len(dc.GSS_FORMS) == 3 and {lv for _, lv in dc.GSS_FORMS} == set(dc.LEVELS)
    assert all(f in dc.DEVICE_FORMS for f, _ in dc.GSS_FORMS) and "slice3" in [f for f, _ in dc.GSS_FORMS]
    for v, (s, e, m) in files:
        assert v.dtype == bool and 30000 < v.size < 45000 and 0 < dc.boundaries(v) < dc.LIST_CAP and len(s) == 120


def test_the_pcm_leg():
    import adaptive_vad_model as am
    import ingest_reference as ir
    from ffsubsync_amd import adaptive_vad as av

    assert dc.pcm_pick_args() == dict(rule=am.RULES[av.DEFAULT_RULE], lo_bin=av.DEFAULT_LO_BIN, t_min=av.DEFAULT_LO_BIN + 1,
                                      floor_ppm=av.DEFAULT_FLOOR_PPM, margin_bins=av.DEFAULT_MARGIN_BINS)
    fl, files = am.gain_files()
    assert tuple(files) == dc.PCM_GAINS and fl == 160
    speech = dc.pcm_speech()
    assert speech.size == 3000 and 0.2 < speech.mean() < 0.6
    for g in dc.PCM_GAINS:  # the three gains: the same labels under the adaptive rule
        assert np.array_equal(am.detect(files[g], fl, **dc.pcm_pick_args())[0], speech), g
    assert np.array_equal(ir.energy_labels(files[0], fl, 50.0)[0], speech)  # the loud file under the fixed rule: the same
    assert not ir.energy_labels(files[-30], fl, 50.0)[0].any()  # the quiet one: silence
    start, end, meta = dc.pcm_track()
    assert start.size >= 16 and (end > start).all() and (start >= 0).all() and not meta.any()
    m = dc.pcm_models()
    assert m["best"] == dc.PCM_RATIO_INDEX and m["seven"][m["best"]][0] == dc.PCM_OFFSET
    assert (m["null"]["ratio"], m["null"]["offset"], m["null"]["score"]) == (dc.pcm_ratio(),) + m["seven"][m["best"]]
    assert (m["stable"]["offset"], m["stable"]["score"]) == m["seven"][m["best"]]
    assert m["null"]["trusted"] and m["stable"]["stable"] and m["null"]["blocks"] >= 8
    lo, hi = dc.pcm_sweep_range()
    assert m["sweep"]["offset"] == dc.PCM_OFFSET and lo < m["sweep"]["ratio"] < hi and len(m["sweep"]["report"]["peaks"]) == 1
    assert abs(m["sweep"]["ratio"] - dc.pcm_ratio()) <= m["sweep"]["step"] / 16
    _answer_is_not_decided_by_rounding(m["sweep"], speech, dc.pcm_track(), dc.PCM_LEVELS, dc.SMALL_W)
    quiet = dc.pcm_models(silent=True)
    assert quiet["null"]["score"] != m["null"]["score"]
    _answer_is_not_decided_by_rounding(quiet["sweep"], np.zeros(speech.size, bool), dc.pcm_track(), dc.PCM_LEVELS, dc.SMALL_W)
