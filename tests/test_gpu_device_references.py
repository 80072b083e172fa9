"""Device-resident references through ``batch_gss.PreparedRatioSolve``: ``fit_gss_batch``, ``ratio_profile_batch`` /
``sweep_sync``, ``null_sync`` and ``stable_sync`` with ``DeviceRaster`` references used in place -- packed, with attached
run lists, as bytes, as misaligned slices of a poisoned buffer, with a low level that is not 0, mixed with host vectors
in one call -- a reference too dense for a boundary list, a silent one, and VAD rasters handed to the solvers straight
from the PCM.  The cases are tests/device_reference_cases.py's (held to what they name by
tests/test_device_reference_cases_host.py).  Expected values come from tests/exact_reference.py, the oracle and the numpy
models, never from the host-vector branch of the code under test; that branch must agree as well.  Comparisons are those
of tests/test_gpu_ratio_sweep.py, tests/test_gpu_surrogate.py, tests/test_gpu_stability.py and
tests/test_gpu_resample_edges.py: exact against the exact reference and the integer models, rel 1e-9 on oracle scores.
Need a real MI355X."""
import math

import numpy as np
import pytest

import device_reference_cases as dc
import resample_edge_cases as rc
import stability_cases as sc
import stability_model as stm
import surrogate_cases as cases
import surrogate_model as sm
import sweep_model
import test_gpu_quality as tgq
import test_gpu_resample_edges as tre
import test_gpu_stability as tst
import test_gpu_surrogate as tsu

pytestmark = pytest.mark.gpu


def _pairs(rec):
    return [(int(o), float(s)) for o, s in zip(rec["offset"], rec["score"])]


def _check_null_result(r, model, where):
    """One ``NullSyncResult`` against the model's dict, as tests/test_gpu_resample_edges.py compares them."""
    assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), where
    tsu._check_record(vars(r.null), model["record"])
    assert r.p == model["p"] and r.trusted == model["trusted"], where
    assert r.z == model["z"] or math.isclose(r.z, model["z"], rel_tol=1e-9), where  # (from null_mean / null_std)
    assert r.reasons == model["reasons"], (where, r.reasons, model["reasons"])


def _check_stable_result(r, model, where):
    assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), where
    tst._check_record(vars(r.record), model["record"])
    assert r.interval_samples == model["interval_samples"] and r.share_within == model["share_within"], where
    assert r.stable is model["stable"] and r.reasons == model["reasons"], (where, r.reasons, model["reasons"])


def _check_sweep_result(r, want, where):
    """One ``SweepSyncResult`` against ``sweep_model.sweep``, as tests/test_gpu_ratio_sweep.py compares them."""
    assert (repr(r.ratio), r.offset, repr(r.coarse_ratio)) == (repr(want["ratio"]), want["offset"], repr(want["coarse_ratio"])), where
    assert r.score == pytest.approx(want["score"], rel=1e-9), where
    assert (r.profile.n_points, r.profile.n_skipped, len(r.profile.peaks)) == (want["grid"].size, want["report"]["n_skipped"],
                                                                               len(want["report"]["peaks"])), where
    assert (r.profile.flags & sweep_model.FLAT) == (want["report"]["flags"] & sweep_model.FLAT), where


# ---- 1. the ratio profile in every form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", dc.LEVELS, ids=["lo0", "lo0.1"])
def test_ratio_profile_of_every_form_equals_the_exact_reference(levels):
    """The two sweep problems in all six forms in ONE call (twelve files, host and device references alternating): every
    record's (offset, score) is the exact reference's with the reference levels given, the score as a value."""
    import torch
    from ffsubsync_amd import ratio_sweep

    entries = [(s, form) for s in dc.SWEEP_SEEDS for form in dc.FORMS]
    problems = [(dc.build(form, dc.sweep_problem(s).reference, levels, torch), dc.sweep_problem(s).track) for s, form in entries]
    lo, hi = dc.PROFILE_RANGE
    prof = ratio_sweep.ratio_profile_batch(problems, lo=lo, hi=hi)
    assert prof.stats["lists"] is True and "careful_files" not in prof.stats and prof.stats["files"] == len(entries)
    recs = prof.records()
    seen = 0
    for (s, form), grid, rec in zip(entries, prof.grids, recs):
        want_grid, want = dc.exact_profile(s, levels)
        assert np.array_equal(grid, want_grid) and 5 <= grid.size <= 8, (s, form)
        assert not (rec["flags"] & 3).any(), (s, form)
        assert _pairs(rec) == want, (s, form, _pairs(rec), want)
        seen += 1
    assert seen == len(dc.SWEEP_SEEDS) * len(dc.FORMS) == 12
    # the second check: the same files as host vectors give the same table, byte for byte
    host = ratio_sweep.ratio_profile_batch([(dc.build("host", dc.sweep_problem(s).reference, levels, torch), dc.sweep_problem(s).track)
                                            for s, _ in entries], lo=lo, hi=hi)
    total = int(prof.first[-1])
    assert np.array_equal(host.first, prof.first) and host.stats["lists"] is True
    assert prof.table[:total * 24].cpu().numpy().tobytes() == host.table[:total * 24].cpu().numpy().tobytes()


# ---- 2. sweep_sync ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", dc.SWEEP_SEEDS)
def test_sweep_sync_of_device_references_mixed_with_host_vectors_equals_the_model(seed):
    import torch
    from ffsubsync_amd import ratio_sweep

    p, levels, (lo, hi) = dc.sweep_problem(seed), dc.SWEEP_LEVELS[seed], dc.SWEEP_RANGE[seed]
    forms = dc.SWEEP_FORMS[seed]
    results = ratio_sweep.sweep_sync([(dc.build(f, p.reference, levels, torch), p.track) for f in forms], lo=lo, hi=hi)
    want = dc.model_sweep(seed)
    seen = 0
    for form, r in zip(forms, results):
        _check_sweep_result(r, want, (seed, form))
        assert abs(r.ratio - p.true_ratio) <= want["step"] / 16 * (1 + 1e-9), (seed, form, r.ratio)
        assert (r.ratio, r.offset, r.score, r.reasons) == (results[0].ratio, results[0].offset, results[0].score, results[0].reasons)
        seen += 1
    assert seen == len(forms) == len(results) and "host" in forms


# ---- 3. a reference too dense for a boundary list ----------------------------------------------------------------------------
def _dense_problems(torch):
    return [(dc.build(form, dc.dense_reference(), levels, torch), dc.small_track()) for form, levels in dc.DENSE_FORMS]


def test_dense_device_references_take_the_bit_rasters_in_place():
    """Every device form of the dense reference in one call: the sweep falls back to the bit rasters, which read the
    rasters through their own pointers -- the ``slice3`` one 12 bytes off a 16-byte boundary with ones all around it."""
    import torch
    from ffsubsync_amd import ratio_sweep

    lo, hi = dc.DENSE_RANGE
    prof = ratio_sweep.ratio_profile_batch(_dense_problems(torch), dc.SMALL_SECONDS, lo=lo, hi=hi, tolerance_samples=dc.DENSE_TOLERANCE)
    assert prof.stats["lists"] is False
    grid = dc.small_grid(lo, hi, dc.DENSE_TOLERANCE)
    seen = 0
    for (form, levels), g, rec in zip(dc.DENSE_FORMS, prof.grids, prof.records()):
        want = dc.exact_records("dense", levels, tuple(grid.tolist()))
        assert np.array_equal(g, grid), form
        assert not (rec["flags"] & 1).any(), form
        assert _pairs(rec) == [(o, s) for o, s, _ in want], (form, _pairs(rec), want)
        seen += 1
    assert seen == len(dc.DENSE_FORMS) == len(dc.DEVICE_FORMS)
    # the control: the host vector takes the same path and gives the same records
    host = ratio_sweep.ratio_profile_batch([(dc.build("host", dc.dense_reference(), dc.LEVELS[0], torch), dc.small_track())],
                                           dc.SMALL_SECONDS, lo=lo, hi=hi, tolerance_samples=dc.DENSE_TOLERANCE)
    assert host.stats["lists"] is False
    assert _pairs(host.records()[0]) == [(o, s) for o, s, _ in dc.exact_records("dense", dc.LEVELS[0], tuple(grid.tolist()))]


@pytest.mark.parametrize("entry", ["null_sync", "stable_sync"])
def test_a_dense_device_reference_is_refused_by_name_once_counted_and_the_next_call_is_sound(entry):
    import torch
    from ffsubsync_amd import stability, surrogate

    null_args = dict(n_surrogates=rc.TRACK_K, block_units=1, seed=rc.TRACK_SEED, min_z=rc.TRACK_MIN_Z)
    stable_args = dict(n_subsamples=rc.TRACK_K, block_runs=1, seed=rc.TRACK_SEED, tol=rc.TRACK_TOL, min_share=rc.TRACK_MIN_SHARE)
    call = (lambda pr: surrogate.null_sync(pr, rc.TRACK_SECONDS, **null_args)) if entry == "null_sync" else \
        (lambda pr: stability.stable_sync(pr, rc.TRACK_SECONDS, **stable_args))
    ref, track = dc.track_problems()[0]
    good = (dc.build(dc.TRACK_FORMS[0], ref, dc.TRACK_LEVELS[0], torch), track)
    seen = 0
    for form, levels in dc.DENSE_FORMS:
        dense = (dc.build(form, dc.dense_reference(), levels, torch), dc.small_track())
        with pytest.raises(ValueError, match=entry + ".*too dense for a boundary list"):
            call([good, dense])  # (a sound file in front of it: the refusal is the call's)
        seen += 1
    assert seen == len(dc.DEVICE_FORMS)
    got = call([good])
    assert len(got) == 1
    if entry == "null_sync":
        _check_null_result(got[0], dc.track_null_model(0), entry)
    else:
        _check_stable_result(got[0], dc.track_stable_model(0), entry)


def _check_gss(got, host_refs, tracks, levels, w):
    """``fit_gss_batch``'s records against the per-file path on the host values, and every recorded (offset, score)
    against the exact reference at the recorded ratio."""
    import exact_reference as er
    from ffsubsync_amd.batch_gss import _fit_gss_batch_per_file
    from oracle import raster_oracle as ro

    want = _fit_gss_batch_per_file(host_refs, tracks, max_offset_samples=w)
    assert len(got) == len(want) == len(host_refs)
    for i, (((score, offset), ratio), ((w_score, w_offset), w_ratio)) in enumerate(zip(got, want)):
        assert (repr(ratio), offset, float(score)) == (repr(w_ratio), w_offset, float(w_score)), i
        s, e, m = tracks[i]
        sub = ro.rasterize(s, e, m, ratio, 100, 0) != 0
        exact = er.candidate(host_refs[i] != levels[i][0], sub, levels[i], (0.0, min(1.0 / ratio, 1.0)), w)
        assert (exact["offset"], exact["score"]) == (offset, float(score)), (i, exact)


def test_fit_gss_batch_on_a_dense_device_reference():
    import torch
    from ffsubsync_amd.batch_gss import fit_gss_batch

    form, levels = dc.DENSE_FORMS[-1]
    assert form == "slice3"
    stats = {}
    got = fit_gss_batch([dc.build(form, dc.dense_reference(), levels, torch)], [dc.small_track()], max_offset_samples=dc.SMALL_W, stats=stats)
    assert stats.get("lists", False) is False  # (absent when a degenerate step sent the call to the per-file path)
    _check_gss(got, [dc.host_values(dc.dense_reference(), levels)], [dc.small_track()], [levels], dc.SMALL_W)


# ---- 4. fit_gss_batch ------------------------------------------------------------------------------------------------------
def test_fit_gss_batch_on_device_references():
    """The three files of tests/test_gpu_raster.py's golden-section test with their references as a misaligned slice, as
    bytes with the low level 0.1 and as a packed raster with attached lists."""
    import torch
    from ffsubsync_amd.batch_gss import fit_gss_batch

    files = dc.gss_files()
    host = [dc.host_values(v, lv) for (v, _), (_, lv) in zip(files, dc.GSS_FORMS)]
    refs = [dc.build(form, v, lv, torch) for (v, _), (form, lv) in zip(files, dc.GSS_FORMS)]
    stats = {}
    got = fit_gss_batch(refs, [t for _, t in files], max_offset_samples=dc.W, stats=stats)
    assert stats["lists"] is True and stats["files"] == 3 and stats["steps"] >= 17
    _check_gss(got, host, [t for _, t in files], [lv for _, lv in dc.GSS_FORMS], dc.W)
    assert len(got) == len(dc.GSS_FORMS) == 3


# ---- 5. null_sync and stable_sync ----------------------------------------------------------------------------------------------
def _sync_problems(torch):
    return [(dc.build(dc.sync_form(i), ref, dc.LEVELS[0], torch), track) for i, (ref, track) in enumerate(cases.sync_problems())]


def test_null_sync_of_the_twelve_problems_in_rotated_forms_equals_the_model():
    import torch
    from ffsubsync_amd import surrogate

    kinds = cases.sync_kinds()
    got = surrogate.null_sync(_sync_problems(torch), 60)
    assert len(got) == len(kinds) == 12
    seen = set()
    for i, (r, kind) in enumerate(zip(got, kinds)):
        model = cases.model_sync(i, surrogate.DEFAULT_MIN_Z)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        tsu._check_record(vars(r.null), model["record"])
        assert math.isclose(r.z, model["z"], rel_tol=1e-9) and r.p == model["p"], i
        assert r.trusted == model["trusted"] == (kind == "matched"), (i, kind, r.z, r.null.n_ge)
        assert [x.split(" ")[0] for x in r.reasons] == [x.split(" ")[0] for x in model["reasons"]], i
        seen.add((dc.sync_form(i), kind))
    assert len(seen) == 2 * len(dc.FORMS)


def test_stable_sync_of_the_twelve_problems_in_rotated_forms_equals_the_model():
    import torch
    from ffsubsync_amd import stability

    kinds = cases.sync_kinds()
    got = stability.stable_sync(_sync_problems(torch), 60, tol=sc.TOL, min_share=sc.MIN_SHARE)
    assert len(got) == len(kinds) == 12
    seen = set()
    for i, (r, kind) in enumerate(zip(got, kinds)):
        model = sc.model_sync(i)
        assert (r.ratio, r.offset, r.score, r.blocks) == (model["ratio"], model["offset"], model["score"], model["blocks"]), i
        tst._check_record(vars(r.record), model["record"])
        assert r.interval_samples == model["interval_samples"] and r.share_within == model["share_within"], i
        assert r.reasons == model["reasons"] and r.stable is model["stable"] is (kind == "matched"), (i, kind, r.share_within)
        seen.add((dc.sync_form(i), kind))
    assert len(seen) == 2 * len(dc.FORMS)


def _track_problems(torch):
    return [(dc.build(form, ref, lv, torch), track) for (ref, track), form, lv in zip(dc.track_problems(), dc.TRACK_FORMS, dc.TRACK_LEVELS)]


def test_null_sync_on_tiny_tracks_in_slice_and_byte_forms():
    """Tracks of one to nine cues against references of 3000, 2464, 2465 and 2495 samples (n % 32 = 24, 0, 1, 31) as
    misaligned slices with ones behind the last sample and as bytes, every other one with the low level 0.1."""
    import torch
    from ffsubsync_amd import surrogate

    got = surrogate.null_sync(_track_problems(torch), rc.TRACK_SECONDS, n_surrogates=rc.TRACK_K, block_units=1, seed=rc.TRACK_SEED,
                              min_z=rc.TRACK_MIN_Z)
    for j, r in enumerate(got):
        _check_null_result(r, dc.track_null_model(j), j)
    assert len(got) == len(dc.TRACK_FORMS) == 8


def test_stable_sync_on_tiny_tracks_in_slice_and_byte_forms():
    import torch
    from ffsubsync_amd import stability

    got = stability.stable_sync(_track_problems(torch), rc.TRACK_SECONDS, n_subsamples=rc.TRACK_K, block_runs=1, seed=rc.TRACK_SEED,
                                tol=rc.TRACK_TOL, min_share=rc.TRACK_MIN_SHARE)
    for j, r in enumerate(got):
        _check_stable_result(r, dc.track_stable_model(j), j)
    assert len(got) == len(dc.TRACK_FORMS) == 8


def test_tiny_files_whose_reference_lists_come_from_slice_and_byte_rasters():
    """The seven tiny files of tests/resample_edge_cases.py through ``null_test_lists`` and ``stability_test_lists`` with
    the reference lists extracted on the device from rasters in the slice and byte forms, and the levels taken from the
    rasters: every score, offset and flag of both tables and every record against the models."""
    import torch
    from ffsubsync_amd import _native, stability, surrogate

    keep, rows = [], []
    for i, (ref_len, ref_lv, _, sub_len, sub_lv, seed, _) in enumerate(rc.TINY_FILES):
        ref, pos, _ = rc.tiny_file(i)
        raster = dc.build(dc.TINY_FORMS[i], ref, ref_lv, torch)
        n_ref = sm.boundaries(ref).size
        ref_block = _native.runs_from_bits(raster.packed_words(), len(raster), cap=n_ref + 2)
        sub_block = torch.from_numpy(sm.encode(pos, sub_len, pos.size + 1)).cuda()
        keep.append((raster, ref_block, sub_block))
        rows.append((ref_block.data_ptr(), len(raster), n_ref, sub_block.data_ptr(), sub_len, pos.size, raster.lo, raster.hi,
                     sub_lv[0], sub_lv[1], seed))
    rp, rl, rb, sp, sl, sb, rlo, rhi, slo, shi, seeds = [np.array(c) for c in zip(*rows)]
    assert list(rl) == [f[0] for f in rc.TINY_FILES]
    block, k = dc.TINY_BLOCK, dc.TINY_K
    null = surrogate.null_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, rc.TINY_W, k, block, ref_lo=rlo,
                                     ref_hi=rhi, sub_lo=slo, sub_hi=shi, seeds=seeds)
    assert not null.status.any() and null.stats["careful_files"] == 0
    tre._check_null_table(null.solves(), null.records, block, k)
    half = stability.stability_test_lists(rp.astype(np.uint64), rl, rb, sp.astype(np.uint64), sl, sb, rc.TINY_W, k, block,
                                          tol=rc.TINY_TOL, ref_lo=rlo, ref_hi=rhi, sub_lo=slo, sub_hi=shi, seeds=seeds)
    assert not half.status.any() and half.stats["careful_files"] == 0
    tre._check_half_table(half.solves(), half.records, block, k)
    assert len(keep) == len(rc.TINY_FILES) == len(dc.TINY_FORMS)


# ---- 6. a silent device reference --------------------------------------------------------------------------------------------
def test_a_silent_device_reference_through_all_four_entries():
    """An all-zero raster with explicit levels (0, 1): every entry gives what its model gives for the all-zero host vector.
    (Should a solve raise FFS_FLAG_AMBIGUOUS, the file is redone by ``ratio_sweep._careful`` on a ``_Vec`` that holds the
    raster; the answers are the same either way.)"""
    import torch
    from ffsubsync_amd import ratio_sweep, stability, surrogate
    from ffsubsync_amd.batch_gss import fit_gss_batch

    zeros, track = np.zeros(dc.silent_reference().size), dc.small_track()
    silent = lambda: dc.build("packed", dc.silent_reference(), dc.SILENT_LEVELS, torch)
    lo, hi = dc.DENSE_RANGE
    seen = 0
    prof = ratio_sweep.ratio_profile_batch([(silent(), track)], dc.SMALL_SECONDS, lo=lo, hi=hi, tolerance_samples=dc.DENSE_TOLERANCE)
    grid = dc.small_grid(lo, hi, dc.DENSE_TOLERANCE)
    rec = prof.records()[0]
    assert np.array_equal(prof.grids[0], grid) and not (rec["flags"] & 1).any()
    assert _pairs(rec) == [(o, s) for o, s, _ in dc.exact_records("silent", dc.SILENT_LEVELS, tuple(grid.tolist()))]
    seen += 1
    got = ratio_sweep.sweep_sync([(silent(), track)], dc.SMALL_SECONDS, lo=lo, hi=hi, tolerance_samples=dc.DENSE_TOLERANCE, top_k=1)
    want = sweep_model.sweep(zeros, track, dc.SMALL_W, lo=lo, hi=hi, tolerance_samples=dc.DENSE_TOLERANCE, top_k=1)
    _check_sweep_result(got[0], want, "silent")
    seen += 1
    null = surrogate.null_sync([(silent(), track)], dc.SMALL_SECONDS, n_surrogates=dc.PCM_K, block_units=1, seed=dc.PCM_SEED, min_z=rc.TRACK_MIN_Z)
    _check_null_result(null[0], sm.null_sync(zeros, track, dc.SMALL_W, None, dc.PCM_K, 1, dc.PCM_SEED, 0, rc.TRACK_MIN_Z), "silent")
    seen += 1
    stable = stability.stable_sync([(silent(), track)], dc.SMALL_SECONDS, n_subsamples=dc.PCM_K, block_runs=1, seed=dc.PCM_SEED,
                                   tol=rc.TRACK_TOL, min_share=rc.TRACK_MIN_SHARE)
    _check_stable_result(stable[0], stm.stable_sync(zeros, track, dc.SMALL_W, None, dc.PCM_K, 1, dc.PCM_SEED, 0, rc.TRACK_TOL,
                                                    rc.TRACK_MIN_SHARE), "silent")
    seen += 1
    gss = fit_gss_batch([silent()], [track], max_offset_samples=dc.SMALL_W)
    _check_gss(gss, [zeros], [track], [dc.SILENT_LEVELS], dc.SMALL_W)
    seen += 1
    assert seen == 5  # the four entries, ratio_profile_batch and sweep_sync counted apart


# ---- 7. PCM to answer --------------------------------------------------------------------------------------------------------
def _pcm_rasters(torch, pcm_dev, detector):
    """The packed raster of device-resident PCM: the adaptive detector, or the fixed 50 dB rule (``ffs_vad_energy_bits``,
    what ``detect_pinned_stream(packed=True)`` wraps the same way)."""
    from ffsubsync_amd import _native, adaptive_vad
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    fl = 160
    if detector == "adaptive":
        raster, rec = adaptive_vad.detect_device_adaptive(pcm_dev, 100, 100 * fl, dc.PCM_LABEL, packed=True)
        assert not rec.flags
        return raster
    words, n = _native.vad_energy_bits(pcm_dev, fl, 50.0)
    return DeviceRaster(words, dc.PCM_LABEL, 1.0, n)


def _pcm_answers(raster):
    """The raster straight into the four syncs; nothing of it is looked at on the host in between."""
    from ffsubsync_amd import quality, ratio_sweep, stability, surrogate

    track = dc.pcm_track()
    lo, hi = dc.pcm_sweep_range()
    return dict(
        quality=quality.quality_sync([(raster, track)], dc.SMALL_SECONDS)[0],
        sweep=ratio_sweep.sweep_sync([(raster, track)], dc.SMALL_SECONDS, lo=lo, hi=hi, **dc.PCM_SWEEP)[0],
        null=surrogate.null_sync([(raster, track)], dc.SMALL_SECONDS, n_surrogates=dc.PCM_K, block_units=1, seed=dc.PCM_SEED,
                                 min_z=rc.TRACK_MIN_Z)[0],
        stable=stability.stable_sync([(raster, track)], dc.SMALL_SECONDS, n_subsamples=dc.PCM_K, block_runs=1, seed=dc.PCM_SEED,
                                     tol=rc.TRACK_TOL, min_share=rc.TRACK_MIN_SHARE)[0])


def _check_pcm_answers(got, silent, where):
    from oracle import raster_oracle as ro

    m = dc.pcm_models(silent)
    q, best = got["quality"], m["best"]
    assert (q.ratio, q.ratio_index, q.offset, q.score) == (float(sweep_model.SEVEN[best]), best) + m["seven"][best], (where, q)
    tr = dc.pcm_track()
    v = np.zeros(dc.pcm_speech().size, bool) if silent else dc.pcm_speech()
    pr = dict(rb=v, sb=ro.rasterize(tr[0], tr[1], tr[2], q.ratio, 100, 0) != 0, r_lv=dc.PCM_LEVELS,
              s_lv=(0.0, min(1.0 / q.ratio, 1.0)), w=dc.SMALL_W, top_k=3, e=300)
    assert tgq._compare(q.quality, pr) is None, (where, tgq._compare(q.quality, pr))
    _check_sweep_result(got["sweep"], m["sweep"], where)
    _check_null_result(got["null"], m["null"], where)
    _check_stable_result(got["stable"], m["stable"], where)


def test_pcm_to_answer_with_nothing_on_the_host_in_between():
    """The three gain files (3 000 frames of 160 samples) through the adaptive detector with non_speech_label 0.1: the
    packed raster goes straight into ``quality_sync``, ``sweep_sync``, ``null_sync`` and ``stable_sync`` and the answers
    are the models' on np.where(model speech, 1.0, 0.1), the same at every gain; the loud file under the fixed rule gives
    the same raster and answers, the quiet one a silent raster and the silent reference's answers; so do the rasters of
    ``detect_pinned_stream_adaptive`` and ``detect_pinned_stream`` (``packed=True``) from pinned host memory."""
    import torch
    import adaptive_vad_model as am

    fl, files = am.gain_files()
    seen = 0
    for gain in dc.PCM_GAINS:
        got = _pcm_answers(_pcm_rasters(torch, torch.from_numpy(files[gain]).cuda(), "adaptive"))
        _check_pcm_answers(got, False, ("adaptive", gain))
        seen += 1
    _check_pcm_answers(_pcm_answers(_pcm_rasters(torch, torch.from_numpy(files[0]).cuda(), "fixed")), False, ("fixed", 0))
    # the same two detectors behind the double-buffered copy loop, from pinned host memory
    from ffsubsync_amd import adaptive_vad, speech_transformers

    pinned = torch.from_numpy(files[-12]).pin_memory()
    raster, rec = adaptive_vad.detect_pinned_stream_adaptive(pinned, 100, 100 * fl, dc.PCM_LABEL, packed=True)
    assert not rec.flags and raster.packed and (raster.lo, raster.hi, len(raster)) == (dc.PCM_LABEL, 1.0, dc.pcm_speech().size)
    _check_pcm_answers(_pcm_answers(raster), False, ("adaptive, pinned", -12))
    raster = speech_transformers.detect_pinned_stream(torch.from_numpy(files[0]).pin_memory(), 100, 100 * fl, dc.PCM_LABEL, packed=True)
    _check_pcm_answers(_pcm_answers(raster), False, ("fixed, pinned", 0))
    seen += 2
    _check_pcm_answers(_pcm_answers(_pcm_rasters(torch, torch.from_numpy(files[-30]).cuda(), "fixed")), True, ("fixed", -30))
    assert seen + 2 == len(dc.PCM_GAINS) + 4 == 7


def test_pcm_to_answer_on_a_side_stream_with_a_late_upload():
    """The same leg inside ``torch.cuda.stream(side)``: the PCM comes from pinned memory by a non-blocking copy and the
    VAD launches and the sync calls are queued behind it with no synchronisation of the test's in between."""
    import torch
    import adaptive_vad_model as am

    fl, files = am.gain_files()
    pinned = {g: torch.from_numpy(files[g]).pin_memory() for g in (0, -12)}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = []
    with torch.cuda.stream(side):
        for g, detector in ((-12, "adaptive"), (0, "fixed")):
            pcm = torch.empty(pinned[g].numel(), dtype=torch.int16, device="cuda")
            pcm.copy_(pinned[g], non_blocking=True)
            got.append(((detector, g), _pcm_answers(_pcm_rasters(torch, pcm, detector))))
    side.synchronize()
    for where, answers in got:
        _check_pcm_answers(answers, False, where)
    assert len(got) == 2
