"""Ratio sweep on the device: ``ffs_sweep_peaks`` against tests/sweep_model.py on record tables uploaded
directly, the ratio profile against the oracle, ``sweep_sync`` end to end against the model, the bit-raster fallback and
sub-batching."""
import math

import numpy as np
import pytest

import sweep_cases as cases
import sweep_model as sm

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025]


def _tables():
    """One record table per file: the sizes around the wave and workgroup widths with random, tie-rich scores, then the
    planted cases."""
    from ffsubsync_amd import _native

    rng = np.random.RandomState(7)
    files = []
    for g in SIZES:
        rec = np.zeros(g, _native.CAND_RESULT_DTYPE)
        rec["score"] = rng.randint(0, 40, g) * 0.37 - 2.0
        rec["offset"] = rng.randint(-6000, 6001, g)
        skip = rng.rand(g)
        rec["score"][skip < 0.05] = -np.inf
        rec["flags"][(skip >= 0.05) & (skip < 0.1)] |= _native.FLAG_EMPTY_WINDOW
        rec["flags"][rng.rand(g) < 0.3] |= _native.FLAG_DIRECT  # a flag the reduction ignores
        files.append(rec)

    def blank(g, value=1.0):
        rec = np.zeros(g, _native.CAND_RESULT_DTYPE)
        rec["score"] = value + 1e-3 * rng.rand(g)
        rec["offset"] = np.arange(g) - 17
        return rec

    waves = blank(600)  # equal maxima held by waves 0, 1, 3 and by wave 0's third trip: the smallest index wins
    waves["score"][[300, 200, 100, 10, 522]] = 9.0
    files.append(waves)
    gone = blank(300)  # a -inf point and an EMPTY_WINDOW point where the maximum would be
    gone["score"][[70, 140, 210]] = [np.inf, 50.0, 7.0]
    gone["score"][5] = -np.inf
    gone["flags"][140] |= _native.FLAG_EMPTY_WINDOW
    gone["score"][250] = np.nan
    files.append(gone)
    files.append(np.array([(0.1, j, 0.0, 0) for j in range(257)], _native.CAND_RESULT_DTYPE))  # all equal
    amb = blank(65)
    amb["flags"][64] |= _native.FLAG_AMBIGUOUS
    files.append(amb)
    none_left = blank(3)  # every point skipped, one of them ambiguous
    none_left["score"][:] = -np.inf
    none_left["flags"][1] |= _native.FLAG_AMBIGUOUS
    files.append(none_left)
    return files


def _upload(files):
    import torch

    first = np.zeros(len(files) + 1, np.int64)
    np.cumsum([f.size for f in files], out=first[1:])
    host = np.concatenate(files) if first[-1] else np.zeros(0, files[0].dtype)
    table = torch.from_numpy(np.concatenate([host, np.zeros(1, host.dtype)]).view(np.uint8).copy()).cuda()
    return table, first


@pytest.mark.parametrize("top_k", [1, 8])
@pytest.mark.parametrize("exclusion", [1, 4, 2000])
def test_sweep_peaks_equal_the_model(top_k, exclusion):
    from ffsubsync_amd import _native, ratio_sweep

    files = _tables()
    table, first = _upload(files)
    before = table.clone()
    got = ratio_sweep.sweep_peaks(table, first, top_k, exclusion)
    assert got.shape == (len(files),)
    assert bool((table == before).all())  # records are read, never written
    for f, (rec, g) in enumerate(zip(files, got)):
        want = sm.report(rec["score"], rec["offset"], rec["flags"], top_k, exclusion)
        n = len(want["peaks"])
        assert int(g["n_peaks"]) == n, f
        # peaks bit for bit; entries beyond the count are zero
        assert g["peak_score"][:n].tobytes() == np.array([p[0] for p in want["peaks"]], np.float64).tobytes(), f
        assert list(g["peak_offset"][:n]) == [p[1] for p in want["peaks"]] and list(g["peak_index"][:n]) == [p[2] for p in want["peaks"]], f
        assert not g["peak_score"][n:].any() and not g["peak_offset"][n:].any() and not g["peak_index"][n:].any()
        assert (int(g["n_points"]), int(g["n_skipped"]), int(g["flags"])) == (rec.size, want["n_skipped"], want["flags"]), f
        assert float(g["mean"]) == pytest.approx(want["mean"], rel=1e-9, abs=0) and float(g["std"]) == pytest.approx(want["std"], rel=1e-9, abs=0), f
        if want["flags"] & sm.FLAT:
            assert float(g["std"]) == 0.0 and float(g["mean"]) == want["mean"]
    planted = len(SIZES)
    if exclusion == 1 and top_k == 8:
        assert list(got[planted]["peak_index"][:5]) == [10, 100, 200, 300, 522]
    assert int(got[planted + 1]["peak_index"][0]) == 210 and float(got[planted + 1]["peak_score"][0]) == 7.0
    assert int(got[planted + 1]["n_skipped"]) == 4
    assert int(got[planted + 2]["flags"]) == _native.SWEEP_FLAT and float(got[planted + 2]["mean"]) == 0.1
    assert int(got[planted + 3]["flags"]) == _native.SWEEP_AMBIGUOUS
    assert int(got[planted + 4]["flags"]) == _native.SWEEP_FLAT | _native.SWEEP_EMPTY | _native.SWEEP_AMBIGUOUS


def test_sweep_peaks_refusals_leave_the_outputs_untouched():
    import torch

    from ffsubsync_amd import _native, ratio_sweep

    files = _tables()[:4]
    table, first = _upload(files)
    first_dev = torch.from_numpy(first).cuda()
    out = torch.full((len(files) * _native.SWEEP_PROFILE_BYTES + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    lib = _native.load()
    stream = _native.current_stream_ptr(torch)

    def call(rec=table.data_ptr(), fst=first_dev.data_ptr(), n=len(files), top_k=3, excl=1, dst=out.data_ptr()):
        return lib.ffs_sweep_peaks(rec, fst, n, top_k, excl, dst, stream)

    for kwargs, word in [(dict(top_k=0), b"top_k"), (dict(top_k=9), b"top_k"), (dict(excl=0), b"exclusion_steps"),
                         (dict(excl=-5), b"exclusion_steps"), (dict(n=-1), b"n_files"), (dict(rec=None), b"null"),
                         (dict(fst=None), b"null"), (dict(dst=None), b"null"), (dict(rec=table.data_ptr() + 4), b"misaligned"),
                         (dict(fst=first_dev.data_ptr() + 4), b"misaligned"), (dict(dst=out.data_ptr() + 4), b"misaligned")]:
        assert call(**kwargs) == -1 and word in lib.ffs_last_error(), kwargs
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all()), kwargs
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert call() == 0  # only n_files records are written
    torch.cuda.synchronize()
    assert bool((out[len(files) * _native.SWEEP_PROFILE_BYTES:] == 0xAB).all())
    want = ratio_sweep.sweep_peaks(table, first, 3, 1)
    assert out[:len(files) * _native.SWEEP_PROFILE_BYTES].cpu().numpy().tobytes() == want.tobytes()
    for bad in (dict(top_k=0), dict(top_k=9), dict(top_k=1.5), dict(exclusion_steps=0)):
        with pytest.raises(ValueError):
            ratio_sweep.sweep_peaks(table, first, **bad)
    with pytest.raises(ValueError):
        ratio_sweep.sweep_peaks(table, first[::-1].copy())
    with pytest.raises(ValueError):
        ratio_sweep.sweep_peaks(table, first + 2)  # more records than the table holds


def _assert_records_equal_oracle(rec, reference, track, grid):
    """Every record against the oracle: the score within 1e-9 relative, the offset equal.  Where several lags score
    within that 1e-9 of the maximum (integer scores at ratios below 1 tie exactly and often; a flickering reference
    repeats its score every other lag) the oracle's argmax is decided by its FFT's rounding.  There, and only there, the
    exact reference (tests/exact_reference.py) arbitrates: the record must be its record, and the exact score at the
    oracle's lag must be within 1e-9 relative of the maximum, i.e. a lag the oracle cannot tell from it."""
    import exact_reference as xr
    from oracle import raster_oracle as ro

    sc, off, _ = sm.evaluate(reference, track, grid, cases.W)
    assert np.allclose(rec["score"], sc, rtol=1e-9, atol=0)
    assert not (rec["flags"] & 3).any()
    for i in np.flatnonzero(rec["offset"] != off):
        r = float(grid[i])
        sub = ro.rasterize(track[0], track[1], track[2], r, 100, 0)
        levels = ((0.0, 1.0), (0.0, min(1.0 / r, 1.0)))
        exact = xr.candidate(reference != 0, sub != 0, levels[0], levels[1], cases.W)
        assert (exact["offset"], exact["score"]) == (int(rec["offset"][i]), float(rec["score"][i])), (i, r, exact)
        at_oracle = xr.score_at(reference != 0, sub != 0, levels[0], levels[1], int(off[i]))
        assert abs(at_oracle - exact["score"]) <= 1e-9 * abs(exact["score"]), (i, r, exact, int(off[i]), at_oracle)


def _assert_profile_equals_oracle(prof, problems):
    recs = prof.records()
    assert len(recs) == len(problems)
    for p, grid, rec in zip(problems, prof.grids, recs):
        _assert_records_equal_oracle(rec, p.reference, p.track, grid)


def test_profile_equals_the_oracle_at_every_ratio():
    from ffsubsync_amd import ratio_sweep

    problems = [cases.problem("free", 5, 300.0), cases.problem("free", 2, 300.0)]  # true ratios 1.0326 and 0.9498
    assert problems[0].true_ratio > 1 > problems[1].true_ratio
    prof = ratio_sweep.ratio_profile_batch([p.problem for p in problems])
    for p, grid in zip(problems, prof.grids):
        want, _ = sm.grid(sm.duration_samples(p.track), 0.9, 1.1, ratio_sweep.DEFAULT_TOLERANCE)
        assert np.array_equal(grid, want) and 30 <= grid.size <= 70
    assert prof.stats["lists"] and list(prof.first) == [0, prof.grids[0].size, prof.grids[0].size + prof.grids[1].size]
    _assert_profile_equals_oracle(prof, problems)
    # the grid maximum is the point nearest the truth, and the device peaks say so
    peaks = ratio_sweep.sweep_peaks(prof.table, prof.first_dev)
    for p, grid, pk in zip(problems, prof.grids, peaks):
        assert int(pk["peak_index"][0]) == int(np.argmin(np.abs(grid - p.true_ratio)))


def test_sweep_sync_finds_unknown_ratios_and_equals_the_model():
    from ffsubsync_amd import quality, ratio_sweep

    found = [("free", s) for s in cases.FREE_SEEDS + (cases.EXTRA_FREE_SEED,)] + [("seven", cases.SEVEN_SEED)]
    problems = [cases.problem(k, s) for k, s in found]
    results = ratio_sweep.sweep_sync([p.problem for p in problems] + [cases.problem("wrong", cases.WRONG_SEED).problem])
    for (kind, seed), p, r in zip(found, problems, results):
        want = cases.model_sweep(kind, seed)
        assert abs(r.ratio - p.true_ratio) <= want["step"] / 16 * (1 + 1e-9), (kind, seed, r.ratio)
        assert r.reasons == [], (kind, seed, r.reasons)
        assert (repr(r.ratio), r.offset, repr(r.coarse_ratio)) == (repr(want["ratio"]), want["offset"], repr(want["coarse_ratio"]))
        assert r.score == pytest.approx(want["score"], rel=1e-9)
        psr, margin = sm.psr_margin(want["report"])
        assert r.profile.psr == pytest.approx(psr, rel=1e-6) and r.profile.margin == pytest.approx(margin, rel=1e-6)
        assert [pk[1] for pk in r.profile.peaks] == [pk[1] for pk in want["report"]["peaks"]]
        # the found ratio feeds the existing aligners unchanged
        q = quality.quality_sync([p.problem], ratios=[r.ratio])[0]
        assert (q.offset, q.score) == (r.offset, r.score)
    assert results[-1].reasons, results[-1]
    assert abs(results[4].ratio - 0.96) <= 1e-12  # the seven ratios are evaluated exactly


def test_dense_reference_takes_the_bit_rasters():
    from ffsubsync_amd import ratio_sweep

    p = cases.problem("free", 1)
    dense = np.maximum(p.reference, (np.arange(p.reference.size) % 2).astype(np.float64))
    assert np.count_nonzero(np.diff(dense)) >= 32768  # more boundaries than a reference list holds
    prof = ratio_sweep.ratio_profile_batch([(dense, p.track)], lo=0.96, hi=1.01)
    assert prof.stats["lists"] is False and 15 <= prof.grids[0].size <= 40
    _assert_records_equal_oracle(prof.records()[0], dense, p.track, prof.grids[0])


def test_three_sub_batches_give_the_same_table():
    from ffsubsync_amd import ratio_sweep

    problems = [cases.problem("free", 5, 300.0).problem, cases.problem("free", 2, 300.0).problem]
    whole = ratio_sweep.ratio_profile_batch(problems)
    total = int(whole.first[-1])
    assert whole.stats["chunks"] == 1 and whole.stats["chunk_vectors"] == total
    budget = whole.stats["vector_bytes"] * int(math.ceil(total / 3))
    parts = ratio_sweep.ratio_profile_batch(problems, budget_bytes=budget)
    assert parts.stats["chunks"] == 3
    assert parts.table[:total * 24].cpu().numpy().tobytes() == whole.table[:total * 24].cpu().numpy().tobytes()
    assert ratio_sweep.sweep_peaks(parts.table, parts.first).tobytes() == ratio_sweep.sweep_peaks(whole.table, whole.first_dev).tobytes()


def test_ambiguous_file_is_redone_on_the_careful_path(monkeypatch):
    """FFS_FLAG_AMBIGUOUS planted on the batch records of file 0 (no input in reach makes the list path raise it): that
    file alone is redone through the drop-in's ``solve_pairs``, which gives the batch's own scores and offsets; its
    neighbour keeps the batch's records byte for byte."""
    import torch

    from ffsubsync_amd import _native, ratio_sweep
    from ffsubsync_amd.batch_gss import PreparedRatioSolve

    problems = [cases.problem("free", 5, 300.0).problem, cases.problem("free", 2, 300.0).problem]
    plain = ratio_sweep.ratio_profile_batch(problems, lo=1.02, hi=1.05)
    assert "careful_files" not in plain.stats and 5 <= plain.grids[0].size <= 8
    solve = PreparedRatioSolve.evaluate

    def planted(self, which, ratios, cand_out):
        solve(self, which, ratios, cand_out)
        m = len(which)
        flags = cand_out[:m * 24].view(torch.int32).reshape(m, 6)[:, 5]
        flags[torch.from_numpy(np.asarray(which) == 0).cuda()] |= _native.FLAG_AMBIGUOUS
        return cand_out

    monkeypatch.setattr(PreparedRatioSolve, "evaluate", planted)
    redone = ratio_sweep.ratio_profile_batch(problems, lo=1.02, hi=1.05)
    assert redone.stats["careful_files"] == 1
    got, want = redone.records(), plain.records()
    assert got[0]["score"].tobytes() == want[0]["score"].tobytes() and list(got[0]["offset"]) == list(want[0]["offset"])
    assert not (got[0]["flags"] & _native.FLAG_AMBIGUOUS).any()
    assert got[1].tobytes() == want[1].tobytes()


def test_refused_problems():
    from ffsubsync_amd import ratio_sweep

    p = cases.problem("free", 5, 300.0)
    levels = p.reference.copy()
    levels[::3] *= 0.4  # three levels
    with pytest.raises(ValueError, match="multi-level float reference"):
        ratio_sweep.ratio_profile_batch([(levels, p.track)])
    assert ratio_sweep.sweep_sync([]) == []
