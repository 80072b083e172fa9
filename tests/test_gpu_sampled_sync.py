"""sampled_sync end to end on the device: seeds 0-7 at 10 min, ten 60 s segments in the spread order, seven
ratios.  The stop update and the answer equal tests/sampled_model.py's run exactly (tests/test_sampled_model_host.py asserts
that no decision statistic of these seeds lies within 1e-6 of a threshold, so the moments' rounding cannot move a
decision)."""
import numpy as np
import pytest

import progressive_cases as pc
import sampled_cases as sc
import sampled_model as sm

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float64(x).view(np.int64)


class Reader:
    """A file's ``read_segment``; raises when called after ``close()`` (sampled_sync closes a settled file)."""

    def __init__(self, ref, rate=100):
        self.ref, self.rate, self.closed, self.calls = ref, rate, False, []

    def __call__(self, start_seconds, seconds):
        assert not self.closed, "read after its file settled"
        a, n = int(round(start_seconds * self.rate)), int(round(seconds * self.rate))
        self.calls.append((a, a + n))
        return self.ref[a:a + n].astype(np.uint8)

    def close(self):
        self.closed = True


def _rule(index):
    from ffsubsync_amd.progressive import StopRule

    r = sc.SYNC_RULES[index]
    return StopRule(r["min_psr"], r["min_margin"], r["min_ratio_margin"], r["stable_updates"], r["offset_tolerance"], 0.0)


@pytest.mark.parametrize("rule_index", [0, 1])
def test_stop_update_and_answer_equal_the_model(rule_index):
    from ffsubsync_amd import sampled

    probs = [pc.sync_problem(s) for s in sc.SYNC_SEEDS]
    readers = [Reader(p[0]) for p in probs]
    res = sampled.sampled_sync([(rd, p[1], p[0].size / 100) for rd, p in zip(readers, probs)], _rule(rule_index),
                               segment_seconds=60, max_offset_seconds=60, top_k=sc.SYNC_TOP_K, exclusion_samples=sc.SYNC_E)
    settled = 0
    for seed, r, rd in zip(sc.SYNC_SEEDS, res, readers):
        want = sc.sync_model_run(seed, rule_index)
        st = want["state"]
        assert (r.updates, r.settled, r.consumed_samples) == (want["updates"], want["settled"], st["ref_len"]), seed
        assert (r.ratio_index, r.offset) == (st["best_cand"], st["offset"]) and _bits(r.score) == _bits(st["score"]), seed
        assert r.ratio == probs[seed][3][r.ratio_index]
        assert rd.calls == sm.segment_schedule(60000, sc.SYNC_SEGMENT)[:r.updates]  # the spread order, nothing after the stop
        assert rd.closed == r.settled  # the close() hook, on settling only
        assert r.reasons == [] if r.settled else True
        settled += r.settled
    if rule_index == 0:
        assert settled >= 4  # (the test is about stopping)


def test_a_file_that_never_settles_has_read_everything_and_equals_quality_sync():
    from ffsubsync_amd import quality, sampled

    probs = [pc.sync_problem(s) for s in sc.SYNC_SEEDS[:4]]
    readers = [Reader(p[0]) for p in probs]
    from ffsubsync_amd.progressive import StopRule

    res = sampled.sampled_sync([(rd, p[1], 600.0) for rd, p in zip(readers, probs)], StopRule(stable_updates=None))
    want = quality.quality_sync([(p[0].astype(float), p[1]) for p in probs])
    for r, q, rd in zip(res, want, readers):
        assert not r.settled and r.updates == 10 and r.consumed_samples == 60000 and not rd.closed
        assert sorted(rd.calls) == [(6000 * k, 6000 * k + 6000) for k in range(10)]
        assert (r.ratio_index, r.ratio, r.offset) == (q.ratio_index, q.ratio, q.offset) and _bits(r.score) == _bits(q.score)
        assert r.quality == q.quality and r.reasons == q.reasons
    # the prefix order ends on the same records
    again = sampled.sampled_sync([(Reader(p[0]), p[1], 600.0) for p in probs], StopRule(stable_updates=None),
                                 order=sampled.prefix_schedule)
    assert [(r.ratio_index, r.offset, _bits(r.score), r.quality) for r in again] == \
        [(r.ratio_index, r.offset, _bits(r.score), r.quality) for r in res]


def test_known_reference_and_the_forms_of_chunks_agree():
    import torch

    from ffsubsync_amd import _native, sampled

    ref, track, _, _ = pc.sync_problem(0)
    appends = [(5000, 0), (6000, 1), (100, 31), (1000, 4000), (131, 33), (0, 100)]
    with sampled.SampledSolve([track, track, track], [70.0, 70.0, 70.0]) as solve:
        assert solve.known(1) == [] and solve.reference(1).n == 7000
        for i, (a, n) in enumerate(appends):
            chunk = ref[a:a + n]
            flat = np.ones(32 * ((8 + n + 31) // 32 + 1), bool)
            flat[8:8 + n] = chunk
            words = torch.from_numpy(np.packbits(flat, bitorder="little").view(np.int32).copy()).cuda()
            labels = torch.from_numpy(np.where(chunk, 1.0, 0.25).astype(np.float32)).cuda()
            got = solve.append_at({2: (a, chunk.astype(bool) if i % 2 else chunk.astype(np.float64)), 0: (a, (words, 8, n)),
                                   1: (a, labels)})
            assert solve.last_records[0].tobytes() == solve.last_records[1].tobytes() == solve.last_records[2].tobytes()
            assert got[0] == got[1] == got[2] and got[0].ref_len == sum(k for _, k in appends[:i + 1])
        want = sm.merge([(a, a + n) for a, n in appends])
        mask = np.zeros(7000, bool)
        for a, b in want:
            mask[a:b] = True
        for f in range(3):
            assert solve.known(f) == want == [(0, 164), (1000, 5000), (6000, 6001)]
            r = solve.reference(f)
            assert r.n == 7000 and (r.lo, r.hi) == (0.0, 1.0)
            assert (_native.unpack_bits(r.bits, r.n).cpu().numpy() != 0).tolist() == (ref[:7000] & mask).tolist()
        with pytest.raises(ValueError, match="overlaps"):
            solve.append_at({0: (4999, np.zeros(3, np.uint8))})
        with pytest.raises(ValueError, match="outside the reference"):
            solve.append_at({0: (6999, np.zeros(2, np.uint8))})
    with pytest.raises(ValueError, match="closed"):
        solve.append_at({0: (0, np.zeros(3, np.uint8))})


def test_pcm_segments_go_through_the_energy_detector():
    import torch

    from ffsubsync_amd import _native, sampled
    from ffsubsync_amd.progressive import StopRule

    _, track, _, _ = pc.sync_problem(1)
    n = 480 * 6000  # 60 s at 48 kHz: 6000 frames of 10 ms
    pcm = ((np.arange(n) % 977 - 488) * ((np.arange(n) // 48000) % 3) * 20).astype(np.int16)  # loud, quiet and silent seconds
    seen = []

    def read_pcm(start_seconds, seconds):
        a, k = int(round(start_seconds * 48000)), int(round(seconds * 48000))
        seen.append((start_seconds, seconds))
        return pcm[a:a + k]

    def read_labels(start_seconds, seconds):
        a, k = int(round(start_seconds * 48000)), int(round(seconds * 48000))
        words, frames = _native.vad_energy_bits(torch.from_numpy(pcm[a:a + k]).cuda(), 480, 0.0)
        return words, 0, frames

    never = StopRule(stable_updates=None)
    got = sampled.sampled_sync([(read_pcm, track, 60.0)], never, segment_seconds=20, energy_threshold_db=0.0)
    want = sampled.sampled_sync([(read_labels, track, 60.0)], never, segment_seconds=20)
    assert seen == [(0.0, 20.0), (20.0, 20.0), (40.0, 20.0)]
    assert got == want and got[0].consumed_samples == 6000 and got[0].updates == 3
    # a short read is refused before the round's native call: labels one short, PCM one frame short
    for short in (lambda start, seconds: np.zeros(int(round(seconds * 100)) - 1, np.uint8),
                  lambda start, seconds: read_pcm(start, seconds)[:-480]):
        with pytest.raises(ValueError, match="returned 1999 samples, the segment has 2000"):
            sampled.sampled_sync([(short, track, 60.0)], never, segment_seconds=20, energy_threshold_db=0.0)


def test_the_one_shot_path_on_the_half_filled_vector_scores_what_the_plan_scores():
    """assemble_sparse_reference(unknown=0.5) through the main solve against SampledSolve on the same windows; and the
    default (zeros) is unchanged, as is the error when no window holds speech."""
    import torch

    from ffsubsync_amd import aligners, sampled
    from ffsubsync_amd.speech_transformers import assemble_sparse_reference

    ref, track, cands, ratios = pc.sync_problem(2)
    windows = [(0, 6000), (24000, 6000), (48000, 6000)]
    labels = [torch.from_numpy(ref[a:a + n].astype(np.float32)).cuda() for a, n in windows]
    starts = [a / 100 for a, _ in windows]
    zeros = assemble_sparse_reference(labels, starts, 600.0, 100).cpu().numpy()
    half = assemble_sparse_reference(labels, starts, 600.0, 100, unknown=0.5).cpu().numpy()
    mask = np.zeros(60002, bool)
    for a, n in windows:
        mask[a:a + n] = True
    assert zeros.size == half.size == 60002 and (zeros[mask] == half[mask]).all() and (zeros[mask] == ref[mask[:60000].nonzero()[0]]).all()
    assert (zeros[~mask] == 0).all() and (half[~mask] == 0.5).all()
    silent = [torch.zeros(100, device="cuda")]
    for kw in ({}, dict(unknown=0.5)):
        with pytest.raises(ValueError, match="Unable to detect speech in any sampled segment"):
            assemble_sparse_reference(silent, [3], 60.0, 100, **kw)
    with pytest.raises(ValueError, match="unknown"):
        assemble_sparse_reference(labels, starts, 600.0, 100, unknown=float("nan"))
    model = sm.Slot(cands, (0.0, 1.0), 6000, 60002)
    for a, n in windows:
        model.append_at(a, ref[a:a + n], sc.SYNC_TOP_K, sc.SYNC_E)
    gap, decision = sm.decision_gap(model)
    assert gap > 0.5  # no rounding of the transforms can move the winner
    with sampled.SampledSolve([track], [600.025], top_k=sc.SYNC_TOP_K, exclusion_samples=sc.SYNC_E) as solve:
        for a, n in windows:
            st = solve.append_at({0: (a, ref[a:a + n])})[0]
    cres, pres = aligners.solve_host_batch([(half.astype(np.float64), [np.where(s, lv[1], lv[0]) for s, lv in cands])], 6000, 6000)
    assert (int(pres[0]["best_cand"]), int(pres[0]["offset"])) == (st.best_cand, st.offset) == decision
    assert abs(float(pres[0]["score"]) - st.score) <= model.slack(decision[0])  # scores_from_counts' slack
