"""progressive_sync end to end on the device: seeds 0-7 at 10 min, six chunks, seven ratios.  The stop
update and the answer equal tests/progressive_model.py's run exactly (tests/test_progressive_model_host.py asserts that no
decision statistic of these seeds lies within 1e-6 of a threshold, so the moments' rounding cannot move a decision)."""
import numpy as np
import pytest

import progressive_cases as pc

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float64(x).view(np.int64)


class Chunks:
    """A file's label chunks; raises when pulled after ``close()`` (progressive_sync closes a settled file)."""

    def __init__(self, ref, chunk=pc.SYNC_CHUNK):
        self.ref, self.chunk, self.at, self.closed, self.pulled = ref, chunk, 0, False, 0

    def __iter__(self):
        return self

    def __next__(self):
        assert not self.closed, "pulled after its file settled"
        if self.at >= self.ref.size:
            raise StopIteration
        out = self.ref[self.at:self.at + self.chunk]
        self.at += self.chunk
        self.pulled += 1
        return out.astype(np.uint8)

    def close(self):
        self.closed = True


def _rule(index):
    from ffsubsync_amd.progressive import StopRule

    r = pc.SYNC_RULES[index]
    return StopRule(r["min_psr"], r["min_margin"], r["min_ratio_margin"], r["stable_updates"], r["offset_tolerance"], 0.0)


@pytest.mark.parametrize("rule_index", [0, 1])
def test_stop_update_and_answer_equal_the_model(rule_index):
    from ffsubsync_amd import progressive

    probs = [pc.sync_problem(s) for s in pc.SYNC_SEEDS]
    sources = [Chunks(p[0]) for p in probs]
    res = progressive.progressive_sync([(src, p[1]) for src, p in zip(sources, probs)], _rule(rule_index),
                                       max_offset_seconds=60, top_k=pc.SYNC_TOP_K, exclusion_samples=pc.SYNC_E)
    settled = 0
    for seed, r, src in zip(pc.SYNC_SEEDS, res, sources):
        want = pc.sync_model_run(seed, rule_index)
        st = want["state"]
        assert (r.updates, r.settled, r.consumed_samples) == (want["updates"], want["settled"], st["ref_len"]), seed
        assert (r.ratio_index, r.offset) == (st["best_cand"], st["offset"]) and _bits(r.score) == _bits(st["score"]), seed
        assert r.ratio == probs[seed][3][r.ratio_index]
        assert src.pulled == r.updates and src.closed == r.settled
        assert r.reasons == [] if r.settled else True
        settled += r.settled
    if rule_index == 0:
        assert settled >= 4  # (the test is about stopping)


def test_a_rule_that_never_settles_gives_quality_sync_bit_for_bit():
    from ffsubsync_amd import progressive, quality

    probs = [pc.sync_problem(s) for s in pc.SYNC_SEEDS[:4]]
    res = progressive.progressive_sync([(Chunks(p[0]), p[1]) for p in probs], progressive.StopRule(stable_updates=None))
    want = quality.quality_sync([(p[0].astype(float), p[1]) for p in probs])
    for r, q in zip(res, want):
        assert not r.settled and r.updates == 6 and r.consumed_samples == 60000
        assert (r.ratio_index, r.ratio, r.offset) == (q.ratio_index, q.ratio, q.offset) and _bits(r.score) == _bits(q.score)
        assert r.quality == q.quality and r.reasons == q.reasons


def test_reference_returns_the_bits_fed_and_forms_of_chunks_agree():
    import torch

    from ffsubsync_amd import _native, progressive

    ref, track, _, _ = pc.sync_problem(0)
    cuts = [0, 1, 31, 4000, 33, 2935]
    with progressive.ProgressiveSolve([track, track, track], max_reference_seconds=100) as solve:
        assert solve.reference(1).n == 0
        o = 0
        for i, n in enumerate(cuts):
            chunk = ref[o:o + n]
            o += n
            flat = np.ones(32 * ((8 + n + 31) // 32 + 1), bool)
            flat[8:8 + n] = chunk
            words = torch.from_numpy(np.packbits(flat, bitorder="little").view(np.int32).copy()).cuda()
            labels = torch.from_numpy(np.where(chunk, 1.0, 0.25).astype(np.float32)).cuda()
            got = solve.append({2: chunk.astype(bool) if i % 2 else chunk.astype(np.float64), 0: (words, 8, n), 1: labels})
            assert solve.last_records[0].tobytes() == solve.last_records[1].tobytes() == solve.last_records[2].tobytes()
            assert got[0] == got[1] == got[2] and got[0].ref_len == o
        for f in range(3):
            r = solve.reference(f)
            assert r.n == o == 7000 and (r.lo, r.hi) == (0.0, 1.0)
            assert (_native.unpack_bits(r.bits, r.n).cpu().numpy() != 0).tolist() == ref[:o].tolist()
        with pytest.raises(ValueError, match="exceed max_reference_seconds"):
            solve.append({0: np.zeros(3001, np.uint8)})
    with pytest.raises(ValueError, match="closed"):
        solve.append({0: np.zeros(3, np.uint8)})


def test_pcm_label_chunks_equal_the_pinned_stream_detector():
    import torch

    from ffsubsync_amd import _native, progressive
    from ffsubsync_amd.speech_transformers import detect_pinned_stream

    n = 480 * 20000 + 123  # two 100 s buffers and a partial frame
    pcm = ((np.arange(n) % 977 - 488) * ((np.arange(n) // 48000) % 3) * 20).astype(np.int16)  # loud, quiet and silent seconds
    want = detect_pinned_stream(torch.from_numpy(pcm).pin_memory(), 100, 48000, 0.0, packed=True)
    bits = []
    for source in (pcm, pcm.tobytes(), torch.from_numpy(pcm).pin_memory()):
        got = list(progressive.pcm_label_chunks(source, 100, 48000))
        assert [g[1] for g in got] == [0, 0, 0] and [g[2] for g in got] == [10000, 10000, 1]
        bits.append(np.concatenate([_native.unpack_bits(w, k).cpu().numpy() for w, _, k in got]))
    assert want.n == 20001 and 0 < int(bits[0].sum()) < 20001
    assert bits[0].tolist() == bits[1].tolist() == bits[2].tolist() == _native.unpack_bits(want.bits, want.n).cpu().numpy().tolist()
