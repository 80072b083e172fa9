"""Every entry point on hostile input layouts (tests/layout_cases.py): vectors at the least alignment the header grants,
0xFF -- ones, NaNs -- in every byte and bit that is not a sample, other vectors' data right behind a vector's last word.

Table-driven, entry point x layout.  Expected values never come from a device run: the solves are held to
tests/exact_reference.py, the producers to oracle/runs_model.py, tests/ingest_reference.py and oracle/raster_oracle.py,
every block family to its own numpy model through the comparison helper of its own GPU test.  As a localiser only, a
hostile run is also compared byte for byte with the ``clean`` run of the same entry point (the control: what
``batch.pack_pairs`` lays out), so that "wrong everywhere" and "wrong only when shifted" read differently.  After every
call the input image must be unchanged on the device, and where the caller owns the output, so must every byte around it.

Shapes are the smallest at which these kernels can go wrong; across the vectors of every problem set the lengths cover
len % 32 in {0, 1, 31}, word counts % 4 in {0, 1, 2, 3} and a vector shorter than 32 samples
(``layout_cases.length_gaps``, asserted on the host by tests/test_layout_cases_host.py).  The solves' inputs are random
runs with one sharp peak: FFS_FLAG_AMBIGUOUS appears in no record, the control's included.  Need a real MI355X.
"""
import numpy as np
import pytest

import layout_cases as lc

pytestmark = pytest.mark.gpu
FLAG_AMBIGUOUS = 2
K = 256  # block length of every block-family cell
N_FAMILY = 6  # problems per block family, taken from the family's own small set
_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _torch():
    import torch

    return torch


def _out_residues(layout, residues, n):
    """Where the caller-owned outputs of a cell start (mod 64): on 64-byte boundaries under the first two layouts, at the
    element type's least alignments under the other two."""
    return [0] * n if layout in ("clean", "poisoned") else [residues[i % len(residues)] for i in range(n)]


def _dump(x):
    """A result as bytes, for the byte-for-byte comparison with the control."""
    if isinstance(x, (np.ndarray, np.generic)):
        return np.ascontiguousarray(x).tobytes()
    if isinstance(x, (list, tuple)):
        return b"|".join(_dump(v) for v in x)
    if isinstance(x, dict):
        return b"|".join(k.encode() + b"=" + _dump(v) for k, v in sorted(x.items()))
    if hasattr(x, "__dict__"):
        return _dump(vars(x))
    return repr(x).encode()


# ---- producers of vectors -----------------------------------------------------------------------------------------------
VECTOR_LENS = (19, 1, 31, 32, 33, 64, 95, 97, 127, 128, 2999, 3000, 8191, 8192, 8225)
EXTRACT_FIRST = (19, 31, 32, 33, 64, 95, 97, 127)  # the lengths every extraction call starts with
SWEEPS = (65536, 131072, 262144)  # samples of one sweep of the 256-, 512- and 1024-thread extraction


def _runs01(rng, n, i):
    """0/1 vector i of a producer set: empty, full, or random runs of 1 to 400 samples, every seventh with a run that
    reaches the end (its list closes at ``len``: the bits behind it must not count)."""
    if i % 11 == 9:
        return np.zeros(n, np.uint8)
    if i % 11 == 10:
        return np.ones(n, np.uint8)
    run = [1, 2, 7, 60, 400][i % 5]
    x = np.repeat((rng.rand(n // run + 2) < [0.1, 0.5, 0.9][i % 3]).astype(np.uint8), run)[:n]
    if i % 7 == 2:
        x[-1] = 1
    return x


def _vectors():
    def make():
        rng = np.random.RandomState(41)
        return [_runs01(rng, n, i) for i, n in enumerate(VECTOR_LENS)]

    return _once("vectors", make)


def _extract_vectors(n_vec):
    """The vectors of one ``ffs_runs_from_bits_batch`` call: 1 to 3000 samples; the 3-vector call adds lengths one sample
    short of, equal to and 33 past one sweep of each extraction width."""
    def make():
        rng = np.random.RandomState(n_vec)
        lens = [int(n) for n in rng.randint(1, 3001, n_vec)]
        if n_vec == 3:
            lens = [19, 95, 2999] + [s + d for s in SWEEPS for d in (-1, 0, 33)]
        else:
            lens[: len(EXTRACT_FIRST)] = EXTRACT_FIRST
        return [_runs01(rng, n, i if n < 60000 else 2 + 5 * (i % 2)) for i, n in enumerate(lens)]

    return _once(("extract", n_vec), make)


def _want_block(v01, cap):
    """The words of the ``ffs_runs_list`` block of a 0/1 vector up to its sentinel (oracle.runs_model.boundaries)."""
    pos, before = lc.rm.boundaries(v01)
    assert pos.size < cap
    words = np.empty(6 + 2 * pos.size, np.int32)
    words[:4] = (pos.size, int(np.asarray(v01).sum()), np.asarray(v01).size, cap)
    words[4:4 + 2 * pos.size:2], words[5:5 + 2 * pos.size:2] = pos, before
    words[-2:] = (lc.INT32_MAX, words[1])
    return words


def _check_blocks(got, vecs, caps):
    bad = [i for i, (g, v, cap) in enumerate(zip(got, vecs, caps)) if not np.array_equal(g, _want_block(v, cap))]
    return ("list blocks differ from oracle.runs_model.boundaries", bad[:8]) if bad else None


def _list_caps(vecs):
    """Tight for even vectors (n boundaries + the sentinel), three entries to spare for odd ones."""
    return [int(lc.rm.boundaries(v)[0].size) + 1 + 3 * (i % 2) for i, v in enumerate(vecs)]


def _run_pack_bits(layout):
    from ffsubsync_amd import _native

    torch, vecs = _torch(), _vectors()
    img = lc.build(vecs, lc.U8, layout).upload()
    can = lc.Canaries([(v.size + 31) // 32 * 4 for v in vecs], _out_residues(layout, lc.RESIDUES[lc.U1], len(vecs)))
    for i, v in enumerate(vecs):
        o = int(img.offs[i])
        _native.pack_bits(img.data[o:o + v.size], out=can.tensor(i, torch.int32))
    img.assert_inputs_untouched("pack_bits")
    can.assert_canaries_intact("pack_bits")
    return [can.tensor(i).cpu().numpy() for i in range(len(vecs))]


def _check_pack_bits(got):
    import ingest_reference as ir

    bad = [i for i, (g, v) in enumerate(zip(got, _vectors())) if not np.array_equal(g, ir.pack_bits(v))]
    return ("bit images differ from ingest_reference.pack_bits", bad) if bad else None


def _run_unpack_bits(layout):
    from ffsubsync_amd import _native

    vecs = _vectors()
    img = lc.build(vecs, lc.U1, layout).upload()
    got = [_native.unpack_bits(img.data[int(o):int(o) + int(nb)], v.size).cpu().numpy()
           for v, o, nb in zip(vecs, img.offs, img.nbytes)]
    img.assert_inputs_untouched("unpack_bits")
    return got


def _check_unpack_bits(got):
    bad = [i for i, (g, v) in enumerate(zip(got, _vectors())) if not np.array_equal(g, v)]
    return ("samples differ from the vectors", bad) if bad else None


def _run_runs_to_bits(layout):
    from ffsubsync_amd import _native

    torch, vecs = _torch(), _vectors()
    img = lc.build(vecs, lc.RUNS, layout).upload()
    can = lc.Canaries([(v.size + 31) // 32 * 4 for v in vecs], _out_residues(layout, lc.RESIDUES[lc.U1], len(vecs)))
    for i, v in enumerate(vecs):
        _native.runs_to_bits(img.data[int(img.offs[i]):], v.size, out=can.tensor(i, torch.int32))
    img.assert_inputs_untouched("runs_to_bits")
    can.assert_canaries_intact("runs_to_bits")
    return [can.tensor(i).cpu().numpy() for i in range(len(vecs))]


def _run_runs_from_bits(layout):
    from ffsubsync_amd import _native

    torch, vecs = _torch(), _vectors()
    caps = _list_caps(vecs)
    img = lc.build(vecs, lc.U1, layout).upload()
    can = lc.Canaries([16 + 8 * c for c in caps], _out_residues(layout, lc.RESIDUES[lc.RUNS], len(vecs)))
    for i, v in enumerate(vecs):
        _native.runs_from_bits(img.data[int(img.offs[i]):], v.size, caps[i], out=can.tensor(i, torch.int32))
    img.assert_inputs_untouched("runs_from_bits")
    can.assert_canaries_intact("runs_from_bits")
    return [can.tensor(i, torch.int32).cpu().numpy() for i in range(len(vecs))]


def _blocks_to_sentinel(got):
    return [g[: 6 + 2 * int(g[0])] for g in got]


def _run_extract(n_vec):
    def run(layout):
        from ffsubsync_amd import _native

        torch, vecs = _torch(), _extract_vectors(n_vec)
        caps = _list_caps(vecs)
        img = lc.build(vecs, lc.U1, layout).upload()
        can = lc.Canaries([16 + 8 * c for c in caps], _out_residues(layout, lc.RESIDUES[lc.RUNS], len(vecs)))
        _native.runs_from_bits_batch(img.ptrs(), img.lens, [can.ptr(i) for i in range(len(vecs))], caps)
        img.assert_inputs_untouched("runs_from_bits_batch")
        can.assert_canaries_intact("runs_from_bits_batch")
        raw = can.buf.cpu().numpy()
        return [raw[o:o + 16 + 8 * c].view(np.int32) for o, c in zip(can.offs, caps)]

    return run


def _raster_tracks():
    """Three short subtitle tracks at three framerate ratios: nine vectors of 2000 to 7000 samples, and what the unmodified
    reference's rasteriser makes of them (oracle.raster_oracle)."""
    def make():
        from oracle import raster_oracle as ro
        from workloads import synth

        tracks = [synth.make_subtitle_records(300 + t, duration_s=23.0 + 19.0 * t) for t in range(3)]
        ratios = (1.0, 1.0417, 0.96)
        track_of = np.repeat(np.arange(3), 3)
        ratio = np.tile(ratios, 3)
        want = [(ro.rasterize(*tracks[t], r) != 0).astype(np.uint8) for t, r in zip(track_of, ratio)]
        return tracks, track_of, ratio, want

    return _once("raster", make)


def _run_rasterize_bits(layout):
    from ffsubsync_amd import _native, batch

    torch = _torch()
    tracks, track_of, ratio, want = _raster_tracks()
    ts = batch.TrackSet(tracks)
    lens = _native.raster_lengths(ts.end_max[track_of], ratio, 100)
    words = (lens + 31) // 32
    if layout in ("clean", "poisoned"):  # 64-byte slots
        at = np.concatenate([[0], np.cumsum((words + 15) // 16 * 16)[:-1]])
    elif layout == "shifted":  # word offsets 1, 2, 3, 5, 15 (mod 16)
        at, cursor = [], 0
        for i, w in enumerate(words):
            cursor += ((1, 2, 3, 5, 15)[i % 5] - cursor) % 16
            at.append(cursor)
            cursor += int(w)
        at = np.array(at)
    else:  # every vector on the heel of the one in front
        at = np.concatenate([[0], np.cumsum(words)[:-1]])
    total = int(at[-1] + words[-1])
    out, can = lc.canaried((total,), torch.int32, _out_residues(layout, lc.RESIDUES[lc.U1], 2)[1])
    _native.rasterize_batch_bits(ts.start_us, ts.end_us, ts.meta, ts.firsts[track_of], ts.counts[track_of], ratio, at, lens, out,
                                 100, 0.0)
    can.assert_canaries_intact("rasterize_batch_bits")
    raw = out.cpu().numpy().view(np.uint8)
    # the call zeroes its whole output, then fills the vectors in: what lies between them is part of the result
    between = np.ones(raw.size, bool)
    for a, w in zip(at, words):
        between[4 * int(a): 4 * int(a + w)] = False
    return dict(lens=lens, vectors=[raw[4 * int(a): 4 * int(a + w)] for a, w in zip(at, words)], gaps=int(raw[between].any()))


def _check_rasterize_bits(got):
    import ingest_reference as ir

    want = _raster_tracks()[3]
    if [int(n) for n in got["lens"]] != [w.size for w in want] or got["gaps"]:
        return ("lengths or the bytes between the vectors", got["lens"], got["gaps"])
    bad = [i for i, (g, w) in enumerate(zip(got["vectors"], want)) if not np.array_equal(g, ir.pack_bits(w))]
    return ("rasters differ from oracle.raster_oracle.rasterize", bad) if bad else None


def _run_rasterize_runs(layout):
    from ffsubsync_amd import _native, batch

    tracks, track_of, ratio, want = _raster_tracks()
    ts = batch.TrackSet(tracks)
    lens = _native.raster_lengths(ts.end_max[track_of], ratio, 100)
    counts = ts.counts[track_of]
    caps = [2 * int(c) + 1 + (i % 2) for i, c in enumerate(counts)]  # the least the entry point accepts, and one more
    can = lc.Canaries([16 + 8 * c for c in caps], _out_residues(layout, lc.RESIDUES[lc.RUNS], len(caps)))
    first, end = can.offs[0], can.offs[-1] + can.slot_bytes[-1]
    _native.rasterize_batch_runs(ts.start_us, ts.end_us, ts.meta, ts.firsts[track_of], counts, ratio,
                                 np.array(can.offs) - first, caps, lens, can.buf[first:end], 100, 0.0)
    can.assert_canaries_intact("rasterize_batch_runs")
    raw = can.buf.cpu().numpy()
    return dict(caps=caps, blocks=_blocks_to_sentinel([raw[o:o + 16 + 8 * c].view(np.int32) for o, c in zip(can.offs, caps)]))


def _check_rasterize_runs(got):
    return _check_blocks(got["blocks"], _raster_tracks()[3], got["caps"])


# ---- solves ------------------------------------------------------------------------------------------------------------
# pair 0: R and S between 3000 and 9000 (no window: up to 17 960 lags, two 12 288-lag tiles); pair 1: R + S <= 2048, a
# plan below 4096 points (the direct kernel).  Three candidates each, one of them 19 samples long.  A record shows only the
# best lag, so the true offsets sit where what lies behind a vector's end would change it.  The run path updates its counts
# from lag to lag with the 32-bit edge words of both vectors (fetch32), and rescoring masks the partial last words:
#   candidate 0 (S = 8000): offset 1010 -- the reference's last word (24 bits behind R = 9000) passes the candidate's end
#     at lags 1000..1023;
#   candidate 1 (S = 8961, 31 bits behind it in its last word): offset 21, inside the +-150 window -- its end lies 18
#     samples in front of the reference's, the bits behind it leave the edge word at lags 8..38;
#   candidate 2 (S = 7969, 31 bits behind it): offset 1018, the same 1031 - 13 samples from the other end of the lag range.
SOLVE_LENS = ((9000, (8000, 8961, 7969)), (1119, (896, 19, 929)))
SOLVE_SHIFTS = ((1010, 21, 1018), (-40, 500, 1119 - 929 - 60))
SOLVE_AMPS = (1.0, 0.96, 1.0)
WINDOWS = (None, 150)


def _solve_problems():
    """Random runs with one sharp peak: every candidate is a window of its reference with 5 % of its samples flipped."""
    def make():
        rng = np.random.RandomState(2026)
        out = []
        for (R, lens), shifts in zip(SOLVE_LENS, SOLVE_SHIFTS):
            seg = np.maximum(1, rng.geometric(1.0 / 40.0, size=R // 10 + 16))
            ref = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R].astype(np.uint8)
            ref[0], ref[1] = 1, 0
            cands = []
            for S, sh in zip(lens, shifts):
                idx = np.arange(S) + sh
                ok = (idx >= 0) & (idx < R)
                c = np.zeros(S, np.uint8)
                c[ok] = ref[idx[ok]]
                cands.append(c ^ (rng.rand(S) < 0.05))
            # the four-level reference of a weighted fused detector: 0.6 a + 0.4 b of two label vectors that mostly agree
            other = ref ^ (np.repeat(rng.rand(R // 25 + 1) < 0.08, 25)[:R]).astype(np.uint8)
            out.append(dict(ref=ref, cands=cands, fused=0.6 * ref + 0.4 * other))
        assert np.unique(out[0]["fused"]).size == 4
        return out

    return _once("solve", make)


SOLVE_TYPES = {
    # name: (reference element type, candidate element type, candidate amplitudes)
    "u1": (lc.U1, lc.U1, SOLVE_AMPS),
    "u8": (lc.U8, lc.U8, SOLVE_AMPS),
    "f32": (lc.F32, lc.F32, (1.0, 1.0, 1.0)),  # (float samples are their own values: a 0/1 vector has the levels 0 and 1)
    "f64ref": (lc.F64, lc.U1, (1.0, 1.0, 1.0)),  # (bit-exact records need 0/1 levels here: tests/test_gpu_exact.py)
    "lists": (lc.RUNS, lc.RUNS, SOLVE_AMPS),
    "levels": (lc.F64, lc.U1, SOLVE_AMPS),  # the four-level float64 reference (k_runs_corr_ml on the run path)
}


def _solve_want(kind, pair, window):
    """``exact_reference.solve`` of one pair (computed once)."""
    def make():
        import exact_reference as er

        pr, amps = _solve_problems()[pair], SOLVE_TYPES[kind][2]
        levels = [(0.0, a) for a in amps]
        if kind == "levels":
            return er.solve(pr["fused"], pr["cands"], None, levels, window, window)
        return er.solve(pr["ref"], pr["cands"], (0.0, 1.0), levels, window, window)

    return _once(("want", kind if kind == "levels" else SOLVE_TYPES[kind][2], pair, window), make)


def _run_solve(kind, path):
    pair = 1 if path == "direct" else 0

    def run(layout):
        from ffsubsync_amd import _native, batch

        torch, probs = _torch(), _solve_problems()
        rk, ck, amps = SOLVE_TYPES[kind]
        vecs = [v for pr in probs for v in [pr["fused"] if kind == "levels" else pr["ref"]] + pr["cands"]]
        img = lc.build(vecs, [rk, ck, ck, ck] * len(probs), layout).upload()
        hi = [[1.0] + list(amps)] * len(probs)
        db = img.device_batch((len(probs), 4), np.zeros((len(probs), 4)), hi, ck, None if rk == ck else rk)
        out = {}
        for window in WINDOWS:
            n_fft = max(_native.plan_length(db.lens[pair, 0], s, window) for s in db.lens[pair, 1:])
            assert (n_fft < 4096) == (path == "direct"), n_fft
            cres, can_c = lc.canaried((3 * 24,), torch.uint8, _out_residues(layout, lc.RESIDUES[lc.F64], 3)[1])
            pres, can_p = lc.canaried((24,), torch.uint8, _out_residues(layout, lc.RESIDUES[lc.F64], 3)[2])
            al = batch.BatchAligner(n_fft, 3, window, pairs_in_flight=1, algorithm=None if path == "direct" else path)
            al.solve_async(db, pair, pair + 1, cand_out=cres, pair_out=pres)
            c = cres.cpu().numpy().view(_native.CAND_RESULT_DTYPE).reshape(1, 3)
            p = pres.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)
            stats = al.plan.runs_stats()  # (calls that tried the run-boundary path, their sub-batches, those that left it)
            al.close()
            img.assert_inputs_untouched("solve %s/%s/%s" % (kind, path, window))
            can_c.assert_canaries_intact("candidate records %s/%s/%s" % (kind, path, window))
            can_p.assert_canaries_intact("pair record %s/%s/%s" % (kind, path, window))
            out[window] = (c, p, stats)
        return out

    def check(got):
        from test_gpu_exact import check as records_equal_exact

        for window in WINDOWS:
            c, p, stats = got[window]
            # the cell runs the kernels it is named after (float candidates have no boundary lists: they take the transforms)
            on_runs = path == "runs" and kind != "f32"
            if (stats[0] >= 1 and stats[2] == 0) != on_runs:
                return ("run-boundary path taken: %s, expected: %s" % (stats, on_runs), window)
            if (c["flags"] & FLAG_AMBIGUOUS).any():
                return ("FFS_FLAG_AMBIGUOUS", window, c["flags"].tolist())
            try:
                records_equal_exact((c, p), [_solve_want(kind, pair, window)], (kind, path, window), direct=path == "direct")
            except AssertionError as e:
                return ("records differ from exact_reference.solve", str(e)[:600])
        return None

    def contract(got):  # the fields the header defines (score_f32 is a diagnostic of the fp32 nomination)
        return [(c[["score", "offset", "flags"]].tolist(), p[["score", "offset", "best_cand", "flags"]].tolist()) for c, p, _ in got.values()]

    return run, check, contract


def _run_correlate(kind):
    """``ffs_correlate_full``: the raw fp32 correlation arrays of pair 0's reference against its first two candidates --
    what the transform kernels make of the samples before any nomination or exact re-scoring can hide it."""
    N = 1 << 15
    element = dict(u8=lc.U8, u1=lc.U1, f32=lc.F32, f64=lc.F64)[kind]
    amp = 1.0 if element in (lc.F32, lc.F64) else 0.96

    def run(layout):
        from ffsubsync_amd import _native

        torch, pr = _torch(), _solve_problems()[0]
        vecs = [pr["ref"], pr["cands"][0], pr["cands"][1]]
        img = lc.build(vecs, element, layout).upload()
        view = {lc.U8: torch.uint8, lc.U1: torch.int32, lc.F32: torch.float32, lc.F64: torch.float64}[element]
        t = [img.data[int(o):int(o) + int(nb)].view(view) for o, nb in zip(img.offs, img.nbytes)]
        plan = _native.Plan(N, 1, 2)
        out_a, out_b = plan.correlate_full(element, t[0], (0, 1), t[1], (0, 1), t[2], (0.0, amp), lens=[v.size for v in vecs])
        got = (out_a.cpu().numpy(), out_b.cpu().numpy())
        plan.close()
        img.assert_inputs_untouched("correlate_full/" + kind)
        return got

    def check(got):
        from test_gpu_parity import _direct_corr

        pr = _solve_problems()[0]
        ref = 2.0 * pr["ref"] - 1
        want = (_direct_corr(ref, 2.0 * pr["cands"][0] - 1, N), _direct_corr(ref, 2.0 * (amp * pr["cands"][1]) - 1, N))
        # A lag is nominated when its fp32 value lies within the margin of the fp32 maximum, and the data-independent part
        # of that margin is eps32 log2(N) sqrt(R S) |s||r| (finish_cand_for_transforms): the true maximum is always among
        # the nominees as long as every value is off by less than HALF of it.  (tests/test_gpu_parity.py holds vectors of
        # N / 2 samples to an eighth; these are shorter, and two fp32 ulps of their largest output are an eighth already.)
        tol = 0.5 * 5.9604645e-08 * np.log2(N) * np.sqrt(pr["ref"].size * min(c.size for c in pr["cands"][:2]))
        err = [float(np.abs(g - w).max()) for g, w in zip(got, want)]
        return ("fp32 correlation arrays off by %s, bound %.3g" % (err, tol)) if not max(err) < tol else None

    return run, check, _dump


# ---- block families ----------------------------------------------------------------------------------------------------
FAMILY_SOURCES = {  # family: (the GPU test module that owns its small set, the set or the function that makes it)
    "split": ("test_gpu_split", "SMALL"), "split_range": ("test_gpu_cut", "SMALL"), "drift": ("test_gpu_drift", "_fuzz_problems"),
    "drift_range": ("test_gpu_drift_range", "SMALL"), "smooth": ("test_gpu_drift_smooth", "_fuzz_problems"),
    "smooth_range": ("drift_range_smooth_cases", "SMALL"), "split_report": ("test_gpu_split_report", "SMALL"),
    "cut_report": ("test_gpu_cut_report", "_small_problems"), "drift_report": ("test_gpu_drift_report", "_fuzz_problems"),
    "split_refine": ("test_gpu_split_refine", "SMALL"), "quality": ("test_gpu_quality", "SMALL"), "match": ("test_gpu_match", "SMALL"),
}


def _family_problems(name):
    """The first N_FAMILY problems of a family's own small set that run at K = 256 (and, over a lag range, hold at most
    100 000 lags: the models stay quick), their vectors shortened by fewer than 160 samples so that the set's lengths
    cover every residue (``layout_cases.cover_lengths``); the last subtitle vector keeps 19 samples."""
    def make():
        import importlib

        module, attr = FAMILY_SOURCES[name]
        source = getattr(importlib.import_module(module), attr)
        pick = [pr for pr in (source() if callable(source) else source) if pr.get("k", K) == K and min(pr["rb"].size, pr["sb"].size) >= 192
                and pr.get("hi", 0) - pr.get("lo", 0) < 100000][:N_FAMILY]
        assert len(pick) == N_FAMILY, (name, len(pick))
        lens = lc.cover_lengths([n for pr in pick for n in (pr["rb"].size, pr["sb"].size)])
        out = []
        for i, pr in enumerate(pick):
            rb, sb = pr["rb"][: lens[2 * i]], pr["sb"][: lens[2 * i + 1]]
            out.append(dict(pr, rb=rb, sb=sb))
        return out

    return _once(("family", name), make)


def _family_image(probs, layout, kind=lc.U1):
    img = lc.build([v for pr in probs for v in (pr["rb"], pr["sb"])], kind, layout).upload()
    lo = [[pr["r_lv"][0], pr["s_lv"][0]] for pr in probs]
    hi = [[pr["r_lv"][1], pr["s_lv"][1]] for pr in probs]
    return img, img.device_batch((len(probs), 2), lo, hi, kind)


def _row(db, p):
    from ffsubsync_amd.batch import DeviceBatch

    return DeviceBatch(db.data, db.offs[p:p + 1], db.lens[p:p + 1], db.lo[p:p + 1], db.hi[p:p + 1], db.dtype)


FAMILY_MODELS = {}  # family: (model, same) as ``_families`` assembles them (tests/stream_cases.py reads them too)


def _family(name, call, model, same):
    """One block family: ``call(row, pr)`` on the one-pair view of every problem in the hostile image, ``model(pr)`` its
    numpy model, ``same(got, want, pr)`` the family's own comparison (None or true when equal)."""
    FAMILY_MODELS[name] = (model, same)

    def run(layout):
        probs = _family_problems(name)
        img, db = _family_image(probs, layout)
        got = []
        for p, pr in enumerate(probs):
            got.append(call(_row(db, p), pr))
            img.assert_inputs_untouched("%s, problem %d" % (name, p))
        return got

    def check(got):
        probs = _family_problems(name)
        want = _once(("model", name), lambda: [model(pr) for pr in probs])
        bad = []
        for p, (g, w, pr) in enumerate(zip(got, want, probs)):
            verdict = same(g, w, pr)  # None, true or an empty list of differences: equal
            if not (verdict is None or (isinstance(verdict, (bool, np.bool_)) and verdict) or verdict == []):
                bad.append((p, verdict))
        return ("differs from the family's numpy model", bad) if bad else None

    return run, check, _dump


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _split_same(res, want, pr):
    offs, scores, total = want[:3]
    return (np.array_equal(np.asarray(res.block_offsets, np.int64), offs) and np.array_equal(_bits64(res.block_scores), _bits64(scores))
            and _bits64([res.total])[0] == _bits64([total])[0])


def _families():
    import cut_model as cm
    import cut_report_model as crm
    import drift_model as dm
    import drift_range_smooth_model as drsm
    import split_model as sm
    import split_refine_model as rfm
    import split_report_model as srm
    import test_gpu_drift as t_drift
    import test_gpu_drift_range as t_drange
    import test_gpu_drift_range_smooth as t_drsmooth
    import test_gpu_drift_report as t_drep
    import test_gpu_drift_smooth as t_dsmooth
    import test_gpu_quality as t_quality
    import test_gpu_split_refine as t_refine
    import test_gpu_split_report as t_srep

    def split_call(row, pr):
        from ffsubsync_amd import split_align as sa

        return sa.split_align_batch(row, pr["w"], K, pr["p"])[0]

    def split_same(res, want, pr):
        pieces = [(p.first_block, p.end_block, p.start_sample, p.end_sample, p.offset, p.score) for p in res.pieces]
        return _split_same(res, want, pr) and pieces == want[3]

    def range_call(row, pr):
        from ffsubsync_amd import cut_align as ca

        return ca.split_align_range_batch(row, (pr["lo"], pr["hi"]), K, pr["p"])[0]

    def drift_call(row, pr):
        from ffsubsync_amd import drift_align as da

        return da.drift_align_batch(row, pr["w"], K, pr["p"], pr["s"], pr["q"])[0]

    def drange_call(row, pr):
        from ffsubsync_amd import drift_range as dr

        return dr.drift_align_range_batch(row, (pr["lo"], pr["hi"]), K, pr["p"], pr["s"], pr["q"])[0]

    def smooth_call(row, pr):
        from ffsubsync_amd import drift_smooth as ds

        return ds.smooth_align_batch(row, pr["w"], K, pr["p"], pr["s"], pr["q"], pr["m"], pr["r"], pr["lam"], raw=True)

    def smooth_same(raw, want, pr):
        res, smooth, knot, recs, counts = raw
        want_solve, want_smooth, want_knot, want_recs = want
        n, nb = len(want_recs), want_smooth.size
        if not t_drift._same(res[0], want_solve) or int(counts[0]) != n:
            return ["drift solve or segment count"]
        d = t_dsmooth._diff(recs[0, :n], want_recs)
        d += [] if np.array_equal(smooth[0, :nb], want_smooth) and not smooth[0, nb:].any() else ["smooth_offset"]
        d += [] if np.array_equal(knot[0, :nb], want_knot) and not knot[0, nb:].any() else ["knot"]
        return d + (["records past the count"] if recs[0, n:].tobytes().strip(b"\0") else [])

    def srange_call(row, pr):
        from ffsubsync_amd import drift_range_smooth as drs

        return drs.smooth_align_range_batch(row, (pr["lo"], pr["hi"]), K, pr["p"], pr["s"], pr["q"], pr["m"], pr["r"],
                                            pr["lam"], raw=True)

    def srep_call(row, pr):
        from ffsubsync_amd import split_report as sr

        return sr.split_report_batch(row, pr["w"], K, pr["p"], pr["top_k"], pr["e"], raw=True)

    def srep_same(raw, want, pr):
        res, recs, counts = raw
        return _split_same(res[0], want[0], pr) and t_srep._records_equal(recs[0, :int(counts[0])], want[1]) \
            and not recs[0, int(counts[0]):].tobytes().strip(b"\0")

    def cutrep_call(row, pr):
        from ffsubsync_amd import cut_report as cr

        return cr.split_range_report_batch(row, (pr["lo"], pr["hi"]), K, pr["p"], pr["top_k"], pr["e"], raw=True)

    def cutrep_model(pr):
        solve = cm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["lo"], pr["hi"], pr["p"])
        return solve, crm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["lo"], pr["hi"], solve[0], pr["top_k"], pr["e"])[0]

    def cutrep_same(raw, want, pr):
        res, recs, counts = raw
        n = int(counts[0])
        return _split_same(res[0], want[0], pr) and n == want[1].size and recs[0, :n].tobytes() == want[1].tobytes() \
            and not recs[0, n:].tobytes().strip(b"\0")

    def drep_call(row, pr):
        from ffsubsync_amd import drift_report as dr

        return dr.drift_report_batch(row, pr["w"], K, pr["p"], pr["s"], pr["q"], pr["top_k"], pr["excl"], raw=True)

    def drep_same(raw, want, pr):
        res, recs, counts = raw
        want_solve, want_recs = want[:2]
        n = len(want_recs)
        if not t_drift._same(res[0], want_solve) or int(counts[0]) != n:
            return ["drift solve or segment count"]
        return t_drep._diff(recs[0, :n], want_recs) + (["records past the count"] if recs[0, n:].tobytes().strip(b"\0") else [])

    def refine_call(row, pr):
        from ffsubsync_amd import split_align as sa
        from ffsubsync_amd import split_refine as sr

        res = sa.split_align_batch(row, pr["w"], K, pr["p"])
        recs, counts = sr.refine_breaks_batch(row, res, K, pr["radius"], pr["beta"], raw=True)
        return res[0], recs, counts

    def refine_model(pr):
        solve = sm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["w"], pr["p"])
        return solve, rfm.refine(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], np.asarray(solve[0], np.int32), K, pr["radius"],
                                 pr["beta"])

    def refine_same(got, want, pr):
        res, recs, counts = got
        n = int(counts[0])
        return _split_same(res, want[0], pr) and t_refine._records_equal(recs[0, :n], want[1]) \
            and not recs[0, n:].tobytes().strip(b"\0")

    def quality_call(row, pr):
        from ffsubsync_amd import quality

        return quality.quality_batch(row, pr["w"], pr["top_k"], pr["e"], raw=True)[0]

    def quality_same(rec, want, pr):
        from ffsubsync_amd import quality

        return t_quality._compare(quality.from_record(rec), pr)  # (the helper runs the model itself)

    fam = {}
    fam["split_align_batch"] = _family("split", split_call,
                                       lambda pr: sm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["w"], pr["p"]), split_same)
    fam["split_align_range_batch"] = _family("split_range", range_call,
                                             lambda pr: cm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["lo"], pr["hi"], pr["p"]),
                                             _split_same)
    fam["drift_align_batch"] = _family("drift", drift_call,
                                       lambda pr: dm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["w"], pr["p"], pr["s"], pr["q"]),
                                       lambda res, want, pr: t_drift._same(res, want))
    fam["drift_align_range_batch"] = _family("drift_range", drange_call, t_drange._model,
                                             lambda res, want, pr: t_drange._same(res, want))
    fam["smooth_align_batch"] = _family("smooth", smooth_call, t_dsmooth._model, smooth_same)
    fam["smooth_align_range_batch"] = _family(
        "smooth_range", srange_call,
        lambda pr: drsm.solve(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["lo"], pr["hi"], pr["p"], pr["s"], pr["q"], pr["m"],
                              pr["r"], pr["lam"]),
        lambda raw, want, pr: t_drsmooth._diff(raw, 0, want))
    fam["split_report_batch"] = _family(
        "split_report", srep_call,
        lambda pr: srm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], K, pr["w"], pr["p"], pr["top_k"], pr["e"])[:2], srep_same)
    fam["split_range_report_batch"] = _family("cut_report", cutrep_call, cutrep_model, cutrep_same)
    fam["drift_report_batch"] = _family("drift_report", drep_call, t_drep._model, drep_same)
    fam["split_refine"] = _family("split_refine", refine_call, refine_model, refine_same)
    fam["quality_batch"] = _family("quality", quality_call, lambda pr: None, quality_same)
    return fam


def _run_match(algorithm):
    """``match.quality_from_lists`` with hostile list blocks in both roles: one table of references, one of subtitle
    vectors, every problem a call of its own at its own window, top_k and exclusion distance."""
    def run(layout):
        from ffsubsync_amd import match

        probs = _family_problems("match")
        img, db = _family_image(probs, layout, lc.RUNS)
        ptr = img.ptrs().reshape(-1, 2)
        got = []
        for p, pr in enumerate(probs):
            got.append(match.quality_from_lists(ptr[:, 0], db.lens[:, 0], db.lo[:, 0], db.hi[:, 0], ptr[:, 1], db.lens[:, 1],
                                                db.lo[:, 1], db.hi[:, 1], [p], [p], pr["w"], pr["top_k"], pr["e"], algorithm)[0])
            img.assert_inputs_untouched("match/%s, problem %d" % (algorithm, p))
        return got

    def check(got):
        import test_gpu_match as t_match
        from ffsubsync_amd import quality

        bad = [(p, why) for p, (rec, pr) in enumerate(zip(got, _family_problems("match")))
               for why in [t_match._compare(quality.from_record(rec), pr)] if why is not None]
        return ("differs from quality_model.report", bad) if bad else None

    return run, check, _dump


# ---- the table ---------------------------------------------------------------------------------------------------------
def _entries():
    def make():
        e = {
            "pack_bits": (_run_pack_bits, _check_pack_bits, _dump),
            "unpack_bits": (_run_unpack_bits, _check_unpack_bits, _dump),
            "runs_to_bits": (_run_runs_to_bits, _check_pack_bits, _dump),
            "runs_from_bits": (_run_runs_from_bits, lambda got: _check_blocks(_blocks_to_sentinel(got), _vectors(), _list_caps(_vectors())),
                               lambda got: _dump(_blocks_to_sentinel(got))),
            "rasterize_batch_bits": (_run_rasterize_bits, _check_rasterize_bits, _dump),
            "rasterize_batch_runs": (_run_rasterize_runs, _check_rasterize_runs, _dump),
        }
        for n_vec in (3, 300, 800):
            e["runs_from_bits_batch-%d" % n_vec] = (
                _run_extract(n_vec),
                lambda got, n_vec=n_vec: _check_blocks(_blocks_to_sentinel(got), _extract_vectors(n_vec), _list_caps(_extract_vectors(n_vec))),
                lambda got: _dump(_blocks_to_sentinel(got)))
        for kind in SOLVE_TYPES:
            for path in (("runs",) if kind == "levels" else ("runs", "fft", "direct")):
                e["solve-%s-%s" % (kind, path)] = _run_solve(kind, path)
        for kind in ("u8", "u1", "f32", "f64"):
            e["correlate_full-%s" % kind] = _run_correlate(kind)
        e.update(_families())
        for algorithm in ("runs", "bits"):
            e["match.quality_from_lists-%s" % algorithm] = _run_match(algorithm)
        return e

    return _once("entries", make)


ENTRY_NAMES = (
    ["pack_bits", "unpack_bits", "runs_to_bits", "runs_from_bits", "runs_from_bits_batch-3", "runs_from_bits_batch-300",
     "runs_from_bits_batch-800", "rasterize_batch_bits", "rasterize_batch_runs"]
    + ["solve-%s-%s" % (k, p) for k in SOLVE_TYPES for p in (("runs",) if k == "levels" else ("runs", "fft", "direct"))]
    + ["correlate_full-%s" % k for k in ("u8", "u1", "f32", "f64")]
    + ["split_align_batch", "split_align_range_batch", "drift_align_batch", "drift_align_range_batch", "smooth_align_batch",
       "smooth_align_range_batch", "split_report_batch", "split_range_report_batch", "drift_report_batch", "split_refine",
       "quality_batch", "match.quality_from_lists-runs", "match.quality_from_lists-bits"])


def problem_set_lengths():
    """{problem set: its vector lengths}, for tests/test_layout_cases_host.py (host data only)."""
    sets = {"vectors": list(VECTOR_LENS), "solve": [n for R, lens in SOLVE_LENS for n in (R,) + lens]}
    for n_vec in (3, 300, 800):
        sets["extract%d" % n_vec] = [v.size for v in _extract_vectors(n_vec)]
    for name in FAMILY_SOURCES:
        sets[name] = [n for pr in _family_problems(name) for n in (pr["rb"].size, pr["sb"].size)]
    return sets


def _clean(name):
    """The control run of an entry point (once per session)."""
    return _once(("clean", name), lambda: _entries()[name][0]("clean"))


def test_the_table_is_complete():
    assert sorted(ENTRY_NAMES) == sorted(_entries()) and len(set(ENTRY_NAMES)) == len(ENTRY_NAMES)


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_clean_control(name):
    """The control layout against the independent reference (solves: no FFS_FLAG_AMBIGUOUS in any record)."""
    run, check, dump = _entries()[name]
    why = check(_clean(name))
    assert why is None, (name, "clean", why)


# (layout-major: poisoned before shifted before abutting, so the first failure names the mildest layout that breaks)
@pytest.mark.parametrize("layout,name", [(layout, name) for layout in lc.HOSTILE for name in ENTRY_NAMES])
def test_hostile_layout(layout, name):
    run, check, dump = _entries()[name]
    got = run(layout)
    why = check(got)
    same = dump(got) == dump(_clean(name))
    if why is not None or not same:
        clean_why = check(_clean(name))
        pytest.fail("%s [%s]: against the reference: %s; against the clean run: %s; the clean run against the reference: %s"
                    % (name, layout, "equal" if why is None else why, "byte-identical" if same else "DIFFERS",
                       "equal" if clean_why is None else clean_why))
