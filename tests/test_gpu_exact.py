"""Every solve record pinned to the exact integer reference (tests/exact_reference.py), ties included, on both paths.

The records' contract: per candidate the maximum of the device's fp64 expression over every lag of the
reference's window, ties to the LARGEST lag, exactly 0.0 for lags without overlap; the pair's winner is the first maximal
candidate after the offset filter.  The goldens of the unmodified reference cannot pin a lag inside a tie (their pick
there is FFT noise); this module can, so the fp32 nomination of both paths (the run path's per-tile prefilter, the
transform path's nominee margin and pool), the tile merge, the zero rule and the pair pick are held to it on the
benchmark's own inputs (tests/golden/exact_golden.npz) and on constructed tie families computed at run time.
FFS_FLAG_AMBIGUOUS (2) is allowed only where the transform path's exhaustive pool overflows (test_interleaved_...).
Need a real MI355X.
"""
import json
import os

import numpy as np
import pytest

import exact_reference as er
from exact_check import FLAG_DIRECT, _same_score, check  # noqa: F401  (the shared comparison rule; other suites import it from here)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = er.load_golden(os.path.join(HERE, "golden", "exact_golden.npz"))
RUNS_T = 12288  # lags per run-boundary tile (csrc/ffs_runs.h)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _golden_want(kind):
    want = []
    for g in EXACT[kind]:
        recs = [dict(score=c[0], offset=c[1], n_at_max=c[2], flags=c[3]) for c in g["cand"]]
        want.append((recs, dict(best_cand=g["winner"][0], offset=g["winner"][1], score=g["winner"][2])))
    return want


def _solve(db, max_off, algorithm, pairs_in_flight=64, n_fft=None):
    from ffsubsync_amd import batch

    n_fft = db.required_fft_length(max_off) if n_fft is None else n_fft
    al = batch.BatchAligner(n_fft, db.n_cand, max_off, pairs_in_flight=pairs_in_flight, algorithm=algorithm)
    out = al.solve(db)
    al.close()
    return out


# ---- the benchmark's inputs: tests/golden/exact_golden.npz -------------------------------------------------------------
@pytest.fixture(scope="module")
def headline(torch):
    from workloads import synth

    specs = [synth.make_pair_spec(g["seed"]) for g in EXACT["headline"]]
    db = synth.build_device_batch(specs)
    yield specs, db
    del db
    torch.cuda.empty_cache()


@pytest.mark.parametrize("algorithm", ["runs", "fft"])
def test_headline_fixture_bits(headline, algorithm):
    """All 1024 benchmark pairs as bit-packed vectors (window and filter 6000): 500+ exact-tie records."""
    specs, db = headline
    ties = check(_solve(db, 6000, algorithm, pairs_in_flight=512), _golden_want("headline"), algorithm)
    assert ties >= 500, ties


def test_headline_fixture_bytes_lists_and_sub_batches(headline):
    """The same pairs as 0/1 bytes (runs), as caller-owned boundary lists (runs_from_bits; runs and fft) and split into
    sub-batches of 100 pairs (pairs_in_flight does not divide the call)."""
    from workloads import synth

    specs, db = headline
    want = _golden_want("headline")
    check(_solve(db, 6000, "runs", pairs_in_flight=100), want, "runs/100")
    lists = db.to_runs()
    check(_solve(lists, 6000, "runs", pairs_in_flight=512), want, "lists/runs")
    check(_solve(lists, 6000, "fft", pairs_in_flight=512), want, "lists/fft")
    del lists
    db8 = synth.build_device_batch(specs, packed=False)
    check(_solve(db8, 6000, "runs", pairs_in_flight=512), want, "bytes/runs")


@pytest.mark.parametrize("algorithm", ["runs", "fft"])
def test_windowless_fixture(torch, algorithm):
    """128 benchmark pairs without a lag window or filter: every lag of the reference's convolve, 170+ tiles a candidate
    on the run path."""
    from workloads import synth

    db = synth.build_device_batch([synth.make_pair_spec(g["seed"]) for g in EXACT["windowless"]])
    check(_solve(db, None, algorithm, pairs_in_flight=32), _golden_want("windowless"), algorithm)


# ---- constructed tie families --------------------------------------------------------------------------------------------
def _periodic(rng, P, mean_run):
    """One period of a 0/1 pattern with a sharp autocorrelation (random runs)."""
    seg = np.maximum(1, rng.geometric(1.0 / mean_run, size=P))
    return np.repeat(rng.rand(seg.size) < 0.5, seg)[:P].astype(np.uint8)


def _shared_period(rng, R, S, P, phase, mean_run=20):
    """ref = a period-P pattern, sub = the same pattern at `phase`: on the lags of full overlap (0 <= d <= R-S) every
    d = phase (mod P) ties at the maximum."""
    pat = _periodic(rng, P, mean_run)
    ref = np.resize(pat, R)
    sub = np.resize(np.roll(pat, -phase), S)
    return ref, sub


def _flat_top(R, S, P, a, b, start=0):
    """Reference runs of length a, candidate runs of length b < a, both of period P: plateaus of a - b + 1 consecutive
    tied lags (S a multiple of P keeps the overlap's counts constant)."""
    ref = np.zeros(R, np.uint8)
    for k in range(start, R, P):
        ref[k:k + a] = 1
    sub = np.zeros(S, np.uint8)
    for k in range(0, S, P):
        sub[k:k + b] = 1
    return ref, sub


def _noise(rng, n, mean=40):
    seg = np.maximum(1, rng.geometric(1.0 / mean, size=n))
    return np.repeat(rng.rand(seg.size) < 0.4, seg)[:n].astype(np.uint8)


def _window_top(R, S, max_off):
    lags = er.qm.lag_set(R, S, max_off)
    return int(lags.max()) if lags.size else None


def constructed(max_off, seed=0):
    """(name, ref01, [cand01 x3], ref_levels, [cand_levels x3]) problems whose answers sit inside exact ties."""
    rng = np.random.RandomState(1000 + seed)
    probs = []
    amp = (0.0, 1.0 / 1.001)
    S = 30720
    R = S + 10 * RUNS_T
    P = RUNS_T // 8
    d_lo = int(er.qm.lag_set(R, S, max_off).min()) if er.qm.lag_set(R, S, max_off).size else 0
    d_lo = max(d_lo, -S + 1)
    # periodic plateaus: the tied lags on every tile's last lag, on every tile's first lag, on the window's top lag
    for name, phase in (("tile_last", (d_lo + RUNS_T - 1) % P), ("tile_first", d_lo % P),
                        ("window_top", (_window_top(R, S, max_off) or 0) % P)):
        ref, sub = _shared_period(rng, R, S, P, phase)
        other = np.roll(sub, 7)
        probs.append(("periodic_" + name, ref, [sub, other, sub], (0.0, 1.0), [(0.0, 1.0), (0.0, 1.0), amp]))
    # flat tops of 41 and of 700 consecutive lags (nominee lists hold 16), several per window
    for a, b in ((60, 20), (900, 201)):
        ref, sub = _flat_top(R, S, 3 * 1024, a, b, start=int(rng.randint(0, 3000)))
        probs.append(("flat_top_%d" % (a - b + 1), ref, [sub, sub, np.roll(sub, 5)], (0.0, 1.0), [(0.0, 1.0), amp, (0.0, 1.0)]))
    # the zero rule: a silent reference against an all-ones candidate (every overlapping lag < 0: d_zero wins), a
    # candidate whose lower level maps to 0 (every lag exactly 0.0: the largest lag of the window wins, a real lag or
    # d_zero), and equal best scores across candidates (zeros of a candidate with lower level 0.5 contribute nothing, so a
    # candidate padded by k zeros ties with the unpadded one k lags lower: the first maximal one wins)
    Rz, Sz = 40000, 30000
    ones, silent = np.ones(Sz, np.uint8), np.zeros(Rz, np.uint8)
    probs.append(("all_negative", silent, [ones, ones, _noise(rng, Sz)], (0.0, 1.0), [(0.0, 1.0)] * 3))
    base = _noise(rng, Rz)
    sub = base[5000:5000 + Sz].copy()
    sub[-300:] = 0
    probs.append(("all_zero", base, [np.zeros(Sz, np.uint8), sub, np.zeros(Sz, np.uint8)], (0.0, 1.0),
                  [(0.5, 1.0), (0.5, 1.0), (0.5, 0.9)]))
    padded = np.roll(sub, 300)
    probs.append(("equal_across_candidates", base, [padded, sub, padded], (0.0, 1.0), [(0.5, 1.0)] * 3))
    probs.append(("equal_across_candidates_amp", base, [sub, padded, sub], (0.0, 1.0), [(0.5, 0.95)] * 3))
    return probs


def _pack(torch, probs, byte_vectors=False):
    """Bit-packed (or 0/1 byte) DeviceBatch of host problems."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.batch import DeviceBatch, _layout

    n_cand = len(probs[0][2])
    vecs = [v for p in probs for v in [p[1]] + list(p[2])]
    lens = np.array([v.size for v in vecs], np.int64).reshape(len(probs), 1 + n_cand)
    nbytes = lens if byte_vectors else (lens + 31) // 32 * 4
    offs, total = _layout(lens, nbytes)
    host = np.zeros(total, np.uint8)
    for v, o in zip(vecs, offs.ravel()):
        b = (np.asarray(v) != 0).astype(np.uint8)
        pk = b if byte_vectors else np.packbits(b, bitorder="little")
        host[o:o + pk.size] = pk
    lo = np.array([[p[3][0]] + [lv[0] for lv in p[4]] for p in probs], np.float64)
    hi = np.array([[p[3][1]] + [lv[1] for lv in p[4]] for p in probs], np.float64)
    return DeviceBatch(torch.from_numpy(host).cuda(), offs, lens, lo, hi,
                       _native.FFS_DTYPE_U8 if byte_vectors else _native.FFS_DTYPE_U1)


def _exact(probs, max_off):
    return [er.solve(p[1], p[2], p[3], p[4], max_off, max_off) for p in probs]


@pytest.mark.parametrize("max_off", [None, 100000, 6000, 2000, 0])
def test_constructed_tie_families(torch, max_off):
    """Periodic plateaus across many 12 288-lag tiles, flat tops wider than the nominee lists, ties on the window's top
    lag, the zero rule and equal scores across candidates -- windowless, at wide and narrow windows, and with a window
    that masks every lag (0: the reference's negative slice) -- on both paths."""
    probs = constructed(max_off)
    want = _exact(probs, max_off)
    db = _pack(torch, probs)
    ties = 0
    for algorithm in ("runs", "fft"):
        # (a window that masks every lag needs no transform: the plan is short, so k_direct writes the records)
        ties = check(_solve(db, max_off, algorithm, pairs_in_flight=4), want, (algorithm, max_off), direct=max_off == 0)
    if max_off != 0:
        assert ties >= 10, ties


@pytest.mark.parametrize("max_off", [None, 6000])
def test_interleaved_with_unrelated_pairs(torch, max_off):
    """The constructed problems mixed into one call with unrelated pairs, at pairs_in_flight 1, 2 and 64: a record does
    not depend on its neighbours."""
    rng = np.random.RandomState(77)
    probs = constructed(max_off, seed=1)
    for k in range(12):
        R, S = int(rng.randint(20000, 160000)), int(rng.randint(10000, 60000))
        probs.append(("noise%d" % k, _noise(rng, R), [_noise(rng, S) for _ in range(3)], (0.0, 1.0),
                      [(0.0, 1.0), (0.0, 0.96), (0.0, 1.0)]))
    order = rng.permutation(len(probs))
    probs = [probs[i] for i in order]
    want = _exact(probs, max_off)
    db = _pack(torch, probs)
    n_fft = db.required_fft_length(max_off)
    for algorithm in ("runs", "fft"):
        for pif in (1, 2, 64):
            # (several flat tops in one call can overflow the call's shared pool on the transform path: the one case
            # where a neighbour changes a record, and the record then says so with FFS_FLAG_AMBIGUOUS)
            check(_solve(db, max_off, algorithm, pairs_in_flight=pif, n_fft=n_fft), want, (algorithm, pif),
                  probs=probs if algorithm == "fft" else None, filter_max=max_off)


@pytest.mark.parametrize("max_off", [None, 150, 3])
def test_short_inputs_on_the_direct_kernel(torch, max_off):
    """Plans shorter than 4096 points solve every lag exactly in k_direct: FFS_FLAG_DIRECT on every record, otherwise the
    same rules -- periodic ties, flat tops, the zero rule."""
    rng = np.random.RandomState(5)
    probs = []
    for R, S, P in ((700, 300, 50), (300, 700, 50), (1000, 999, 37)):
        ref, sub = _shared_period(rng, R, S, P, int(rng.randint(P)), mean_run=4)
        fr, fs = _flat_top(R, S, 100, 30, 9)
        probs.append(("direct", ref, [sub, fs, np.ones(S, np.uint8)], (0.0, 1.0), [(0.0, 1.0), (0.0, 0.96), (0.0, 1.0)]))
        probs.append(("direct_zero", np.zeros(R, np.uint8), [np.ones(S, np.uint8), sub, np.zeros(S, np.uint8)], (0.0, 1.0),
                      [(0.0, 1.0), (0.5, 1.0), (0.5, 1.0)]))
    db = _pack(torch, probs, byte_vectors=True)
    n_fft = db.required_fft_length(max_off)
    assert n_fft < 4096
    check(_solve(db, max_off, None, pairs_in_flight=2, n_fft=n_fft), _exact(probs, max_off), max_off, direct=True)


# ---- other input forms ----------------------------------------------------------------------------------------------
def _host_vectors(torch, db, p):
    """Pair p's vectors of a bit-packed DeviceBatch as host 0/1 arrays (read back from the device)."""
    data = db.data.cpu().numpy()
    out = []
    for v in range(db.offs.shape[1]):
        n = int(db.lens[p, v])
        words = data[int(db.offs[p, v]): int(db.offs[p, v]) + (n + 31) // 32 * 4]
        out.append(np.unpackbits(words, bitorder="little")[:n])
    return out


def test_interval_lists(torch):
    """Subtitle interval lists rasterised on the device into bits and into boundary lists (ffs_rasterize_batch_runs):
    both solve to the exact records of the rasterised vectors."""
    from ffsubsync_amd import batch
    from ffsubsync_amd.constants import candidate_ratios
    from workloads import synth

    ratios = candidate_ratios()
    recs = []
    for i in range(6):
        ref = synth.make_subtitle_records(100 + i, duration_s=1800.0)
        s, e, m = synth.make_subtitle_records(200 + i, duration_s=1800.0)
        recs.append((ref, (s + 1_370_000, e + 1_370_000, m)))
    d_bits = batch.pairs_from_intervals(recs, ratios)
    d_runs = batch.pairs_from_intervals(recs, ratios, lists=True)
    want = []
    for p in range(d_bits.n_pairs):
        vec = _host_vectors(torch, d_bits, p)
        want.append(er.solve(vec[0], vec[1:], (d_bits.lo[p, 0], d_bits.hi[p, 0]),
                             [(d_bits.lo[p, j], d_bits.hi[p, j]) for j in range(1, d_bits.offs.shape[1])], 6000, 6000))
    n_fft = d_bits.required_fft_length(6000)
    for db in (d_bits, d_runs):
        for algorithm in ("runs", "fft"):
            check(_solve(db, 6000, algorithm, pairs_in_flight=6, n_fft=n_fft), want, algorithm)


@pytest.mark.parametrize("algorithm", ["runs", "fft"])
def test_dropin_classes_on_host_arrays(torch, monkeypatch, algorithm):
    """FFTAligner / MaxScoreAligner on host float64 arrays of constructed ties and a benchmark pair."""
    from ffsubsync_amd.aligners import FFTAligner, MaxScoreAligner
    from workloads import synth

    monkeypatch.setenv("FFS_ALGORITHM", algorithm)
    probs = constructed(None)[:3] + constructed(None)[5:7]
    for name, ref01, cands01, rl, cls in probs:
        ref = np.where(ref01 != 0, rl[1], rl[0])
        cands = [np.where(c != 0, lv[1], lv[0]) for c, lv in zip(cands01, cls)]
        recs, win = er.solve(ref01, cands01, rl, cls, None)
        for c, r in zip(cands, recs):
            score, offset = FFTAligner().fit_transform(ref, c, get_score=True)
            assert int(offset) == r["offset"] and _same_score(float(score), r["score"]), (name, offset, score, r)
        (score, offset), winner = MaxScoreAligner(FFTAligner()).fit_transform(ref, list(cands))
        assert winner is cands[win["best_cand"]] and int(offset) == win["offset"], name
    spec = synth.make_pair_spec(EXACT["headline"][3]["seed"])
    ref, cands = synth.pair_float_arrays(spec)
    (score, offset), winner = MaxScoreAligner(FFTAligner, None, 100, 60).fit_transform(ref, list(cands))
    (recs, win), = _golden_want("headline")[3:4]
    assert winner is cands[win["best_cand"]] and int(offset) == win["offset"] and _same_score(float(score), win["score"])


@pytest.mark.parametrize("ref_dtype", [np.float64, np.float32])
def test_float_references(torch, ref_dtype):
    """F32 / F64 references with bit-packed candidates.  With (0, 1) levels every record is bit-exact.  With amplitude
    levels the device's re-score sums products of the samples (not the counts' expression), so only the offset is held
    to the reference: its exact score lies within the fp64 summation bound of the maximum."""
    from ffsubsync_amd import _native
    from ffsubsync_amd.batch import DeviceBatch

    for max_off in (None, 6000):
        probs = constructed(max_off)[:5]
        want = _exact(probs, max_off)
        for amps in (False, True):
            db = _pack(torch, [(n, r, c, rl, [(0.0, 1.0)] * 3 if not amps else cl) for n, r, c, rl, cl in probs])
            refs = [p[1].astype(ref_dtype) for p in probs]
            data = db.data.cpu().numpy()
            offs = db.offs.copy()
            base = (data.size + 63) // 64 * 64
            blobs, o = [], base
            for p, r in enumerate(refs):
                offs[p, 0] = o
                blobs.append((o, r.view(np.uint8)))
                o += (r.nbytes + 63) // 64 * 64
            host = np.zeros(o, np.uint8)
            host[: data.size] = data
            for o_, b in blobs:
                host[o_: o_ + b.size] = b
            rd = _native.FFS_DTYPE_F64 if ref_dtype == np.float64 else _native.FFS_DTYPE_F32
            fdb = DeviceBatch(torch.from_numpy(host).cuda(), offs, db.lens, db.lo, db.hi, _native.FFS_DTYPE_U1, ref_dtype=rd)
            ref_want = want if amps else _exact([(n, r, c, rl, [(0.0, 1.0)] * 3) for n, r, c, rl, cl in probs], max_off)
            for algorithm in ("runs", "fft"):
                out = _solve(fdb, max_off, algorithm, pairs_in_flight=4)
                if not amps:
                    check(out, ref_want, (algorithm, max_off, ref_dtype))
                    continue
                cres = out[0]
                for i, (recs, _) in enumerate(ref_want):
                    for j, r in enumerate(recs):
                        name, ref01, cands01, rl, cl = probs[i]
                        d = int(cres[i, j]["offset"])
                        assert d in set(er.qm.lag_set(ref01.size, cands01[j].size, max_off).tolist()), (name, j, d)
                        at = er.score_at(ref01, cands01[j], rl, cl[j], d)
                        bound = 1e-12 * (ref01.size + cands01[j].size)  # fp64 sums of ~1e5 products of magnitude <= 1
                        assert at >= r["score"] - bound, (name, j, d, at, r)


def test_multilevel_references_on_the_run_path(torch):
    """The `weighted` fused VAD's four-level references (tests/test_gpu_levels.py's headline-size pairs) on the run
    path, against the multi-level form of the exact reference (weighted counts M11 / Mx1, LevelInfo coefficients)."""
    from workloads import synth

    gold = json.load(open(os.path.join(HERE, "golden", "float_golden.json")))["pairs"]
    specs = [synth.make_pair_spec(g["seed"]) for g in gold]
    db = synth.build_fused_batch(specs)
    want = []
    for sp in specs:
        _, cands = synth.pair_arrays(sp)
        want.append(er.solve(synth.fused_reference(sp), cands, None, [(0.0, a) for a in sp.cand_amp], 6000, 6000))
    check(_solve(db, 6000, "runs", pairs_in_flight=4), want, "multilevel")
