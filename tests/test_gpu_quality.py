"""Alignment quality report on the device (csrc/ffs_quality.h via ffsubsync_amd.quality): against the numpy model on
seeded small problems, peak 1 against the seven-ratio solve's own records on the headline goldens, input forms and
batching, quality_sync's verdicts on matched and wrong pairs, and argument errors."""
import json
import os

import numpy as np
import pytest

import quality_model as qm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _device_pairs(problems, packed=True):
    """DeviceBatch (one candidate per pair) from host (ref values, sub values) pairs of two-level float vectors."""
    from ffsubsync_amd import batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    pairs = [(DeviceRaster.from_host(r, lists=False), [DeviceRaster.from_host(s, lists=False)]) for r, s in problems]
    return batch.pack_pairs(pairs, packed=packed)


def _small_problems(n=64):
    """R < S and R > S, non-default levels and amplitudes 1/ratio, top_k 1..8, E from 1 to beyond the window,
    windowless on short vectors, windows past both ends and the negative-slice window."""
    out = []
    for seed in range(n):
        rng = np.random.RandomState(3000 + seed)
        R, S = int(rng.randint(40, 12000)), int(rng.randint(40, 12000))
        w = [None, 1, 2, 37, 300, 2500, 6000, 30000][seed % 8]
        if w is None:
            R, S = R % 3000 + 40, S % 3000 + 40
        if seed % 16 == 15:  # negative-slice window: W past N - 1 - S
            R, S = int(rng.randint(40, 400)), int(rng.randint(400, 900))
            w = qm.orc.fft_length(R, S) - S + int(rng.randint(0, 30))
        top_k = 1 + seed % 8
        e = [1, 2, 50, 300, 5000, 10 ** 6][seed % 6]
        r_lv = [(0.0, 1.0), (-1.0, 2.5), (0.3, 0.8), (0.0, 1.0)][seed % 4]
        s_lv = [(0.0, 1.0), (0.0, 24.0 / 25.0), (0.0, 23.976 / 24.0), (-0.5, 1.25), (0.0, 1.0)][seed % 5]
        seg = np.maximum(1, rng.geometric(1.0 / 60.0, size=R // 20 + 16))
        rb = np.repeat(rng.rand(seg.size) < 0.45, seg)[:R]
        rb = np.concatenate([rb, np.zeros(R - rb.size, bool)])
        shift = int(rng.randint(-min(w or 3000, 3000), min(w or 3000, 3000) + 1))
        idx = np.arange(S) + shift
        sb = np.zeros(S, bool)
        ok = (idx >= 0) & (idx < R)
        sb[ok] = rb[idx[ok]]
        sb ^= rng.rand(S) < 0.08
        rb[0], rb[1], sb[0], sb[1] = True, False, True, False  # both levels present
        out.append(dict(ref=np.where(rb, r_lv[1], r_lv[0]), sub=np.where(sb, s_lv[1], s_lv[0]), rb=rb, sb=sb, r_lv=r_lv,
                        s_lv=s_lv, w=w, top_k=top_k, e=e))
    return out


SMALL = _small_problems()


def _close(a, b, scale):
    """|a - b| within 4 ulps of ``scale``: the magnitude of the terms a score sums (the device's fused chain -- the solve
    records' arithmetic -- and the model's separate products round differently, and a small score can be the difference
    of large terms)."""
    return abs(a - b) <= 4 * np.spacing(scale)


def _compare(q, pr):
    """None if the device's AlignmentQuality matches the model's report of problem ``pr``, else a description."""
    rep = qm.report(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["w"], pr["top_k"], pr["e"])
    exact = pr["r_lv"] == (0.0, 1.0) and pr["s_lv"] == (0.0, 1.0)
    if q.n_lags != rep["n_lags"] or len(q.peaks) != len(rep["peaks"]):
        return ("n", q.n_lags, rep["n_lags"], len(q.peaks), len(rep["peaks"]))
    lags, sc = qm.scores(pr["rb"], pr["sb"], pr["r_lv"], pr["s_lv"], pr["w"])
    m = lambda x: 2.0 * x - 1.0
    scale = min(pr["rb"].size, pr["sb"].size) * max(abs(m(a) * m(b)) for a in pr["r_lv"] for b in pr["s_lv"])
    for (ds, do), (ms, mo) in zip(q.peaks, rep["peaks"]):
        if exact:
            if do != mo or np.float64(ds).view(np.int64) != np.float64(ms).view(np.int64):
                return ("peak", ds, do, ms, mo)
            continue
        if do != mo:
            # the model's two contenders must be within 4 ulps; the greedy sequences may part from here on
            if not _close(float(sc[np.searchsorted(lags, do)]), ms, scale):
                return ("offset", do, mo)
            break
        if not _close(ds, ms, scale):
            return ("score", ds, ms)
    for got, want in ((q.mean, rep["mean"]), (q.std, rep["std"])):
        if abs(got - want) > 1e-9 * max(abs(want), 1e-300) and not (got == want == 0.0):
            return ("moments", q.mean, rep["mean"], q.std, rep["std"])
    if (q.flags & qm.FLAT) != (rep["flags"] & qm.FLAT):
        return ("flags", q.flags, rep["flags"])
    return None


def test_device_equals_model():
    from ffsubsync_amd import quality

    bad = []
    for i, pr in enumerate(SMALL):
        q = quality.quality_batch(_device_pairs([(pr["ref"], pr["sub"])]), pr["w"], pr["top_k"], pr["e"])[0]
        why = _compare(q, pr)
        if why is not None:
            bad.append((i, pr["w"], pr["top_k"], pr["e"], why))
    assert not bad, bad[:5]
    assert sum(pr["w"] is None for pr in SMALL) >= 8
    assert sum(qm.lag_set(pr["ref"].size, pr["sub"].size, pr["w"]).size < 2 * (pr["w"] or 0) for pr in SMALL) >= 4


@pytest.mark.parametrize("algorithm", ["auto", "fft"])
def test_peak1_equals_the_solve_records_on_headline_goldens(algorithm):
    from ffsubsync_amd import batch, quality
    from workloads import synth

    gold = json.load(open(os.path.join(HERE, "golden", "headline_golden.json")))["pairs"][:128]
    specs = [synth.make_pair_spec(g["seed"]) for g in gold]
    db = synth.build_device_batch(specs)
    al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=64, algorithm=algorithm)
    try:
        _, pres = al.solve(db)
    finally:
        al.close()
    best = pres["best_cand"].astype(np.int64)
    assert (best >= 0).all()
    recs = quality.quality_batch(db.select_candidates(best), 6000, raw=True)
    bad = [(g["seed"], float(r["peak_score"][0]), int(r["peak_offset"][0]), float(p["score"]), int(p["offset"]))
           for g, r, p in zip(gold, recs, pres)
           if np.float64(r["peak_score"][0]).view(np.int64) != np.float64(p["score"]).view(np.int64)
           or int(r["peak_offset"][0]) != int(p["offset"]) or int(r["n_lags"]) != 12000]
    assert not bad, bad[:5]


def test_input_forms_and_batching_give_identical_records():
    from ffsubsync_amd import quality

    probs = [pr for pr in SMALL if pr["w"] is not None and pr["w"] >= 300][:16]
    probs = (probs * 16)[:256]
    for i, pr in enumerate(probs):  # vary the pairs
        probs[i] = dict(pr, sub=np.roll(pr["sub"], 37 * i))
    hp = [(pr["ref"], pr["sub"]) for pr in probs]
    w, k, e = 2500, 5, 120
    u1 = _device_pairs(hp)
    base = quality.quality_batch(u1, w, k, e, raw=True)
    assert base["n_peaks"].min() >= 1
    forms = {"u8": _device_pairs(hp, packed=False), "runs": u1.to_runs()}
    for name, db in forms.items():
        got = quality.quality_batch(db, w, k, e, raw=True)
        assert got.tobytes() == base.tobytes(), name
    for pif in (1, 7, 100, 256):
        quality.clear_plan_cache()
        got = quality.quality_batch(u1, w, k, e, pairs_in_flight=pif, raw=True)
        assert got.tobytes() == base.tobytes(), pif
    quality.clear_plan_cache()
    for i in range(256):
        one = quality.quality_batch(_one(u1, i), w, k, e, raw=True)
        assert one.tobytes() == base[i:i + 1].tobytes(), i


def _one(db, i):
    from ffsubsync_amd.batch import DeviceBatch

    s = slice(i, i + 1)
    return DeviceBatch(db.data, db.offs[s], db.lens[s], db.lo[s], db.hi[s], db.dtype, db.ref_dtype)


def _spec_track(spec):
    """The subtitle track of a synth pair as interval records (its ratio-1.0 candidate's samples, 10 ms each)."""
    j = spec.ratios.index(1.0)
    start = spec.cand_starts[j].astype(np.int64) * 10000
    end = spec.cand_ends[j].astype(np.int64) * 10000
    keep = end > start
    return start[keep], end[keep], np.zeros(int(keep.sum()), np.uint8)


@pytest.mark.parametrize("duration_s", [600.0, 7200.0])
def test_quality_sync_trusts_matched_and_rejects_wrong_pairs(duration_s):
    from ffsubsync_amd import quality
    from workloads import synth

    specs = [synth.make_pair_spec(seed, duration_s=duration_s) for seed in range(33)]
    refs = [synth.rasterize(sp.ref_len, sp.ref_starts, sp.ref_ends).astype(float) for sp in specs]
    tracks = [_spec_track(sp) for sp in specs[:32]]
    matched = quality.quality_sync(list(zip(refs[:32], tracks)))
    wrong = quality.quality_sync(list(zip(refs[1:33], tracks)))
    bad = [("matched", i, r.reasons, r.quality.psr, r.quality.margin) for i, r in enumerate(matched) if r.reasons]
    bad += [("wrong", i, r.quality.psr, r.quality.margin) for i, r in enumerate(wrong) if not r.reasons]
    assert not bad, bad[:5]
    for r in matched + wrong:
        assert r.quality.peaks[0] == (r.score, r.offset)


def test_errors_raise_before_any_kernel():
    from ffsubsync_amd import _native, quality
    from ffsubsync_amd.batch import DeviceBatch
    from workloads import synth

    spec = synth.make_pair_spec(3, duration_s=120.0)
    fused = synth.build_fused_batch([spec]).select_candidates([0])
    with pytest.raises(ValueError, match="multi-level float reference"):
        quality.quality_batch(fused, 6000)
    pr = SMALL[4]
    db = _device_pairs([(pr["ref"], pr["sub"])])
    for kw in (dict(top_k=0), dict(top_k=9), dict(exclusion_samples=0)):
        with pytest.raises(ValueError):
            quality.quality_batch(db, 300, **kw)
    empty = DeviceBatch(db.data, db.offs, np.array([[0, db.lens[0, 1]]]), db.lo, db.hi, db.dtype)
    with pytest.raises(ValueError, match="empty speech data"):
        quality.quality_batch(empty, 300)
    # the C entry point's own checks (FFS_E_INVALID / FFS_E_EMPTY) run before any launch as well
    plan = _native.QualityPlan(1, 1024, 4096)
    torch = _native.require_gpu()
    out = torch.zeros(160, dtype=torch.uint8, device="cuda")
    ptr = np.array([db.data.data_ptr()], dtype=np.uint64)
    args = lambda rl, sl: (ptr, [rl], [0.0], [1.0], ptr, [sl], [0.0], [1.0])
    try:
        for top_k, e, code in ((0, 300, -1), (9, 300, -1), (3, 0, -1)):
            with pytest.raises(_native.NativeError) as err:
                plan.report(*args(100, 100), 300, top_k, e, out)
            assert err.value.code == code
        with pytest.raises(_native.NativeError) as err:
            plan.report(*args(0, 100), 300, 3, 300, out)
        assert err.value.code == -5
        torch.cuda.synchronize()
        assert int(out.sum()) == 0
    finally:
        plan.close()
