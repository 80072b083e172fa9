"""bench.py --dump-outputs: the records the timed path returned in its last step, written as float arrays by which two
builds can be compared output for output.  The writer is checked on the host; the GPU test runs bench.py itself and
checks its files against a direct solve of the same seeded pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from ffsubsync_amd import _native  # noqa: E402


def _records(n, n_cand=7, seed=5):
    rng = np.random.RandomState(seed)
    pres = np.zeros(n, _native.PAIR_RESULT_DTYPE)
    pres["score"] = rng.rand(n) * 1e5
    pres["offset"] = rng.randint(-6000, 6001, n)
    pres["best_cand"] = rng.randint(0, n_cand, n)
    pres["flags"] = rng.randint(0, 4, n)
    cres = np.zeros((n, n_cand), _native.CAND_RESULT_DTYPE)
    cres["score"] = rng.rand(n, n_cand) * 1e5
    cres["offset"] = rng.randint(-6000, 6001, (n, n_cand))
    cres["score_f32"] = cres["score"].astype(np.float32)
    cres["flags"] = rng.randint(0, 4, (n, n_cand))
    return pres, cres


def _load(d):
    return {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_field_of_every_record(tmp_path):
    """The default headline batch (8192 pairs x 7 candidates) is written whole: every field of both record types, one
    row per pair in batch order, integers exact in float64, score_f32 as float32."""
    n = 8192
    seeds = list(range(100, 100 + n))
    pres, cres = _records(n)
    out = str(tmp_path / "out")
    assert bench.dump_outputs(out, seeds, pres, cres) == n
    got = _load(out)
    assert set(got) == ({"pair_seed"} | {"pair_" + f for f in pres.dtype.names} | {"cand_" + f for f in cres.dtype.names})
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["cand_score_f32"].dtype == np.float32 and got["cand_score"].dtype == np.float64
    assert np.array_equal(got["pair_seed"], seeds)
    for f in pres.dtype.names:
        assert got["pair_" + f].shape == (n,) and np.array_equal(got["pair_" + f], pres[f]), f
    for f in cres.dtype.names:
        assert got["cand_" + f].shape == (n, 7) and np.array_equal(got["cand_" + f], cres[f]), f
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= bench.DUMP_LIMIT


def test_dump_above_the_limit_keeps_the_same_sample_of_whole_records(tmp_path):
    n, limit = 5000, 200_000
    seeds = list(range(n))
    pres, cres = _records(n)
    dumps = []
    for name in ("a", "b"):
        d = str(tmp_path / name)
        kept = bench.dump_outputs(d, seeds, pres, cres, limit=limit)
        assert 0 < kept < n
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= limit
        dumps.append(_load(d))
    a, b = dumps
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["pair_seed"].astype(np.int64)  # seed i is row i here
    assert np.all(np.diff(rows) > 0)
    for f in pres.dtype.names:
        assert np.array_equal(a["pair_" + f], pres[f][rows]), f
    for f in cres.dtype.names:
        assert np.array_equal(a["cand_" + f], cres[f][rows]), f


@pytest.mark.gpu
def test_bench_dumps_what_its_timed_steps_computed(tmp_path):
    """bench.py --steps 3 --dump-outputs DIR: the line reports the three timed steps and their ms_per_step, and DIR holds
    exactly the records a direct solve of the same seeded pairs returns."""
    import torch

    from ffsubsync_amd import batch
    from workloads import synth

    assert torch.cuda.is_available()
    n = 64
    out = str(tmp_path / "dump")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", str(n), "--steps", "3", "--warmup", "1",
                          "--pairs-in-flight", "64", "--algorithm", "auto", "--full", "--skip-secondary", "--cpu-pairs", "0",
                          "--dump-outputs", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["offset_match"]["pairs_matching_reference_golden"] == "%d/%d" % (n, n)
    got = _load(out)
    assert np.array_equal(got["pair_seed"], np.arange(n))
    db = synth.build_device_batch([synth.make_pair_spec(s) for s in range(n)], packed=True)
    al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=64, algorithm="auto")
    cres, pres = al.solve(db)
    al.close()
    for f in pres.dtype.names:
        assert np.array_equal(got["pair_" + f], pres[f].astype(np.float64)), f
    for f in cres.dtype.names:
        assert np.array_equal(got["cand_" + f], cres[f].astype(got["cand_" + f].dtype)), f


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_what_a_full_run_dumps(tmp_path):
    """bench.py without --full: the same timed steps on the same pairs as a --full run -- identical dumped records, the
    headline fields of the line -- and none of the legs, tables or checks that --full adds."""
    import torch

    assert torch.cuda.is_available()
    n = 64
    lines, dumps = {}, {}
    for mode in ("plain", "full"):
        out = str(tmp_path / mode)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--pairs", str(n), "--steps", "3", "--warmup", "1",
               "--pairs-in-flight", "64", "--dump-outputs", out] + (["--full", "--skip-secondary", "--cpu-pairs", "0"]
                                                                      if mode == "full" else [])
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (mode, run.stdout[-2000:], run.stderr[-3000:])
        lines[mode] = json.loads(run.stdout.strip().splitlines()[-1])
        dumps[mode] = _load(out)
    plain, full = lines["plain"], lines["full"]
    assert plain["full"] is False and full["full"] is True
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "scaling"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"] == full["config"]
    assert plain["offset_match"] == {} and plain["roofline"] is None and "kernels_us_per_pair" not in plain
    assert "cpu_baseline" not in plain and plain["detail"] == {}
    assert full["offset_match"]["pairs_matching_reference_golden"] == "%d/%d" % (n, n) and full["roofline"] is not None
    a, b = dumps["plain"], dumps["full"]
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
