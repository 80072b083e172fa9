#!/usr/bin/env python
"""Headline benchmark: seven-ratio MaxScoreAligner(FFTAligner) solves per second on 2 h @ 100 Hz
activity vectors (BASELINE.json metric; workload = configs[2]: batches of 1024 pairs x 7 framerate
ratios, max_offset_samples = 6000, reference transform length N = 2^21).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong] [--dump-outputs DIR] [--full]

One "step" = one pass of the hot path (ffs_align_batch: pass A -> mid -> pass C -> nominees -> exact
re-evaluation -> max over ratios) over this rank's pairs -- by default eight 1024-pair batches
(`--pairs 8192`, seeds 0..8191, ~0.13 s on one MI355X, so that 20 steps time > 2 s) --, inputs already
resident in HBM (bit-packed, FFS_DTYPE_U1), plus the RCCL all-gather of the 24-byte per-pair results when
N > 1.  Pairs are sharded by rank, no data exchange during solves.  `--scaling weak` (default): every
rank owns --pairs problems; `--scaling strong`: the same --pairs problems are split over the ranks
(BASELINE configs[3]).  With --gpus N > 1 and no launcher in the environment the script starts itself
under torch.distributed.run (one process per GPU).

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the headline.  `--full` adds
everything else the benchmark measures and checks, after the same timed steps: per-kernel tables and rooflines, the
reference's goldens and the generator's ground truth, configs[3] scaling, the other paths, input formats and lag
windows, the CPU baselines, the VAD and end-to-end figures.  Rank 0 prints the full record on a `# detail:` line (and
writes bench_detail.json), then -- LAST -- one compact JSON line below 4 KB: the bench contract's fields, `roofline`,
`cpu_baseline` and the scalars of the secondary legs (a reader of the output may keep only an 8 KB tail).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (MI355X_MICROARCH.md)
HBM_COPY_CEILING = 6.29e12  # measured float4-copy ceiling, same guide


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8192, help="problems per step (per GPU when weak, in total when strong)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--duration", type=float, default=7200.0, help="seconds of activity per vector")
    ap.add_argument("--pairs-in-flight", type=int, default=512)
    ap.add_argument("--streams", type=int, default=1,
                    help="HIP streams (one plan each, pairs-in-flight shared) the sub-batches of a step are spread over; "
                         "above 1 the per-kernel table and the roofline record are omitted (concurrent kernels share the chip)")
    ap.add_argument("--input-format", choices=("bits", "bytes"), default="bits",
                    help="bits = FFS_DTYPE_U1 (native), bytes = FFS_DTYPE_U8")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, measure and check everything beyond the headline (per-kernel tables, "
                         "rooflines, goldens, scaling, secondary legs, CPU baselines, VAD, end to end); a plain run only "
                         "sets up, warms up, times the steps, dumps and prints the line")
    ap.add_argument("--cpu-pairs", type=int, default=16, help="with --full: pairs timed on the CPU oracle (0 = skip)")
    ap.add_argument("--algorithm", choices=("auto", "fft", "runs"), default="auto",
                    help="auto (library default): run-boundary path for bit-packed vectors with short boundary lists, "
                         "transforms otherwise; fft: transforms only; runs: run-boundary path without the budget")
    ap.add_argument("--no-profile", action="store_true",
                    help="skip per-kernel HIP-event timing (recorded in the timed steps of every run, read with --full)")
    ap.add_argument("--no-vad", action="store_true", help="with --full: skip the VAD frame-energy sweep figures")
    ap.add_argument("--e2e-files", type=int, default=32,
                    help="with --full: files in the end-to-end PCM -> VAD -> rasterise -> align figure (0 = skip)")
    ap.add_argument("--skip-secondary", action="store_true",
                    help="with --full: the headline's own tables and checks only (used by the rocprofv3 runs)")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl",
                    help="torch.distributed backend for N > 1.  nccl (= RCCL, the default): one rank per GPU.  gloo: the "
                         "ranks may share GPUs (rank r runs on device r mod device_count) and the 24-byte records are "
                         "gathered through host memory -- exercises the sharded N > 1 path on a one-GPU box (RCCL refuses "
                         "two ranks on one device); not a scaling measurement")
    ap.add_argument("--reference-length", action="store_true",
                    help="force the reference's transform length N=2^ceil(log2(R+S)) instead of the shorter "
                         "alias-free length the lag window allows")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the records the timed path returned in its last step as "
                         "DIR/<name>.npy (float64 / float32; rank 0's pairs; at most 64 MB in all, a fixed sample of pairs "
                         "above that): for comparing two builds output for output on identical seeded inputs")
    return ap.parse_args()


def _num(x, digits=6):
    """Shorten a float for the compact line (the full precision stays in the detail record)."""
    if isinstance(x, float):
        return float("%.*g" % (digits, x))
    return x


def _pick(d, *path):
    for p in path:
        if not isinstance(d, dict) or p not in d:
            return None
        d = d[p]
    return _num(d)


COMPACT_LIMIT = 4096  # bytes: the driver keeps the last 8 KB of stdout and parses the last line


def compact_record(result, detail_path=None):
    """The LAST stdout line: the bench contract's fields, `roofline` of the dominant kernel, `cpu_baseline`, and the
    scalars of the secondary legs -- always below COMPACT_LIMIT bytes.  The full record (kernel tables, notes, every
    secondary leg) goes to `bench_detail.json` and to an earlier `# detail:` line."""
    cfg = result.get("config", {})
    out = {k: _num(result.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                            "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    if "full" in result:
        out["full"] = result["full"]
    if "error" in result:
        out["error"] = str(result["error"])[:300]
    out["config"] = {k: cfg.get(k) for k in ("workload", "algorithm", "path", "pairs_per_gpu", "pairs_in_flight", "n_fft_reference",
                                             "n_fft_device", "input_format", "parallelism", "gather_impl", "gather_fallback",
                                             "devices_used", "ranks_seen")
                     if k in cfg}
    if isinstance(out["config"].get("ranks_seen"), list) and len(out["config"]["ranks_seen"]) > 16:
        out["config"]["ranks_seen"] = out["config"]["ranks_seen"][:16]
    for k in ("workload", "input_format", "parallelism", "path", "gather_impl"):
        if isinstance(out["config"].get(k), str):
            out["config"][k] = out["config"][k][:200]
    om = result.get("offset_match", {})
    out["offset_match"] = {k: om.get(k) for k in ("pairs_matching_reference_golden", "pairs", "pairs_matching_ground_truth",
                                                  "gpu_equals_cpu_oracle_on_sample", "ambiguous_flags") if k in om}

    def slim_roofline(r):
        if not isinstance(r, dict):
            return None
        keep = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "wasted", "avg_launch_ms",
                "share_of_kernel_time", "per_launch", "peak_source", "lds_conflict_frac", "frac_of_conflict_free_rate")
        return {k: _num(r[k]) for k in keep if k in r}

    for k in ("gathered_records", "gathered_best_cand_valid"):  # N > 1: every rank's records arrived
        if k in result:
            out[k] = result[k]
    out["roofline"] = slim_roofline(result.get("roofline"))
    if result.get("roofline_hbm") is not None:
        out["roofline_hbm"] = slim_roofline(result.get("roofline_hbm"))
    if isinstance(result.get("kernels"), dict):
        out["kernels_us_per_pair"] = {k: _num(v.get("us_per_pair"), 4) for k, v in result["kernels"].items()}
    cb = result.get("cpu_baseline")
    if isinstance(cb, dict):
        out["cpu_baseline"] = {k: (_num(cb[k]) if not isinstance(cb[k], str) else cb[k][:160])
                               for k in ("value", "unit", "cores", "kind", "sample") if k in cb}
        if isinstance(cb.get("parallel"), dict) and "value" in cb["parallel"]:
            out["cpu_baseline"]["parallel"] = {"value": _num(cb["parallel"]["value"]), "cores": cb["parallel"].get("cores")}
    # the legs a reader of the headline needs next to it: the north star's transform kernels on the same pairs, the
    # reference's own transform length, the windowless solve
    out["fft_path_value"] = _pick(result, "fft_path", "value")
    out["fft_path_roofline"] = slim_roofline((result.get("fft_path") or {}).get("roofline"))
    out["reference_length_value"] = _pick(result, "reference_length", "value")
    out["windowless_value"] = _pick(result, "windowless", "value")
    out["windowless_golden"] = _pick(result, "windowless", "pairs_matching_reference_golden")
    detail = {
        "fft_path_identical_records": _pick(result, "fft_path", "identical_candidate_results"),
        "single_ratio_6000": _pick(result, "single_ratio", "max_offset_6000", "solves_per_s"),
        "single_ratio_none": _pick(result, "single_ratio", "max_offset_none", "solves_per_s"),
        "byte_inputs": _pick(result, "byte_inputs", "value"),
        "float_inputs": _pick(result, "float_inputs", "value"),
        "float_inputs_path": _pick(result, "float_inputs", "path"),
        "float_inputs_golden": _pick(result, "float_inputs", "pairs_matching_reference_golden"),
        "gss_files_per_s": _pick(result, "gss", "files_per_s"),
        "gss_all_files_equal_per_file_search": _pick(result, "gss", "all_files_equal_per_file_search"),
        "ingest_cold_pairs_per_s": _pick(result, "ingest_inclusive", "solves_per_s"),
        "ingest_warm_plan_stream_pairs_per_s": _pick(result, "ingest_inclusive", "warm_plan_stream", "solves_per_s"),
        "ingest_lists_warm_pairs_per_s": _pick(result, "ingest_inclusive", "boundary_lists", "solves_per_s"),
        "ingest_lists_resident_tracks_pairs_per_s": _pick(result, "ingest_inclusive", "boundary_lists", "resident_tracks", "solves_per_s"),
        "ingest_lists_trackset_per_batch_pairs_per_s": _pick(result, "ingest_inclusive", "boundary_lists", "trackset_built_per_batch", "solves_per_s"),
        "resident_lists_value": _pick(result, "resident_lists", "value"),
        "drop_in_ms_device_rasters": _pick(result, "drop_in", "device_rasters", "ms_per_solve_median"),
        "drop_in_ms_host_arrays": _pick(result, "drop_in", "host_float64_arrays", "ms_per_solve_median"),
        "vad_GBps": _pick(result, "vad", "roofline", "achieved"),
        "vad_frac": _pick(result, "vad", "roofline", "frac"),
        "vad_parity": _pick(result, "vad", "parity"),
        "end_to_end_files_per_s": _pick(result, "end_to_end", "files_per_s"),
        "normaliser_frac_of_8TBps": _pick(result, "normaliser", "frac_of_8TBps_per_gpu"),
    }
    ss = result.get("strong_scaling") or result.get("strong_scaling_proxy")
    if isinstance(ss, dict):
        detail["strong_proxy" if "strong_scaling_proxy" in result else "strong"] = {
            k: _num(ss[k]) for k in ("pairs_per_rank_per_step", "ms_per_step", "solves_per_s_this_gpu", "value",
                                     "efficiency_vs_headline_batch", "predicted_8_gpu_strong_solves_per_s") if k in ss}
        if isinstance(ss.get("vectors_resident_as_boundary_lists"), dict) and "ms_per_step" in ss["vectors_resident_as_boundary_lists"]:
            detail["strong_proxy_lists"] = {k: _num(v) for k, v in ss["vectors_resident_as_boundary_lists"].items()
                                            if k in ("ms_per_step", "solves_per_s_this_gpu", "predicted_8_gpu_strong_solves_per_s")}
    bd = (result.get("boundary_density") or {}).get("sweep")
    if bd:  # [boundaries per vector, auto solves/s, transforms solves/s, path initial]
        detail["boundary_density"] = [[int(s["boundaries_per_vector"]), int(s["auto_solves_per_s"]), int(s["transforms_solves_per_s"]),
                                       s["auto_path"][:1]] for s in bd]
    out["detail"] = {k: v for k, v in detail.items() if v is not None}
    if detail_path:
        out["detail_file"] = detail_path
    line = json.dumps(out, separators=(",", ":"))
    # never let the line outgrow the driver's tail: drop optional blocks, least important first
    for victim in ("detail", "kernels_us_per_pair", "fft_path_roofline", "roofline_hbm"):
        if len(line) < COMPACT_LIMIT:
            break
        out.pop(victim, None)
        line = json.dumps(out, separators=(",", ":"))
    assert len(line) < COMPACT_LIMIT, len(line)
    return line


def emit(result):
    """Full record -> bench_detail.json (+ gpurun_out/, + an earlier `# detail:` stdout line); compact record LAST."""
    full = json.dumps(result)
    written = None
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        try:
            if os.path.isdir(d):
                with open(os.path.join(d, "bench_detail.json"), "w") as f:
                    f.write(full + "\n")
                written = written or "bench_detail.json"
        except OSError:
            pass
    print("# detail: " + full, flush=True)
    print(compact_record(result, written), flush=True)


DUMP_LIMIT = 64 * 10 ** 6  # bytes: what --dump-outputs may write in all, .npy headers included


def dump_outputs(out_dir, seeds, pres, cres, limit=DUMP_LIMIT):
    """--dump-outputs: the records a caller of the timed path receives -- pres [pairs] (PAIR_RESULT_DTYPE), cres [pairs,
    candidates] (CAND_RESULT_DTYPE) -- one float array per field, as <out_dir>/<name>.npy, with the seed of every pair
    (pair_seed).  Integers go to float64, which holds them exactly.  Above `limit` bytes the same pairs are always kept:
    a sample drawn by RandomState(0), in batch order.  Returns the number of pairs written."""
    import numpy as np

    arrays = {"pair_seed": np.asarray(seeds, dtype=np.float64)}
    for f in pres.dtype.names:
        arrays["pair_" + f] = pres[f].astype(np.float64)
    for f in cres.dtype.names:
        arrays["cand_" + f] = cres[f].astype(np.float32 if cres.dtype[f] == np.float32 else np.float64)
    n = len(seeds)
    per_pair = sum(a.nbytes for a in arrays.values()) / max(1, n)
    room = limit - 1024 * len(arrays)  # per file, room for its .npy header (128 bytes for arrays of these shapes)
    if n * per_pair > room:
        keep = np.sort(np.random.RandomState(0).choice(n, int(room // per_pair), replace=False))
        arrays = {k: a[keep] for k, a in arrays.items()}
        n = keep.size
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(a))
    return n


def fail_line(args, message, world=None):
    """A bench run that cannot measure what was asked for says so in the JSON line (and exits non-zero) instead of
    measuring something else."""
    print(json.dumps({"metric": "alignments/sec (2 h@100 Hz, 7 framerate ratios)", "value": None, "unit": "7-ratio solves/s",
                      "n_gpus": world or args.gpus, "steps": args.steps, "warmup": args.warmup, "error": message}), flush=True)
    raise SystemExit(2)


def self_launch(args):
    """--gpus N > 1 without a launcher: run this script under torch.distributed.run, one process per GPU."""
    import torch

    if args.backend == "nccl" and torch.cuda.device_count() < args.gpus:
        fail_line(args, "--gpus %d asked for, %d HIP device(s) visible" % (args.gpus, torch.cuda.device_count()))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.call(cmd, env=env))


def vad_figures(torch, _native, minutes=90.0, iters=20):
    """Second kernel of the hot path: frame-energy VAD sweep over one 90-minute 48 kHz s16le file
    resident in HBM (BASELINE config 5 shape: 259.2 M samples, 518 MB).  Algorithmic bytes =
    2*n_samples + 4*n_frames."""
    from oracle import vad_oracle as vo

    frame = 480
    n_frames = int(minutes * 60 * 100)
    n = n_frames * frame
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    seg = torch.randint(0, 2, (n_frames // 50 + 1,), generator=g, device="cuda").repeat_interleave(50)[:n_frames].bool()
    sigma = torch.where(seg, 3000.0, 30.0).repeat_interleave(frame)
    pcm = (torch.randn(n, generator=g, device="cuda") * sigma).round().clamp(-32768, 32767).to(torch.int16)
    del sigma
    labels = _native.vad_energy(pcm, frame, 50.0, 0.0)
    ok = bool(torch.equal(labels > 0.5, seg))
    # bit-exact vs the CPU oracle on the first 100 s chunk (the reference's buffer size)
    head = pcm[: frame * 10000].cpu().numpy()
    ok_oracle = bool((labels[:10000].cpu().numpy() == vo.detect_fast(head)).all())
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _native.vad_energy(pcm, frame, 50.0, 0.0)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        _native.vad_energy(pcm, frame, 50.0, 0.0)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / iters
    bytes_ = 2 * n + 4 * n_frames
    # the same sweep with bit-packed labels (ffs_vad_energy_bits: what the end-to-end path uses)
    words = torch.zeros((n_frames + 31) // 32, dtype=torch.int32, device="cuda")
    _native.vad_energy_bits(pcm, frame, 50.0, out=words)
    bits_ok = bool(torch.equal(_native.unpack_bits(words, n_frames), (labels > 0.5).to(torch.uint8)))
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(iters):
        _native.vad_energy_bits(pcm, frame, 50.0, out=words)
    ev1.record()
    torch.cuda.synchronize()
    ms_bits = ev0.elapsed_time(ev1) / iters
    t1 = time.perf_counter()
    cpu_n = frame * 10000 * 3
    vo.chunked_detect(pcm[:cpu_n].cpu().numpy())
    cpu_s = time.perf_counter() - t1
    lo, hi = _native.speech_bounds(labels)
    # the rocprofv3 record of the same kernel on the same workload (profiles/secondary_kernels.py under --kernel-trace and
    # --pmc FETCH_SIZE / WRITE_SIZE; refreshed by profiles/refresh_all.sh): duration, HBM bytes measured vs algorithmic
    rocprof = None
    spath = os.path.join(ROOT, "profiles", "r05_secondary_kernels.json")
    if not os.path.exists(spath):
        spath = os.path.join(ROOT, "profiles", "r04_secondary_kernels.json")
    if os.path.exists(spath):
        sj = json.load(open(spath))
        rocprof = {k: {kk: v[kk] for kk in ("avg_us", "achieved_GBps", "frac_of_8TBps", "pmc_hbm_bytes_per_launch", "pmc_over_algorithmic")
                       if kk in v} for k, v in sj.items() if k.startswith("k_vad_energy")}
        rocprof["source"] = "profiles/%s (rocprofv3 --kernel-trace --stats + --pmc FETCH_SIZE / WRITE_SIZE)" % os.path.basename(spath)
    return {
        "roofline": {"kernel": "k_vad_energy", "bound": "hbm", "achieved": bytes_ / (ms * 1e-3) / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                     "frac": bytes_ / (ms * 1e-3) / HBM_PEAK, "bytes_per_launch": bytes_, "avg_launch_ms": ms,
                     "timed_with": "torch.cuda events on the launch stream around %d launches" % iters, "rocprofv3": rocprof},
        "workload": "one %.0f-min 48 kHz s16le file in HBM (%d samples, %d frames)" % (minutes, n, n_frames),
        "kernel": "k_vad_energy",
        "ms_per_file": ms,
        "audio_hours_per_s": minutes / 60.0 / (ms * 1e-3),
        "achieved_GBps": bytes_ / (ms * 1e-3) / 1e9,
        "frac_of_8TBps": bytes_ / (ms * 1e-3) / HBM_PEAK,
        "bit_packed_labels": {"entry_point": "ffs_vad_energy_bits", "ms_per_file": ms_bits,
                              "achieved_GBps": (2 * n + n_frames / 8) / (ms_bits * 1e-3) / 1e9,
                              "frac_of_8TBps": (2 * n + n_frames / 8) / (ms_bits * 1e-3) / HBM_PEAK,
                              "equal_to_fp32_labels": bits_ok},
        "read_only_ceiling": "6.2-6.9 TB/s on this part (profiles/read_ceiling.hip, profiles/r03_ab_experiments.json)",
        "labels_match_generator": ok,
        "labels_match_cpu_oracle_first_chunk": ok_oracle,
        "speech_bounds": [lo, hi],
        "cpu_oracle_audio_hours_per_s": (cpu_n / 48000.0 / 3600.0) / cpu_s,
        "parity": "unpinned (auditok 0.1.5 absent: oracle/vad_oracle.py restates its published energy rule)",
    }


def e2e_figures(torch, _native, n_files, minutes=90.0, cpu_files=4):
    """BASELINE configs[4] at one GPU's share (256 files / 8 GPUs = 32 files x 90 min): per file, 48 kHz s16le PCM
    streamed from PINNED HOST memory in the reference's 100 s buffers (H2D on a copy stream overlapped with
    the frame-energy sweep, ``detect_pinned_stream``) -> 100 Hz activity vector (stays in HBM, bit-packed);
    its subtitle file -> seven rasterised framerate-ratio candidates (from interval lists, bit-packed);
    then one batched MaxScoreAligner solve over all files.  Ground truth: every file's subtitles were
    stretched by one of the seven ratios and shifted by a known offset.  The PCIe rate is measured, not
    estimated; the same files' first `cpu_files` go through the CPU oracles for the wall-clock next to it."""
    import numpy as np

    from ffsubsync_amd import batch
    from ffsubsync_amd.constants import candidate_ratios
    from ffsubsync_amd.speech_transformers import detect_pinned_stream, frames_per_window
    from ffsubsync_amd.subtitle_raster import rasterize_candidates
    from workloads import synth

    ratios = candidate_ratios()
    frame, n_frames = 480, int(minutes * 60 * 100)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    files, truth = [], []
    for f in range(n_files):
        rng = np.random.RandomState(7000 + f)
        s_us, e_us, meta = synth.make_subtitle_records(7000 + f, duration_s=minutes * 60 * 0.9)
        idx, shift = int(rng.randint(7)), int(rng.randint(-4000, 4000))
        act = _native.rasterize_subtitles(s_us, e_us, meta, ratios[idx], 100, 0)  # where people speak
        speech = torch.zeros(n_frames, dtype=torch.bool, device="cuda")
        lo, hi = max(shift, 0), min(n_frames, shift + act.numel())
        speech[lo:hi] = act[lo - shift: hi - shift] != 0
        sigma = torch.where(speech, 3000.0, 30.0).repeat_interleave(frame)
        pcm = (torch.randn(n_frames * frame, generator=g, device="cuda") * sigma).round().clamp(-32768, 32767).to(torch.int16)
        del sigma
        host = torch.empty(pcm.numel(), dtype=torch.int16).pin_memory()
        host.copy_(pcm)
        del pcm
        files.append((host, (s_us, e_us, meta)))
        truth.append((idx, shift))
    torch.cuda.synchronize()
    chunk = frames_per_window(100, 48000) * 10000
    staging = ([torch.empty(chunk, dtype=torch.int16, device="cuda") for _ in range(2)], torch.cuda.Stream())

    def run():
        pairs = []
        t_v = time.perf_counter()
        for host, (s_us, e_us, meta) in files:
            ref = detect_pinned_stream(host, 100, 48000, 0.0, staging=staging, packed=True)  # bit-packed, in HBM
            pairs.append((ref, rasterize_candidates(s_us, e_us, meta, ratios)))
        torch.cuda.synchronize()
        t_v = time.perf_counter() - t_v
        db = batch.pack_pairs(pairs)
        al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=min(128, n_files))
        _, pres = al.solve(db)
        al.plan.close()
        return pres, t_v

    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pres, t_vad = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = sum(int(pres[i]["best_cand"]) == truth[i][0] and abs(int(pres[i]["offset"]) - truth[i][1]) <= 2
             for i in range(n_files))
    pcm_bytes = 2 * n_frames * frame
    out = {
        "workload": "%d files x %.0f min: 48 kHz PCM streamed from pinned host memory -> VAD -> 7 rasterised "
                    "candidates -> batched solve (one GPU's share of configs[4])" % (n_files, minutes),
        "files_per_s": n_files / dt,
        "ms_per_file": 1e3 * dt / n_files,
        "pcie_GBps_achieved_during_vad": n_files * pcm_bytes / t_vad / 1e9,
        "vad_share_of_wall": t_vad / dt,
        "recovered_ratio_and_offset": "%d/%d" % (ok, n_files),
    }
    if cpu_files > 0:
        from oracle import aligners_oracle as orc
        from oracle import raster_oracle as ro
        from oracle import vad_oracle as vo

        t1 = time.perf_counter()
        agree, detail = True, []
        for i in range(min(cpu_files, n_files)):
            host, (s_us, e_us, meta) = files[i]
            lab = vo.chunked_detect(host.numpy())
            cands = [ro.rasterize(s_us, e_us, meta, r, 100, 0) for r in ratios]  # amplitude min(1/r, 1) included
            (sc, off), idx = orc.max_score_align(lab, cands, 6000)
            agree &= (idx == int(pres[i]["best_cand"]) and off == int(pres[i]["offset"])
                      and abs(sc - pres[i]["score"]) <= 1e-5 * abs(sc))
            detail.append({"cpu": [int(idx), int(off), float(sc)],
                           "gpu": [int(pres[i]["best_cand"]), int(pres[i]["offset"]), float(pres[i]["score"])]})
        out["cpu_vs_gpu_sample"] = detail
        cpu_s = (time.perf_counter() - t1) / min(cpu_files, n_files)
        out["cpu_oracle_s_per_file_1core"] = cpu_s
        out["gpu_equals_cpu_oracle_on_sample"] = bool(agree)
        out["speedup_vs_1core"] = cpu_s / (dt / n_files)
    return out


def drop_in_figures(torch, specs, n=12):
    """One seven-ratio 2 h solve at a time THROUGH THE DROP-IN CLASSES (the seam ffsubsync.py:230-235 calls):
    MaxScoreAligner(FFTAligner, None, 100, 60).fit_transform(ref, candidates) -- (i) from host float64 arrays, what an
    unpatched pipeline hands over; (ii) from the device rasters that install(device_rasters=True) leaves in HBM
    (DeviceSubtitleSpeechTransformer outputs + the cached device copy of the reference vector): bit-packed samples AND,
    since round 5, their boundary lists with host-known length bounds -- the solve extracts nothing and does not wait
    for the device before it returns."""
    import numpy as np

    from ffsubsync_amd import _native
    from ffsubsync_amd.aligners import FFTAligner, MaxScoreAligner
    from ffsubsync_amd.subtitle_raster import DeviceRaster
    from workloads import synth

    out = {}
    host = [synth.pair_float_arrays(sp) for sp in specs[:n]]
    dev = []
    for ref, cands in host:
        dev.append((DeviceRaster.from_host(ref), [DeviceRaster.from_host(c) for c in cands]))
    answers = {}
    for label, problems in (("host_float64_arrays", host), ("device_rasters", dev)):
        for ref, cands in problems[:2]:
            MaxScoreAligner(FFTAligner, None, 100, 60).fit_transform(ref, list(cands))
        torch.cuda.synchronize()
        ts, got = [], []
        for ref, cands in problems:
            cands = list(cands)
            t0 = time.perf_counter()
            (score, offset), winner = MaxScoreAligner(FFTAligner, None, 100, 60).fit_transform(ref, cands)
            ts.append(time.perf_counter() - t0)
            got.append((float(score), int(offset), [i for i, c in enumerate(cands) if c is winner][0]))
        answers[label] = got
        out[label] = {"ms_per_solve_median": 1e3 * float(np.median(ts)), "ms_per_solve_min": 1e3 * min(ts),
                      "solves_per_s_one_at_a_time": len(ts) / sum(ts)}
    out["same_answers"] = answers["host_float64_arrays"] == answers["device_rasters"]
    # the same host float64 arrays, all problems in ONE call (aligners.solve_host_batch: threaded level detection + bit
    # packing, one upload, one ffs_align_batch)
    from ffsubsync_amd.aligners import solve_host_batch

    solve_host_batch(host[:2], 6000, 6000)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, pres_h = solve_host_batch(host, 6000, 6000)
    dt = time.perf_counter() - t0
    out["host_batch"] = {
        "ms_per_solve": 1e3 * dt / len(host), "solves_per_s": len(host) / dt,
        "same_answers": [(float(r["score"]), int(r["offset"]), int(r["best_cand"])) for r in pres_h] == answers["host_float64_arrays"],
        "what": "%d problems' float64 arrays in one solve_host_batch call" % len(host)}
    out["recovered_ratio"] = "%d/%d" % (sum(a[2] == sp.true_ratio_index for a, sp in zip(answers["device_rasters"], specs)), n)
    out["what"] = ("MaxScoreAligner(FFTAligner, None, 100, 60).fit_transform, one 2 h x 7-ratio problem per call, %d problems; "
                   "the unmodified reference needs ~2.9 s for the same call in the build container "
                   "(profiles/r04_cpu_reference_baseline.json)" % n)
    return out


def gss_figures(torch, _native, specs, n_files=256):
    """Batched golden-section search over the framerate ratio (MaxScoreAligner.fit_gss, aligners.py:111-129, for many
    files at once): every one of the 17 steps is ONE batched rasterisation (each file's subtitle track at that file's
    current ratio) + ONE batched solve, plan and reference vectors held across the steps.  Files: the benchmark pairs --
    reference vector bit-packed in HBM, subtitle file = the pair's track in its own clock (the ratio-1.0 candidate)."""
    import numpy as np

    from ffsubsync_amd import batch
    from ffsubsync_amd.batch_gss import fit_gss_batch
    from ffsubsync_amd.subtitle_raster import DeviceRaster

    specs = specs[:n_files]
    n = len(specs)
    refs_t = batch.TrackSet([(sp.ref_starts * 10000, sp.ref_ends * 10000, None) for sp in specs])
    data, offs, lens = refs_t.rasterize(np.arange(n), np.ones(n))
    # (the rasteriser sizes a vector by its last interval; the aligner only needs the activity, not the silent tail)
    refs = [DeviceRaster(data[int(o): int(o) + (int(l) + 31) // 32 * 4].view(torch.int32), 0.0, 1.0, int(l)) for o, l in zip(offs, lens)]
    i1 = [i for i, r in enumerate(specs[0].ratios) if r == 1.0][0]
    recs = [(sp.cand_starts[i1] * 10000, sp.cand_ends[i1] * 10000, None) for sp in specs]
    fit_gss_batch(refs, recs, max_offset_samples=6000)  # warm-up at the timed size: plan, staging buffers, allocator pools
    torch.cuda.synchronize()
    stats = {}
    t0 = time.perf_counter()
    got = fit_gss_batch(refs, recs, max_offset_samples=6000, stats=stats)
    el = time.perf_counter() - t0
    # the search maximises a score that is not unimodal in the ratio (as in the reference): count how many files end
    # within 1e-3 of the ratio their subtitles were really stretched by, and check one file against the scalar search
    near = sum(abs(ratio - sp.ratios[sp.true_ratio_index]) < 1e-3 for (_, ratio), sp in zip(got, specs))
    from ffsubsync_amd.aligners import FFTAligner, MaxScoreAligner
    from ffsubsync_amd.subtitle_raster import rasterize_candidates

    class Pipe:
        def __init__(self, r):
            self.r = r

        def fit_transform(self, *_):
            return rasterize_candidates(recs[0][0], recs[0][1], None, [self.r])[0]

    msa = MaxScoreAligner(FFTAligner(max_offset_samples=6000))
    msa.fit(refs[0], [lambda r: Pipe(r)])
    (s1, o1), pipe = msa.transform()
    # every file against the per-file search (one rasterisation and one solve per file and step through the drop-in's
    # solve_pairs: the path fit_gss_batch falls back to): same recorded (score, offset, ratio) -- VERDICT r4 item 9
    from ffsubsync_amd.batch_gss import _fit_gss_batch_per_file

    n_chk = min(n, int(os.environ.get("FFS_BENCH_GSS_CHECK", "256")))
    per_file = _fit_gss_batch_per_file(refs[:n_chk], recs[:n_chk], max_offset_samples=6000)
    same = sum(int(repr(a[1]) == repr(b[1]) and int(a[0][1]) == int(b[0][1]) and float(a[0][0]) == float(b[0][0]))
               for a, b in zip(got[:n_chk], per_file))
    return {
        "all_files_equal_per_file_search": "%d/%d" % (same, n_chk),
        "lists": bool(stats.get("lists")),
        "what": "%d files x 2 h: fit_gss_batch(max_offset_samples=6000), golden-section search on [0.9, 1.1] to 1e-4; a warm "
                "service (the same search has run once before at this size: plan, staging buffers and allocator pools exist); "
                "per step one ffs_rasterize_batch_runs (device-resident subtitle tables) + one ffs_align_batch_runs on boundary "
                "lists + the read-back of the scores" % n,
        "files_per_s": n / el, "ms_per_file": 1e3 * el / n, "steps": stats.get("steps"), "ms_per_step": 1e3 * el / max(1, stats.get("steps", 1)),
        "evaluations_per_s": n * stats.get("steps", 0) / el,
        "files_ending_within_1e-3_of_the_true_ratio": "%d/%d" % (near, n),
        "file_0_equals_scalar_search_through_the_drop_in": bool(
            (repr(pipe.r), int(o1), float(s1)) == (repr(got[0][1]), int(got[0][0][1]), float(got[0][0][0]))),
    }


def ingest_inclusive_figures(torch, _native, n_pairs=256, minutes=120.0):
    """Solves/s when the timed region starts from INTERVAL LISTS: per pair, the subtitle track is rasterised at the
    seven framerate ratios on the device (ffs_rasterize_subtitles_bits), the reference activity likewise, the vectors are
    packed into one batch buffer and solved.  (The headline `value` starts from bit-packed vectors resident in HBM.)"""
    import numpy as np

    from ffsubsync_amd import batch
    from ffsubsync_amd.constants import candidate_ratios
    from ffsubsync_amd.subtitle_raster import rasterize_candidates
    from workloads import synth

    ratios = candidate_ratios()
    recs, truth = [], []
    for f in range(n_pairs):
        rng = np.random.RandomState(9000 + f)
        s_us, e_us, meta = synth.make_subtitle_records(9000 + f, duration_s=minutes * 60 * 0.95)
        idx, shift_us = int(rng.randint(7)), int(rng.randint(-40, 40)) * 1_000_000
        # the reference: the same track as the audio would show it (stretched by the true ratio, shifted)
        r_s = np.maximum(np.rint(s_us * ratios[idx]).astype(np.int64) + shift_us, 0)
        r_e = np.maximum(np.rint(e_us * ratios[idx]).astype(np.int64) + shift_us, 0)
        recs.append(((r_s, r_e, meta), (s_us, e_us, meta)))
        truth.append((idx, shift_us // 10_000))

    def solve(db):
        al = batch.BatchAligner(db.required_fft_length(6000), 7, 6000, pairs_in_flight=min(256, n_pairs))
        _, pres = al.solve(db)
        al.close()
        return pres

    def per_vector():
        pairs = []
        for (r_s, r_e, r_m), (s_us, e_us, meta) in recs:
            ref = rasterize_candidates(r_s, r_e, r_m, [1.0])[0]
            pairs.append((ref, rasterize_candidates(s_us, e_us, meta, ratios)))
        return solve(batch.pack_pairs(pairs))

    def one_call():
        return solve(batch.pairs_from_intervals(recs, ratios))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pres = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = sum(int(pres[i]["best_cand"]) == truth[i][0] and abs(int(pres[i]["offset"]) - truth[i][1]) <= 2
                 for i in range(n_pairs))
        return pres, {"solves_per_s": n_pairs / dt, "ms_per_pair": 1e3 * dt / n_pairs,
                      "recovered_ratio_and_offset": "%d/%d" % (ok, n_pairs)}

    pres_a, fig_a = timed(per_vector)
    pres_b, fig_b = timed(one_call)

    # A service keeps its plan: the same work with the aligner created once, as a stream of batches -- the interval
    # tables of batch k+1 are prepared, uploaded and rasterised while batch k is being solved (the calls are asynchronous;
    # the TrackSet of a batch is built inside the timed region, like everything else that starts from the interval lists).
    def warm_stream(n_batches=8):
        al = batch.BatchAligner(batch.pairs_from_intervals(recs, ratios).required_fft_length(6000), 7, 6000,
                                pairs_in_flight=min(256, n_pairs))
        outs = [(torch.empty(n_pairs * 7 * 24, dtype=torch.uint8, device="cuda"),
                 torch.empty(n_pairs * 24, dtype=torch.uint8, device="cuda")) for _ in range(2)]
        keep = []

        def run(k):
            db = batch.pairs_from_intervals(recs, ratios)
            keep.append(db)  # alive until its solve has run
            al.solve_async(db, 0, n_pairs, outs[k % 2][0], outs[k % 2][1])
            if len(keep) > 2:
                keep.pop(0)

        run(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n_batches):
            run(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        pres = outs[(n_batches - 1) % 2][1].cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:n_pairs].copy()
        al.close()
        return pres, n_batches * n_pairs / dt

    pres_w, rate_w = warm_stream()

    # Round 5: the same stream without any bitmap -- interval lists -> BOUNDARY lists (ffs_rasterize_batch_runs) -> solve
    # (ffs_align_batch_runs with the lists' host-known bounds: no pass over a vector, nothing read back per batch).
    def lists_stream(n_batches=16, tables="per_batch"):
        al = batch.BatchAligner(batch.pairs_from_intervals(recs, ratios).required_fft_length(6000), 7, 6000,
                                pairs_in_flight=min(256, n_pairs))
        outs = [(torch.empty(n_pairs * 7 * 24, dtype=torch.uint8, device="cuda"),
                 torch.empty(n_pairs * 24, dtype=torch.uint8, device="cuda")) for _ in range(2)]
        keep = []
        tracks = [t for rec in recs for t in rec]
        track_of = (np.tile(np.array([0] + [1] * len(ratios)), (n_pairs, 1)) + 2 * np.arange(n_pairs)[:, None]).ravel()
        ratio = np.tile(np.array([1.0] + list(ratios)), (n_pairs, 1)).ravel()
        hi = np.minimum(1.0 / ratio, 1.0).reshape(n_pairs, 8)
        held = None if tables == "per_batch" else batch.TrackSet(tracks)
        if tables == "device":
            held.to_device()
        # (tables == "host": pageable tables, staged by the entry point.  TrackSet.pin() -- uploads straight from pinned
        # memory -- is faster per call when calls are synchronised, 0.31 vs 0.43 ms, but slower in a stream of unsynchronised
        # batches, 0.92 vs 0.52 ms of host time per call: profiles/ingest_profile.py)

        arenas = [None, None]  # (per_batch: the host tables of batch k - 2 are filled again -- its call has long returned)

        def run(k):
            if held is not None:
                ts = held
            else:
                ts = arenas[k % 2] = batch.TrackSet(tracks, arena=arenas[k % 2])
            data, offs, lens, bounds = ts.rasterize_runs(track_of, ratio)
            db = batch.DeviceBatch(data, offs.reshape(n_pairs, 8), lens.reshape(n_pairs, 8), np.zeros_like(hi), hi,
                                   _native.FFS_DTYPE_RUNS, None, bounds.reshape(n_pairs, 8))
            keep.append(db)
            al.solve_async(db, 0, n_pairs, outs[k % 2][0], outs[k % 2][1])
            if len(keep) > 2:
                keep.pop(0)

        for k in range(8):  # warm: staging buffers, descriptor storage and the allocator's pools reach their final size
            run(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n_batches):
            run(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        pres = outs[(n_batches - 1) % 2][1].cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:n_pairs].copy()
        al.close()
        return pres, n_batches * n_pairs / dt

    try:
        pres_l, rate_l = lists_stream(tables="per_batch")
        pres_h, rate_h = lists_stream(tables="host")
        pres_r, rate_r = lists_stream(tables="device")
        lists_fig = {
            "what": "the warm stream with boundary lists instead of bitmaps: batches of %d pairs back to back (16 timed after 8 "
                    "warm ones), per batch ffs_rasterize_batch_runs -> ffs_align_batch_runs with host-known list bounds (no "
                    "extraction pass, nothing read back).  solves_per_s: the subtitle tables held in one host TrackSet and "
                    "uploaded with every batch" % n_pairs,
            "solves_per_s": rate_h, "same_results": bool(np.array_equal(pres_h, pres_b)),
            "trackset_built_per_batch": {
                "what": "the TrackSet itself (numpy concatenation of the 2 x %d per-track arrays) built inside the timed region, "
                        "as warm_plan_stream does" % n_pairs,
                "solves_per_s": rate_l, "same_results": bool(np.array_equal(pres_l, pres_b))},
            "resident_tracks": {
                "what": "the subtitle tables uploaded once (TrackSet.to_device: the same files against many references, the "
                        "steps of a search): per batch only the 32-byte-per-vector table travels",
                "solves_per_s": rate_r, "same_results": bool(np.array_equal(pres_r, pres_b))}}
    except Exception as exc:
        lists_fig = {"error": repr(exc)[:300]}
    out = {"what": "%d pairs from interval lists -> rasters of the reference track and of the subtitle track at the seven "
                   "ratios -> one batch buffer -> one batched solve; includes plan creation.  One ffs_rasterize_batch_bits "
                   "call for the whole batch (interval arithmetic on the device, written straight into the batch buffer)"
                   % n_pairs}
    out.update(fig_b)
    out["same_results_as_per_vector_calls"] = bool(np.array_equal(pres_a, pres_b))
    out["warm_plan_stream"] = {
        "what": "8 batches of %d pairs back to back on one aligner created beforehand (plan, staging buffers and boundary-list "
                "workspace warm): interval lists -> rasters -> solve, results of the last batch checked" % n_pairs,
        "solves_per_s": rate_w, "same_results": bool(np.array_equal(pres_w, pres_b))}
    out["boundary_lists"] = lists_fig
    out["per_vector_calls"] = dict(fig_a, what="8 ffs_rasterize_subtitles_bits calls per pair from a Python loop (host interval "
                                                "arithmetic) + pack_pairs: the round-3 figure before the batched entry point")
    return out


def strong_leg(torch, _native, batch, synth, args, rank, world, dist, comm, host_coll, n_dev, headline_value, coll_dev,
               total_pairs=1024, proxy_world=8, steps=100, warmup=5):
    """Strong scaling of BASELINE configs[3] (1024 pairs in total).  world > 1: every rank solves its shard and joins the
    gather, timed like the headline (barrier + synchronize, max over ranks).  world == 1: the share a rank would own at
    `proxy_world` GPUs, with the gather on a one-rank communicator."""
    import numpy as np

    w_eff = world if world > 1 else proxy_world
    per = (total_pairs + w_eff - 1) // w_eff
    lo, hi = batch.shard_bounds(total_pairs, rank if world > 1 else 0, w_eff)
    n_local = hi - lo
    specs = [synth.make_pair_spec(s, duration_s=args.duration) for s in range(lo, hi)]
    db = synth.build_device_batch(specs)
    in_flight = batch.pairs_in_flight_for(n_local)
    al = batch.BatchAligner(n_dev, 7, 6000, pairs_in_flight=in_flight)
    cand_out = torch.empty(max(n_local, 1) * 7 * 24, dtype=torch.uint8, device="cuda")
    pair_out = torch.zeros(per * 24, dtype=torch.uint8, device="cuda")
    gathered = torch.empty(max(world, 1) * per * 24, dtype=torch.uint8, device="cuda")
    own_comm = None
    if world == 1:
        try:
            own_comm = _native.Comm(0, 1, _native.Comm.unique_id())
            how = "ffs_gather_results on a one-rank RCCL communicator"
        except Exception as exc:  # no librccl: the record copy stands in for the gather
            how = "device copy of the records (one-rank communicator failed: %s)" % repr(exc)[:80]
    else:
        how = ("ffs_gather_results" if comm is not None else "torch.distributed.all_gather_into_tensor"
               + (" through host memory (gloo)" if host_coll else ""))

    def step():
        al.solve_async(db, 0, n_local, cand_out, pair_out)
        if world == 1:
            if own_comm is not None:
                own_comm.gather_pair_results(pair_out, gathered)
            else:
                gathered.copy_(pair_out)
        elif comm is not None:
            comm.gather_pair_results(pair_out, gathered)
        elif host_coll:
            host_all = torch.empty(world * per * 24, dtype=torch.uint8)
            dist.all_gather_into_tensor(host_all, pair_out.cpu())
            gathered.copy_(host_all)
        else:
            dist.all_gather_into_tensor(gathered, pair_out)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    rec = gathered.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)
    lists_fig = None
    if world == 1:
        # the same share with the vectors resident as BOUNDARY LISTS (converted once, outside the timed steps; their
        # lengths known on the host): a step is k_runs_corr + k_finalize_pairs + the gather, and the call never waits
        try:
            dl = db.to_runs(cap=8192)
            torch.cuda.synchronize()
            n_l = dl.data.view(torch.int32).reshape(-1, int(dl.offs.ravel()[1]) // 4)[:, 0].cpu().numpy().reshape(dl.offs.shape)
            dl.bounds = (n_l + 2).astype(np.int32)
            db_bits, db = db, dl
            for _ in range(warmup):
                step()
            fence()
            t1 = time.perf_counter()
            for _ in range(steps):
                step()
            fence()
            el_l = time.perf_counter() - t1
            same = bool(np.array_equal(gathered.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:n_local], rec[:n_local]))
            db = db_bits
            lists_fig = {"ms_per_step": 1e3 * el_l / steps, "solves_per_s_this_gpu": n_local * steps / el_l,
                         "efficiency_vs_headline_batch": n_local * steps / el_l / headline_value, "same_records": same,
                         "predicted_%d_gpu_strong_solves_per_s" % proxy_world: n_local * steps / el_l * proxy_world}
        except Exception as exc:
            lists_fig = {"error": repr(exc)[:200]}
    golden = load_headline_golden()
    mine = rec[(rank if world > 1 else 0) * per:][:n_local]
    ok = sum(int(mine[i]["best_cand"]) == golden[s]["index"] and int(mine[i]["offset"]) == golden[s]["offset"]
             for i, s in enumerate(range(lo, hi)) if s in golden)
    n_gold = sum(1 for s in range(lo, hi) if s in golden)
    al.close()
    if own_comm is not None:
        own_comm.close()
    out = {
        "workload": "configs[3]: %d pairs x 7 ratios in total, contiguous shards of %d pairs per rank, one all-gather of the "
                    "24-byte records per step" % (total_pairs, per),
        "pairs_per_rank_per_step": n_local, "pairs_in_flight": in_flight, "steps": steps,
        "ms_per_step": 1e3 * elapsed / steps, "gather": how,
        "own_shard_matching_reference_golden": "%d/%d" % (ok, n_gold),
    }
    if world > 1:
        out["value"] = total_pairs * steps / elapsed
        out["unit"] = "7-ratio solves/s (all ranks, strong scaling)"
    else:
        rate = n_local * steps / elapsed
        out.update({
            "what": "ONE GPU running one rank's share at %d GPUs" % proxy_world,
            "solves_per_s_this_gpu": rate,
            "efficiency_vs_headline_batch": rate / headline_value,
            "predicted_%d_gpu_strong_solves_per_s" % proxy_world: rate * proxy_world,
            "note": "prediction = this rate x %d: shards are independent, the only collective is the %d-byte gather timed "
                    "here on one rank (xGMI latency of a %d-rank all-gather of %d bytes comes on top: ~20-30 us per step)"
                    % (proxy_world, per * 24, proxy_world, per * 24 * proxy_world),
        })
        if lists_fig is not None:
            out["vectors_resident_as_boundary_lists"] = lists_fig
    return out


def load_headline_golden():
    path = os.path.join(ROOT, "tests", "golden", "headline_golden.json")
    if not os.path.exists(path):
        return {}
    return {g["seed"]: g for g in json.load(open(path))["pairs"]}


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(args)
    import numpy as np
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    n_dev_visible = torch.cuda.device_count()
    if n_dev_visible == 0:
        fail_line(args, "no HIP device visible", world)
    if args.backend == "nccl" and local_rank >= n_dev_visible:
        fail_line(args, "rank %d (local rank %d) has no GPU: %d HIP device(s) visible; one rank per GPU with RCCL"
                  % (rank, local_rank, n_dev_visible), world)
    device = local_rank % n_dev_visible
    torch.cuda.set_device(device)
    dist = None
    force_dist = os.environ.get("FFS_BENCH_FORCE_DIST") == "1"  # exercise the RCCL path with one rank
    use_dist = world > 1 or force_dist
    host_coll = args.backend == "gloo"  # control collectives and the record gather go through host memory
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if host_coll:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    coll_dev = "cpu" if host_coll else "cuda"

    from ffsubsync_amd import _native, batch
    from workloads import synth

    n_cand = 7
    strong = args.scaling == "strong"
    if strong:
        lo, hi = batch.shard_bounds(args.pairs, rank, world)
        seeds = list(range(lo, hi))
    else:
        seeds = [rank * args.pairs + i for i in range(args.pairs)]
    P = len(seeds)
    per = (args.pairs + world - 1) // world if strong else args.pairs  # records per rank in the gather
    specs = [synth.make_pair_spec(s, duration_s=args.duration) for s in seeds]
    db = synth.build_device_batch(specs, packed=(args.input_format == "bits"))
    n_ref = db.required_fft_length(6000, reference_length=True)  # the reference's N = 2^ceil(log2(R+S)) (aligners.py:67-68)
    # the +-6000 lag window lets the device use the shortest alias-free transform (ffs_plan_length)
    n_dev = n_ref if args.reference_length else db.required_fft_length(6000)
    cand_out = torch.empty(max(P, 1) * n_cand * 24, dtype=torch.uint8, device="cuda")
    pair_out = torch.zeros(per * 24, dtype=torch.uint8, device="cuda")
    gathered = torch.empty(world * per * 24, dtype=torch.uint8, device="cuda") if use_dist else None
    # per-kernel HIP events are recorded in the timed steps of a plain run too, so that it times exactly the steps a
    # --full run times; only --full reads them into the kernel tables and rooflines
    profile = not args.no_profile and args.streams == 1
    gather_impl = None
    comm = None
    ranks_seen = [0]
    if use_dist:
        seen = [None] * world
        dist.all_gather_object(seen, (rank, device, socket.gethostname()))
        ranks_seen = [list(x) for x in seen]
    if use_dist and host_coll:
        gather_impl = "torch.distributed (gloo) all_gather_into_tensor through host memory [--backend gloo: ranks may share a GPU]"
    elif use_dist:
        # the library's own collective (ffs_gather_results, RCCL C API); checked once against torch's
        try:
            comm = batch.make_comm(rank, world)
            probe = (torch.arange(per * 24, dtype=torch.int32, device="cuda") + rank).to(torch.uint8)
            a = comm.gather_pair_results(probe)
            b = torch.empty_like(a)
            dist.all_gather_into_tensor(b, probe)
            torch.cuda.synchronize()
            if not torch.equal(a, b):
                raise RuntimeError("ffs_gather_results disagrees with all_gather_into_tensor")
            gather_impl = "ffs_gather_results (RCCL ncclAllGather via the C ABI)"
        except Exception as exc:  # keep the scaling record: fall back to torch.distributed's RCCL binding
            comm = None
            gather_impl = "torch.distributed.all_gather_into_tensor (ffs_comm_create failed: %s)" % repr(exc)[:120]
        # every rank must take the same branch
        flag = torch.tensor([1 if comm is not None else 0], dtype=torch.int32, device=coll_dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0 and comm is not None:
            comm.close()
            comm = None
            gather_impl = "torch.distributed.all_gather_into_tensor (ffs_comm_create failed on another rank)"

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    info_now = {}  # what the most recent timed() call went through (run-boundary statistics of its plan)

    def timed(n_fft, steps, warmup, max_offset=6000, the_db=None, cands=n_cand, algorithm=None):
        """W untimed + K timed passes over this rank's pairs with a plan of length n_fft."""
        the_db = db if the_db is None else the_db
        aligner = batch.BatchAligner(n_fft, cands, max_offset_samples=max_offset, pairs_in_flight=args.pairs_in_flight,
                                     streams=args.streams, algorithm=algorithm or args.algorithm)

        def step():
            aligner.solve_async(the_db, 0, P, cand_out, pair_out)
            if use_dist and cands == n_cand:
                if comm is not None:
                    comm.gather_pair_results(pair_out, gathered)
                elif host_coll:
                    host_all = torch.empty(world * per * 24, dtype=torch.uint8)
                    dist.all_gather_into_tensor(host_all, pair_out.cpu())
                    gathered.copy_(host_all)
                else:
                    dist.all_gather_into_tensor(gathered, pair_out)

        for _ in range(warmup):
            step()
        aligner.plan.profile(profile)
        fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        fence()
        elapsed = time.perf_counter() - t0
        ktimes = aligner.plan.profile_read() if profile else {}
        aligner.plan.profile(False)
        if use_dist:
            t = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        seg = (n_fft % 3 == 0 and n_fft // 3 >= 65536 and os.environ.get("FFS_DISABLE_SEGMENTED") != "1"
               and max_offset is not None)
        calls, chunks, fft_chunks = aligner.plan.runs_stats()
        info_now.clear()
        info_now.update({
            "algorithm": algorithm or args.algorithm,
            "path": ("transforms" if calls == 0 or fft_chunks == chunks else
                     "run boundaries" if fft_chunks == 0 else
                     "run boundaries, %d of %d sub-batches through the transforms" % (fft_chunks, chunks)),
            "boundaries_last_call": aligner.plan.runs_boundaries_last_call() if calls else 0,
            "vectors_bytes_per_pair": float(np.mean(the_db.lens.sum(axis=1))) / 8.0,
            "pairs_per_call": P, "cands": cands,
        })
        aligner.close()
        return elapsed, ktimes, seg

    # Bytes every kernel HAS to move per pair, in units of one complex fp32 transform
    # slot U = 8*n bytes (n = device transform length): a pair is 1 reference + ceil(cands/2) packed candidate
    # transforms; the reference's spectrum is real-input Hermitian, so only half of its rows are stored.
    def must_move(n_fft, seg, cands, ref_bytes_per_sample=None):
        # an odd candidate count leaves one real candidate in the last packed transform: only half of its rows
        # are stored, transformed and read (HALF_LAST, ffs_kernels.h)
        half_last = cands % 2 == 1 and os.environ.get("FFS_DISABLE_HALF_LAST") != "1"
        slots = (cands + 1) // 2 - (0.5 if half_last else 0.0)
        unit = 8.0 * n_fft
        in_bytes = float(np.mean(db.lens.sum(axis=1))) / (8.0 if db.dtype == _native.FFS_DTYPE_U1 else 1.0)
        if cands != n_cand:
            in_bytes *= (1 + cands) / (1 + n_cand)
        if ref_bytes_per_sample is not None:  # references in another element type than the candidates (float64: 8 bytes)
            in_bytes += float(np.mean(db.lens[:, 0])) * (ref_bytes_per_sample - (0.125 if db.dtype == _native.FFS_DTYPE_U1 else 1.0))
        if seg:  # three blocks of n/3 per candidate, spectrum products added in the mid pass
            return {"pass_a": (slots + 0.5) * unit + in_bytes, "mid": (slots + 0.5 + slots / 3.0) * unit,
                    "pass_c": slots / 3.0 * unit}
        return {"pass_a": (slots + 0.5) * unit + in_bytes, "mid": (2 * slots + 0.5) * unit, "pass_c": slots * unit}

    # SURVEY 8(d) normaliser: 168*N bytes per seven-ratio solve (N = the reference's 2^21), apportioned
    # by transform halves: pass A = 14 halves of 4*N, mid = 21, pass C = 7
    share = {"pass_a": 56, "mid": 84, "pass_c": 28}

    def kernel_table(ktimes, steps, n_fft, seg, cands=n_cand, ref_bytes_per_sample=None):
        mm = must_move(n_fft, seg, cands, ref_bytes_per_sample)
        last_info = dict(info_now)  # of the timed() call these kernel times belong to
        work_pmc = {}
        tpath_w = os.path.join(ROOT, "profiles", "traffic_per_pair.json")
        if os.path.exists(tpath_w) and cands == n_cand:
            work_pmc = json.load(open(tpath_w)).get("%d_work" % n_fft, {})
        per_kernel = {}
        for k, (ms, n) in ktimes.items():
            if n == 0:
                continue
            pairs_per_launch = P * steps / n
            entry = {"avg_ms": ms / n, "launches": n, "total_ms": ms, "us_per_pair": 1e3 * ms / (P * steps)}
            if k == "runs_extract" and last_info.get("boundaries_last_call"):
                # reads every bit-packed vector once, writes one entry per boundary (+ the sentinel of each list): 8 bytes
                # (position, ones in front) in the reference's list, 4 (position) in the candidates' (RunsRef, ffs_runs.h);
                # the call's boundary count is split between the lists by their number -- the vectors are equally dense
                entry_bytes = (8.0 + 4.0 * cands) / (1.0 + cands)
                per_pair = (last_info["vectors_bytes_per_pair"]
                            + entry_bytes * last_info["boundaries_last_call"] / last_info["pairs_per_call"] + 8.0 + 4.0 * cands)
                entry["must_move_bytes_per_launch"] = per_pair * pairs_per_launch
                entry["must_move_GBps"] = entry["must_move_bytes_per_launch"] / (ms / n * 1e-3) / 1e9
                entry["frac_of_8TBps"] = entry["must_move_GBps"] * 1e9 / HBM_PEAK
                entry["boundaries_per_vector"] = last_info["boundaries_last_call"] / (last_info["pairs_per_call"] * (1.0 + cands))
            if k == "levels" and ref_bytes_per_sample is not None:
                # k_levels_sample + k_levels_bits: every float sample of the references read once, three threshold planes of
                # one bit per sample written
                per_pair = float(np.mean(db.lens[:, 0])) * (ref_bytes_per_sample + 3.0 / 8.0)
                entry["must_move_bytes_per_launch"] = per_pair * pairs_per_launch
                entry["must_move_GBps"] = entry["must_move_bytes_per_launch"] / (ms / n * 1e-3) / 1e9
                entry["frac_of_8TBps"] = entry["must_move_GBps"] * 1e9 / HBM_PEAK
            if k == "runs_corr":
                entry["bound"] = "LDS atomics (one ds_add_u32 per boundary coincidence inside the lag window) -- not an HBM kernel"
            if k in work_pmc:  # wave-instructions and LDS-array cycles per pair from the PMC passes (profiles/make_traffic.py)
                entry["pmc_work_per_pair"] = work_pmc[k]
            if k in mm:
                entry["must_move_bytes_per_launch"] = mm[k] * pairs_per_launch
                entry["must_move_GBps"] = entry["must_move_bytes_per_launch"] / (ms / n * 1e-3) / 1e9
                entry["frac_of_8TBps"] = entry["must_move_GBps"] * 1e9 / HBM_PEAK
                if cands == n_cand:
                    entry["normaliser_GBps"] = share[k] * n_ref * pairs_per_launch / (ms / n * 1e-3) / 1e9
            per_kernel[k] = entry
        return per_kernel

    elapsed, ktimes, seg_mode = timed(n_dev, args.steps, args.warmup)
    head_info = dict(info_now)
    by_runs = head_info["path"] != "transforms"

    pres = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P].copy()
    cres = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[: P * n_cand].reshape(P, n_cand).copy()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, seeds, pres, cres)
    if args.full:
        # correctness of what was timed: every pair the reference-generated goldens cover (bench seeds 0..255,
        # tests/golden/headline_golden.json = the UNMODIFIED reference's (ratio, offset, score)), plus the
        # generator's ground truth for all pairs
        golden = load_headline_golden() if args.duration == 7200.0 else {}
        g_total = g_ok = 0
        for i, s in enumerate(seeds):
            g = golden.get(s)
            if g is None:
                continue
            g_total += 1
            sc = float(g["score"])
            gaps = g.get("per_candidate_top2_gap", [0.0] * n_cand)
            g_ok += int(int(pres[i]["best_cand"]) == g["index"] and int(pres[i]["offset"]) == g["offset"]
                        and abs(float(pres[i]["score"]) - sc) <= 1e-5 * abs(sc)
                        and all((int(cres[i, j]["offset"]) == off or gaps[j] <= 0.5)
                                and abs(float(cres[i, j]["score"]) - float(csc)) <= 1e-5 * abs(float(csc))
                                for j, (csc, off) in enumerate(g["per_candidate"])))
        truth_ok = sum(
            int(pres[i]["best_cand"] == sp.true_ratio_index and abs(int(pres[i]["offset"]) - sp.true_offset_samples) <= 30)
            for i, sp in enumerate(specs)
        )
        ambiguous = int(((cres["flags"] & 2) != 0).sum())
        # health of the fp32 transform chain itself (the exact re-evaluation would mask a damaged one as long
        # as the true peak still gets nominated): fp32 value of every winning lag vs its exact score
        fp32_err = float(np.abs(cres["score_f32"].astype(np.float64) - cres["score"]).max()) if P else 0.0

    total_pairs = args.pairs if strong else world * args.pairs
    solves_per_s = total_pairs * args.steps / elapsed
    result = {
        "metric": "alignments/sec (2 h@100 Hz, 7 framerate ratios)",
        "value": solves_per_s,
        "unit": "7-ratio solves/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        # the arithmetic the timed path computes in: exact int32 counts (run-boundary path; fp64 only for the final score
        # expression) or fp32 transforms that nominate + integer re-evaluation (transform path)
        "dtype": "i32" if by_runs else "f32",
        "data": "synthetic",
        "config": {
            "workload": "configs[2]: %d x %.0f s@100 Hz pairs %s (%d batches of 1024), MaxScoreAligner over 7 framerate "
                        "ratios, max_offset_samples=6000" % (args.pairs, args.duration,
                                                            "in total" if strong else "per GPU", max(1, args.pairs // 1024)),
            "n_fft_reference": n_ref,
            "n_fft_device": n_dev,
            "pairs_per_gpu": P,
            "pairs_in_flight": args.pairs_in_flight,
            "streams": args.streams,
            "input_format": "bit-packed 0/1 vectors (FFS_DTYPE_U1) resident in HBM" if db.dtype == _native.FFS_DTYPE_U1
                            else "0/1 bytes (FFS_DTYPE_U8) resident in HBM",
            "algorithm": head_info["algorithm"],
            "path": head_info["path"],
            "arithmetic": ("run-boundary correlation (csrc/ffs_runs.h): the exact integer correlation of the run-length-coded "
                           "vectors at EVERY lag of the window (boundary lists -> sparse second difference -> two prefix sums), "
                           "argmax over exact scores; chosen per sub-batch by the library (FFS_ALGO_AUTO) because the boundary "
                           "lists are short -- the batched-FFT path on the same pairs is the `fft_path` entry"
                           if by_runs else
                           "fp32 transforms nominate lags; integer (popcount) re-evaluation of the winners: offsets and "
                           "scores are exact"),
            "parallelism": ("pairs sharded by rank, %s of 24 B/pair results" % gather_impl) if use_dist else "single GPU",
            "gather_impl": gather_impl,
            # 0 = the library's own collective (ffs_gather_results), 1 = torch.distributed's all_gather_into_tensor was used
            # instead (ffs_comm_create failed somewhere / --backend gloo); None on one GPU
            "gather_fallback": (0 if comm is not None else 1) if use_dist else None,
            "ranks_seen": ranks_seen,  # [rank, device, host] of every rank, all-gathered
            "devices_used": len({(x[2], x[1]) for x in ranks_seen}) if use_dist else 1,
        },
        "full": bool(args.full),
    }
    if args.full:
        result["offset_match"] = {
            "pairs_matching_reference_golden": "%d/%d" % (g_ok, g_total),
            "golden": "tests/golden/headline_golden.json (unmodified reference, bench seeds 0..1023): winning index and "
                      "offset bit-identical, all 7 per-candidate scores within 1e-5, per-candidate offsets "
                      "bit-identical wherever the reference's own top-2 gap exceeds 0.5 (exact ties on the "
                      "plateaus of wrong-ratio candidates are decided by its fp64 rounding noise)",
            "pairs_matching_ground_truth": truth_ok, "pairs": P, "ambiguous_flags": ambiguous,
            "max_abs_fp32_error_at_winning_lags": fp32_err}
        result["normaliser"] = {
            "what": "SURVEY 8(d): the reference's 168*N bytes per seven-ratio solve (N = 2^21) x solves/s -- measures "
                    "algorithmic saving, not HBM efficiency (the device moves fewer bytes: see roofline)",
            "bytes_per_solve": 168 * n_ref,
            "GBps": solves_per_s * 168 * n_ref / 1e9,
            "frac_of_8TBps_per_gpu": solves_per_s * 168 * n_ref / (HBM_PEAK * world),
        }

    def roofline_of(per_kernel, pairs, steps, n_fft, seg_mode, cands=n_cand):
        """`roofline` object for the kernel that takes the most time among those that move bytes through HBM."""
        hbm_kernels = [k for k in per_kernel if "must_move_GBps" in per_kernel[k]]
        dom = max(hbm_kernels, key=lambda k: per_kernel[k]["total_ms"])
        pairs_per_launch = pairs * steps / per_kernel[dom]["launches"]
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "traffic_per_pair.json")
        if os.path.exists(tpath):  # PMC-measured HBM bytes (profiles/run_pmc.sh), keyed by device length
            tj = json.load(open(tpath)).get(str(n_fft), {})
            if dom in tj:
                traffic = tj[dom] * pairs_per_launch
        mm_launch = per_kernel[dom]["must_move_bytes_per_launch"]
        out = {
            "kernel": {"pass_a": "k_pass_a", "pass_c": "k_pass_c_pruned", "runs_extract": "k_runs_extract",
                       "mid": ("k_mid_seg_one" if (cands + 1) // 2 <= 4 else "k_mid_seg_pipe") if seg_mode else "k_mid"}[dom],
            "bound": "hbm",
            "achieved": per_kernel[dom]["must_move_GBps"],
            "peak": HBM_PEAK / 1e9,
            "unit": "GB/s",
            "frac": per_kernel[dom]["must_move_GBps"] * 1e9 / HBM_PEAK,
            "traffic": traffic,
            "wasted": (traffic / mm_launch) if traffic else None,
            "bytes_per_launch": mm_launch,
            "avg_launch_ms": per_kernel[dom]["avg_ms"],
            "frac_of_copy_ceiling": per_kernel[dom]["must_move_GBps"] * 1e9 / HBM_COPY_CEILING,
            "share_of_kernel_time": per_kernel[dom]["total_ms"] / sum(v["total_ms"] for v in per_kernel.values()),
        }
        if dom == "runs_extract":
            out["note"] = ("achieved = bytes k_runs_extract HAS to move per launch (every bit-packed vector read once, 8 bytes "
                           "written per run boundary; DESIGN.md section 5) / its average launch duration from HIP events on the "
                           "launch stream; traffic = PMC-measured HBM bytes per launch (profiles/traffic_per_pair.json).  The "
                           "other kernel of the path, k_runs_corr, works out of LDS (boundary lists of a few KB per vector, one "
                           "ds_add_u32 per boundary coincidence) and moves no comparable HBM volume: see kernels.runs_corr")
        else:
            out["note"] = ("achieved = bytes this kernel HAS to move per launch (DESIGN.md section 5: every stored row read "
                           "once, every result row written once) / its average launch duration from HIP events on the "
                           "launch stream; traffic = PMC-measured HBM bytes per launch (profiles/traffic_per_pair.json); "
                           "wasted = traffic / must-move")
        return out

    def coincidences_per_pair(sample=256):
        """Boundary coincidences inside the lag window per seven-ratio pair = the scatter-adds k_runs_corr HAS to make
        (one +-1 per pair of boundaries (p, q) with q - p among the window's lags but the last), counted exactly on the
        host for the first `sample` pairs of the batch (numpy searchsorted over the generator's run lists)."""
        tot, n_s = 0, min(sample, P)
        for sp in specs[:n_s]:
            ref, cands = synth.pair_arrays(sp)
            q = np.flatnonzero(np.diff(np.concatenate([[0], ref, [0]]).astype(np.int8)))
            R = ref.size
            for c in cands:
                p_ = np.flatnonzero(np.diff(np.concatenate([[0], c, [0]]).astype(np.int8)))
                S = c.size
                d_lo, d_hi = max(-5999, -S + 1), min(6000, R - 1)  # FFTAligner(6000): lags [-max+1, +max]
                tot += int((np.searchsorted(q, p_ + d_hi - 1, "right") - np.searchsorted(q, p_ + d_lo, "left")).sum())
        return tot / max(1, n_s), n_s

    def lds_roofline(per_kernel, pairs, steps):
        """`roofline` of k_runs_corr: bound by the LDS scatter-add rate for uniformly random words (the ceiling is reached
        only with all 64 lanes adding; `frac_of_conflict_free_rate` prices the same adds against the conflict-free rate)."""
        k = per_kernel["runs_corr"]
        per_pair, n_s = coincidences_per_pair()
        pairs_per_launch = pairs * steps / k["launches"]
        # Ceiling: profiles/lds_issue_rates.hip (round 6: NO vector ALU work between the DS operations; its ds_write_b32 control
        # reproduces the guide's 4 cycles per wave-instruction).  ds_add_u32 costs 4.08 cycles conflict-free and 7.36 for
        # uniformly random words (bank conflicts: 32 random addresses per 32 banks) -- the histogram's situation.
        peak, peak_free, src = None, None, os.path.join(ROOT, "profiles", "lds_issue_rates.json")
        if os.path.exists(src):
            cj = json.load(open(src))
            row = cj["ds_add_u32_32_waves_per_cu"]
            per_s = 64.0 * cj["cus"] * cj["clock_MHz"] * 1e6
            peak, peak_free = per_s / row["random_words"] / 1e9, per_s / row["conflict_free"] / 1e9
        achieved = per_pair * pairs_per_launch / (k["avg_ms"] * 1e-3) / 1e9
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "traffic_per_pair.json")
        if os.path.exists(tpath):
            tj = json.load(open(tpath)).get(str(n_dev), {})
            if "runs_corr" in tj:
                traffic = tj["runs_corr"] * pairs_per_launch
        out = {"kernel": "k_runs_corr", "bound": "lds", "achieved": achieved, "peak": peak, "unit": "G lane-adds/s",
               "frac": (achieved / peak) if peak else None, "traffic": traffic,
               "per_launch": per_pair * pairs_per_launch, "avg_launch_ms": k["avg_ms"],
               "share_of_kernel_time": k["total_ms"] / sum(v["total_ms"] for v in per_kernel.values()),
               "frac_of_conflict_free_rate": (achieved / peak_free) if peak_free else None,
               "peak_source": "profiles/lds_issue_rates.json (VALU-free harness; ds_write_b32 control = the guide's 4 cycles): "
                              "ds_add_u32 to uniformly random words = 7.36 cycles per wave-instruction (bank conflicts), "
                              "conflict-free 4.08; 64 lanes x 256 CUs x 2.4 GHz",
               "note": "achieved = boundary coincidences inside the lag window per launch (exact count on the host for the first "
                       "%d pairs x pairs per launch) / average launch duration (HIP events); traffic = PMC-measured HBM bytes "
                       "per launch (the kernel reads the boundary lists: not what bounds it)" % n_s}
        lj = json.load(open(tpath)).get("%d_work" % n_dev, {}).get("runs_corr", {}) if os.path.exists(tpath) else {}
        if lj.get("lds_idx_active_per_pair"):
            out["lds_conflict_frac"] = lj.get("lds_bank_conflict_per_pair", 0.0) / lj["lds_idx_active_per_pair"]
        return out

    if args.full and profile and rank == 0:
        per_kernel = kernel_table(ktimes, args.steps, n_dev, seg_mode)
        result["kernels"] = per_kernel
        hbm_roof = roofline_of(per_kernel, P, args.steps, n_dev, seg_mode)
        dom_all = max(per_kernel, key=lambda k: per_kernel[k]["total_ms"])
        if dom_all == "runs_corr" and args.duration == 7200.0:
            # the DOMINANT kernel of the timed path is not an HBM kernel: its roofline is the LDS scatter-add rate; the
            # HBM record of the path's streaming kernel (k_runs_extract) stays beside it
            result["roofline"] = lds_roofline(per_kernel, P, args.steps)
            result["roofline_hbm"] = hbm_roof
        else:
            result["roofline"] = hbm_roof

    # BASELINE configs[3] in the same invocation: the SAME 1024 pairs split over the ranks, every step = this rank's share
    # (contiguous block, batch.shard_bounds) + the all-gather of the 24-byte records.  On one GPU it is the proxy the
    # 8-GPU run reduces to: one rank's share at world 8 (128 pairs per step), gathered through a one-rank RCCL
    # communicator -- what a rank of the sharded job does per step, launch overheads and sweep tails included.
    if args.full and not args.skip_secondary and not strong and args.duration == 7200.0:
        try:
            result["strong_scaling" if world > 1 else "strong_scaling_proxy"] = strong_leg(
                torch, _native, batch, synth, args, rank, world, dist if use_dist else None, comm, host_coll, n_dev,
                solves_per_s, coll_dev)
        except Exception as exc:
            if world > 1:
                raise
            result["strong_scaling_proxy"] = {"error": repr(exc)[:300]}

    secondary = args.full and rank == 0 and world == 1 and not args.skip_secondary
    if secondary and by_runs:
        # The SAME pairs through the batched-FFT path (FFS_ALGO_FFT: what rounds 1-3 timed as the headline, and what the
        # library still runs for float / byte inputs and for vectors whose boundary lists are long): the north star's
        # "batched 1-D real FFT + complex multiply + inverse FFT + argmax" kernels with their own roofline.
        st_x = max(2, args.steps // 4)
        el_x, kt_x, seg_x = timed(n_dev, st_x, 1, algorithm="fft")
        pres_x = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P]
        cres_x = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[: P * n_cand].reshape(P, n_cand)
        result["fft_path"] = {
            "what": "same %d pairs, FFS_ALGO_FFT (window-shortened block-segmented transforms, n_fft_device %d): fp32 "
                    "transforms nominate, integer re-evaluation decides" % (P, n_dev),
            "value": P * st_x / el_x, "unit": "7-ratio solves/s", "ms_per_step": 1e3 * el_x / st_x, "dtype": "f32",
            "identical_pair_results": bool(np.array_equal(pres_x, pres)),
            "identical_candidate_results": bool(all(np.array_equal(cres_x[f], cres[f]) for f in ("score", "offset", "flags"))),
            "normaliser_frac_of_8TBps": (P * st_x / el_x) * 168 * n_ref / HBM_PEAK,
            "max_abs_fp32_error_at_winning_lags": float(np.abs(cres_x["score_f32"].astype(np.float64) - cres_x["score"]).max()),
        }
        if profile:
            pk_x = kernel_table(kt_x, st_x, n_dev, seg_x)
            result["fft_path"]["kernels"] = pk_x
            result["fft_path"]["roofline"] = roofline_of(pk_x, P, st_x, n_dev, seg_x)
    if secondary and by_runs and db.dtype == _native.FFS_DTYPE_U1:
        # The same pairs with their BOUNDARY LISTS resident in HBM instead of their bits (FFS_DTYPE_RUNS: what the list
        # rasteriser and ffs_runs_from_bits hand over): no extraction pass, and -- the lists' lengths are known on the
        # host -- nothing read back per call.
        try:
            dl = db.to_runs(cap=8192)
            torch.cuda.synchronize()
            n_l = dl.data.view(torch.int32).reshape(-1, dl.offs.ravel()[1] // 4)[:, 0].cpu().numpy().reshape(dl.offs.shape)
            dl.bounds = (n_l + 2).astype(np.int32)
            st_l = max(2, args.steps // 2)
            el_l, kt_l, _ = timed(n_dev, st_l, 1, the_db=dl)
            pres_l = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P]
            cres_l = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[: P * n_cand].reshape(P, n_cand)
            result["resident_lists"] = {
                "what": "same %d pairs, boundary lists resident in HBM (FFS_DTYPE_RUNS, %.0f entries per vector on average) with "
                        "host-known bounds: k_runs_corr only" % (P, float(n_l.mean())),
                "value": P * st_l / el_l, "unit": "7-ratio solves/s", "ms_per_step": 1e3 * el_l / st_l, "path": info_now["path"],
                "identical_pair_results": bool(np.array_equal(pres_l, pres)),
                "identical_candidate_results": bool(all(np.array_equal(cres_l[f], cres[f]) for f in ("score", "offset", "flags"))),
            }
            if profile:
                result["resident_lists"]["kernels_us_per_pair"] = {k: 1e3 * v[0] / (P * st_l) for k, v in kt_l.items() if v[1]}
            del dl
        except Exception as exc:
            result["resident_lists"] = {"error": repr(exc)[:300]}
    if secondary and not args.reference_length and n_dev != n_ref:
        # the same pairs with the reference's own transform length N = 2^21 (single transform), for the record
        st2 = max(2, args.steps // 4)
        el2, kt2, seg2 = timed(n_ref, st2, 1, algorithm="fft")
        pres2 = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P]
        result["reference_length"] = {
            "n_fft_device": n_ref,
            "path": "transforms (FFS_ALGO_FFT), single transform of the reference's own length",
            "value": P * st2 / el2,
            "ms_per_step": 1e3 * el2 / st2,
            "identical_pair_results": bool(np.array_equal(pres2, pres)),
            "normaliser_frac_of_8TBps": (P * st2 / el2) * 168 * n_ref / HBM_PEAK,
        }
        if profile:
            result["reference_length"]["kernels"] = {
                k: {kk: v[kk] for kk in ("avg_ms", "us_per_pair", "must_move_GBps", "frac_of_8TBps") if kk in v}
                for k, v in kernel_table(kt2, st2, n_ref, seg2).items()}

    if secondary:
        # single-ratio FFTAligner solves/s (BASELINE configs[1] as a batch: every pair against
        # the candidate rasterised at its true ratio), with the production lag window and without one
        sdb = db.select_candidates([sp.true_ratio_index for sp in specs])
        single = {}
        for label, mo, key in (("max_offset_6000", 6000, "single_6000"), ("max_offset_none", None, "single_none")):
            n1 = sdb.required_fft_length(mo)
            st1 = max(2, args.steps // 4)
            el_auto, path_auto = None, None
            if args.algorithm != "fft":  # what the library picks on its own, then the transform kernels for the table
                el_auto, _, _ = timed(n1, st1, 1, max_offset=mo, the_db=sdb, cands=1)
                path_auto = info_now["path"]
                c_auto = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:P].copy()
            el, kt1, seg1 = timed(n1, st1, 1, max_offset=mo, the_db=sdb, cands=1, algorithm="fft")
            c1 = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[:P]
            hits = [(int(c1[i]["offset"]) == golden[s][key][1]
                     and abs(float(c1[i]["score"]) - float(golden[s][key][0])) <= 1e-5 * abs(float(golden[s][key][0])))
                    for i, s in enumerate(seeds) if s in golden]
            single[label] = {
                "n_fft_device": int(n1),
                "solves_per_s": P * st1 / (el_auto or el),
                "path": path_auto or "transforms",
                "transforms_solves_per_s": P * st1 / el,
                "pairs_matching_reference_golden": "%d/%d" % (sum(hits), len(hits)),
            }
            if el_auto is not None:
                single[label]["identical_results_on_both_paths"] = bool(
                    all(np.array_equal(c_auto[f], c1[f]) for f in ("score", "offset", "flags")))
            if profile:
                single[label]["kernels"] = {
                    k: {kk: v[kk] for kk in ("us_per_pair", "must_move_GBps", "frac_of_8TBps") if kk in v}
                    for k, v in kernel_table(kt1, st1, n1, seg1, cands=1).items()}
        result["single_ratio"] = single

        # the reference's DEFAULT constructor FFTAligner() has no lag window: seven-ratio MaxScoreAligner(FFTAligner())
        # solves, every lag of the full correlation searched (device length 3*2^19 by the zero-overlap rule)
        n_w = db.required_fft_length(None)
        st_w = max(2, args.steps // 5)
        el_w, kt_w, seg_w = timed(n_w, st_w, 1, max_offset=None)
        pres_w = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P]
        cres_w = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[: P * n_cand].reshape(P, n_cand)
        from workloads import golden_check

        wl_gold = golden_check.load("windowless_golden") if args.duration == 7200.0 else {}
        wl_ok, wl_total, wl_first = golden_check.matching(wl_gold, seeds, pres_w, cres_w)
        result["windowless"] = {
            "what": "max_offset_samples=None (aligners.py:25-29 default): same pairs, every lag searched",
            "n_fft_device": int(n_w), "path": info_now["path"], "value": P * st_w / el_w, "unit": "7-ratio solves/s",
            "ms_per_step": 1e3 * el_w / st_w,
            "pairs_matching_ground_truth": int(sum(
                int(pres_w[i]["best_cand"]) == sp.true_ratio_index and abs(int(pres_w[i]["offset"]) - sp.true_offset_samples) <= 30
                for i, sp in enumerate(specs))),
            "pairs": P,
            # the unmodified reference's MaxScoreAligner(FFTAligner()) on the same seeds (tests/golden/windowless_golden.json):
            # same rule as the windowed headline (workloads/golden_check.py)
            "pairs_matching_reference_golden": "%d/%d" % (wl_ok, wl_total),
        }
        if wl_first:
            result["windowless"]["first_mismatches"] = [str(x) for x in wl_first]
        if profile:
            result["windowless"]["kernels"] = {
                k: {kk: v[kk] for kk in ("avg_ms", "us_per_pair", "must_move_GBps", "frac_of_8TBps") if kk in v}
                for k, v in kernel_table(kt_w, st_w, n_w, seg_w).items()}

        # How the automatic choice moves with the number of runs per vector: the benchmark generator with gaps, runs and
        # jitter scaled down (1/scale times as many runs: from subtitle-like activity to a flickering frame-level
        # detector), 256 pairs each, library default (auto) next to the forced transform path.
        if args.algorithm == "auto" and args.duration == 7200.0:
            keep_db, keep_P, keep_specs = db, P, specs
            sweep = []
            try:
                for scale in (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125):
                    P = 256
                    specs = [synth.make_pair_spec(7000 + i, duration_s=args.duration, run_scale=scale) for i in range(P)]
                    db = synth.build_device_batch(specs)
                    n_s = db.required_fft_length(6000)
                    # (dense rows: ~4 ms per step either way -- eight timed steps each, so that a 1 % difference between the
                    # automatic choice and the forced transforms is not launch-to-launch noise)
                    n_st = 3 if scale >= 0.25 else 8
                    el_a, kt_a, _ = timed(n_s, n_st, 2)
                    path_a = info_now["path"]
                    bnd = info_now["boundaries_last_call"] / (P * 8.0)
                    pa_ = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P].copy()
                    el_f, _, _ = timed(n_s, n_st, 2, algorithm="fft")
                    el_a, el_f = el_a * 3 / n_st, el_f * 3 / n_st  # (the figures below are per three steps)
                    pf_ = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:P]
                    sweep.append({
                        "run_scale": scale, "boundaries_per_vector": bnd, "auto_solves_per_s": P * 3 / el_a, "auto_path": path_a,
                        "transforms_solves_per_s": P * 3 / el_f, "identical_pair_results": bool(np.array_equal(pa_, pf_)),
                        "pairs_matching_ground_truth": int(sum(
                            int(pa_[i]["best_cand"]) == sp.true_ratio_index
                            and abs(int(pa_[i]["offset"]) - sp.true_offset_samples) <= 30 for i, sp in enumerate(specs))),
                    })
                result["boundary_density"] = {
                    "what": "256 pairs x 2 h x 7 ratios, max_offset_samples=6000; workloads.synth.make_pair_spec(run_scale): "
                            "gaps U[0.2,8] s and runs U[0.5,6] s times run_scale.  Budget of the automatic choice: twelve boundary "
                            "coincidences per point of the plan length and transform slot; lists of 32 768 boundaries or more "
                            "always go through the transforms", "sweep": sweep}
            except Exception as exc:
                result["boundary_density"] = {"error": repr(exc)[:300], "sweep": sweep}
            finally:
                db, P, specs = keep_db, keep_P, keep_specs

        # the same headline batch as 0/1 BYTES (FFS_DTYPE_U8), the north star's literal input format
        if db.dtype == _native.FFS_DTYPE_U1:
            nb = min(P, 1024)
            keep_db, keep_P = db, P
            try:
                db = synth.build_device_batch(specs[:nb], packed=False)
                P = nb
                st_b = max(2, args.steps // 4)
                el_b, kt_b, seg_b = timed(n_dev, st_b, 1)
                pres_b = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:nb]
                result["byte_inputs"] = {
                    "what": "FFS_DTYPE_U8 vectors (one byte per 10 ms frame) resident in HBM, first %d pairs of the batch" % nb,
                    "path": info_now["path"], "value": nb * st_b / el_b, "unit": "7-ratio solves/s",
                    "identical_pair_results": bool(np.array_equal(pres_b, pres[:nb])),
                }
                if profile:
                    result["byte_inputs"]["kernels"] = {
                        k: {kk: v[kk] for kk in ("us_per_pair", "must_move_GBps", "frac_of_8TBps") if kk in v}
                        for k, v in kernel_table(kt_b, st_b, n_dev, seg_b).items()}
            finally:
                db, P = keep_db, keep_P
        # float-valued references: four-level float64 reference vectors -- the weighted fused VAD's
        # {0, .4, .6, 1}, speech_transformers.py:290-293 -- against the usual bit-packed subtitle rasters, one element
        # type per role (ffs_align_batch_typed).  Seeds 5000.. (tests/golden/float_golden.json pins the first of them to
        # the unmodified reference); the exact re-evaluation is an fp64 dot product over the caller's float64 samples.
        keep_db, keep_P, keep_specs = db, P, specs
        try:
            nf = min(P, 512)
            fspecs = [synth.make_pair_spec(5000 + i, duration_s=args.duration) for i in range(nf)]
            db = synth.build_fused_batch(fspecs)
            P = nf
            st_f = max(2, args.steps // 4)
            el_f, kt_f, seg_f = timed(n_dev, st_f, 1)
            pres_f = pair_out.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)[:nf].copy()
            cres_f = cand_out.cpu().numpy().view(_native.CAND_RESULT_DTYPE)[: nf * n_cand].reshape(nf, n_cand).copy()
            fgold = {}
            fpath = os.path.join(ROOT, "tests", "golden", "float_golden.json")
            if os.path.exists(fpath) and args.duration == 7200.0:
                fgold = {g["seed"]: g for g in json.load(open(fpath))["pairs"]}
            f_ok = f_tot = 0
            for i in range(nf):
                g = fgold.get(5000 + i)
                if g is None:
                    continue
                f_tot += 1
                f_ok += int(int(pres_f[i]["best_cand"]) == g["index"] and int(pres_f[i]["offset"]) == g["offset"]
                            and abs(float(pres_f[i]["score"]) - float(g["score"])) <= 1e-5 * abs(float(g["score"]))
                            and all((int(cres_f[i, j]["offset"]) == off or g["per_candidate_top2_gap"][j] <= 1e-6)
                                    and abs(float(cres_f[i, j]["score"]) - float(csc)) <= 1e-5 * abs(float(csc))
                                    for j, (csc, off) in enumerate(g["per_candidate"])))
            result["float_inputs"] = {
                "what": "%d pairs: float64 four-level reference vectors (0.6*silero + 0.4*webrtc levels) + seven bit-packed "
                        "candidates per pair, resident in HBM; ffs_align_batch_typed (reference FFS_DTYPE_F64, candidates "
                        "FFS_DTYPE_U1); n_fft_device %d.  Round 5: the library finds the levels on the device, writes the "
                        "reference's three threshold planes (one pass over the 5.8 MB of float64 per reference: what bounds the "
                        "leg), and the run-boundary kernel adds the levels up with integer multiplicities 2 : 1 : 2" % (nf, n_dev),
                "path": info_now["path"], "value": nf * st_f / el_f, "unit": "7-ratio solves/s",
                "pairs_matching_reference_golden": "%d/%d" % (f_ok, f_tot),
                "golden": "tests/golden/float_golden.json (unmodified reference on seeds 5000..): offsets bit-identical, scores "
                          "within 1e-5",
                "pairs_matching_ground_truth": int(sum(
                    int(pres_f[i]["best_cand"]) == sp.true_ratio_index
                    and abs(int(pres_f[i]["offset"]) - sp.true_offset_samples) <= 30 for i, sp in enumerate(fspecs))),
                "pairs": nf, "ambiguous_flags": int(((cres_f["flags"] & 2) != 0).sum()),
                "max_abs_fp32_error_at_winning_lags": float(np.abs(cres_f["score_f32"].astype(np.float64) - cres_f["score"]).max()),
            }
            if profile:
                result["float_inputs"]["kernels"] = {
                    k: {kk: v[kk] for kk in ("us_per_pair", "must_move_GBps", "frac_of_8TBps") if kk in v}
                    for k, v in kernel_table(kt_f, st_f, n_dev, seg_f, ref_bytes_per_sample=8.0).items()}
        except Exception as exc:
            result["float_inputs"] = {"error": repr(exc)[:300]}
        finally:
            db, P, specs = keep_db, keep_P, keep_specs
        if args.duration == 7200.0:
            try:
                result["gss"] = gss_figures(torch, _native, specs)
            except Exception as exc:
                result["gss"] = {"error": repr(exc)[:300]}
        try:
            result["drop_in"] = drop_in_figures(torch, specs)
        except Exception as exc:
            result["drop_in"] = {"error": repr(exc)[:300]}
        try:
            result["ingest_inclusive"] = ingest_inclusive_figures(torch, _native)
        except Exception as exc:
            result["ingest_inclusive"] = {"error": repr(exc)[:300]}

    if args.full and rank == 0 and world == 1 and args.cpu_pairs > 0:
        from oracle import aligners_oracle as orc

        # SURVEY 8(d) CPU baseline on this box's host cores.  /root/reference does not exist here, so the timed
        # code is the numpy restatement of aligners.py:50-167 (oracle/aligners_oracle.py), which is pinned to the
        # unmodified reference by tests/golden/*.json; the unmodified reference itself is timed in the build
        # container (profiles/r02_cpu_reference_baseline.json).
        n_s = min(args.cpu_pairs, P)
        inputs = [synth.pair_float_arrays(specs[i]) for i in range(n_s)]
        runs = []
        for _ in range(3):
            t1 = time.perf_counter()
            cpu = [orc.max_score_align(r, c, 6000) for r, c in inputs]
            runs.append(time.perf_counter() - t1)
            if sum(runs) > 40.0:
                break
        agree = all(
            int(pres[i]["best_cand"]) == idx and int(pres[i]["offset"]) == off and abs(pres[i]["score"] - sc) <= 1e-5 * abs(sc)
            for i, ((sc, off), idx) in enumerate(cpu)
        )
        result["cpu_baseline"] = {
            "value": n_s / min(runs),
            "unit": "7-ratio solves/s",
            "cores": 1,
            "kind": "port",
            "sample": "%d of the same pairs (seeds 0..%d), best of %d runs (%s s): numpy complex128 restatement of "
                      "aligners.py:50-167 (oracle/aligners_oracle.py, golden-pinned to the unmodified reference), single "
                      "thread" % (n_s, n_s - 1, len(runs), "/".join("%.1f" % r for r in runs)),
            "host_cpus": os.cpu_count(),
            "unmodified_reference_in_build_container": "profiles/r04_cpu_reference_baseline.json (0.36 solves/s on one process)",
        }
        result["offset_match"]["gpu_equals_cpu_oracle_on_sample"] = bool(agree)
        # SURVEY 8(d) baseline (ii): the same restatement on many host cores at once (separate process: it
        # forks workers, which must not happen in a process that has initialised the GPU runtime)
        try:
            usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            try:  # cgroup v2 CPU quota of this container, if any
                quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
                if quota != "max":
                    usable = min(usable, max(1, int(int(quota) / int(period))))
            except (OSError, ValueError):
                pass
            runs_par = []
            for procs in sorted({max(1, min(64, usable // 2 if usable > 2 else usable)), max(1, min(64, usable))}):
                per = max(2, (16 + procs - 1) // procs)  # at least 16 solves per process count
                out = subprocess.run([sys.executable, "-m", "oracle.cpu_parallel_baseline", str(procs), str(per), str(args.duration)],
                                     cwd=ROOT, capture_output=True, text=True, timeout=300,
                                     env=dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1"))
                par = json.loads(out.stdout.strip().splitlines()[-1])
                runs_par.append({"value": par["value"], "cores": par["cores"], "solves": par["solves"],
                                 "mean_solve_s_per_process": par["mean_solve_s"],
                                 "ratios_recovered": "%d/%d" % (par["recovered"], par["solves"])})
            best = max(runs_par, key=lambda r: r["value"])
            result["cpu_baseline"]["parallel"] = {
                "value": best["value"], "unit": "7-ratio solves/s", "cores": best["cores"], "usable_cpus": usable,
                "runs": runs_par,
                "sample": "same restatement, one process per core, >= 16 solves per process count (half and all of the %d "
                          "CPUs this container may use); the best is reported" % usable,
            }
        except Exception as exc:  # a baseline figure must never take the bench line down
            result["cpu_baseline"]["parallel"] = {"error": repr(exc)[:200]}

    if args.full and rank == 0 and world == 1 and not args.no_vad and not args.skip_secondary:
        result["vad"] = vad_figures(torch, _native)
    if args.full and rank == 0 and world == 1 and args.e2e_files > 0 and not args.skip_secondary:
        try:
            result["end_to_end"] = e2e_figures(torch, _native, args.e2e_files)
        except Exception as exc:  # e.g. not enough pinnable host memory on the box
            result["end_to_end"] = {"error": repr(exc)[:300]}

    if use_dist and args.full:
        # every rank's records arrived, in rank order
        mine = gathered[rank * per * 24:(rank + 1) * per * 24]
        assert bool(torch.equal(mine, pair_out)), "all-gathered records differ from the local ones"
        if rank == 0:
            allp = gathered.cpu().numpy().view(_native.PAIR_RESULT_DTYPE)
            result["gathered_records"] = int(allp.size)
            result["gathered_best_cand_valid"] = int((allp["best_cand"][: (args.pairs if strong else world * per)] >= 0).sum())
    if use_dist:
        if comm is not None:
            comm.close()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes a version banner to the C stdout when a communicator is created; push it out first so
        # that the JSON record is the LAST line of the output
        try:
            import ctypes

            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        emit(result)


if __name__ == "__main__":
    main()
