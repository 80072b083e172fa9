"""The steady-run gate behind the adaptive VAD (ffs_vad_steady_gate) as a model: the sequential definition,
a vectorised restatement, the kernels' decomposition into tiles, summaries and carries restated in Python (so the scan
algebra is pinned on the CPU), and the case tables of tests/test_gpu_steady_gate.py.  Integers only."""
import numpy as np

NO_QUIET, ALL_REJECTED, TOO_LONG = 1, 2, 4
FIELDS = ("threshold_bin", "flags", "n_stretches", "n_rejected", "longest_run", "reserved", "n_frames", "n_active", "n_kept")
MAX_FRAMES = 1 << 23
TILE = 4096   # GATE_TILE of csrc/ffs_vad_gate.h
WS_PER_TILE = 56


def classes(levels, t, dip_bins):
    lv = np.asarray(levels, np.uint8).astype(np.int64)
    return lv >= int(t), lv < int(t) - int(dip_bins)


def record(t, dip_bins, n, lengths=(), kept_frames=0, n_active=0, max_run=1, too_long=False):
    flags = (NO_QUIET if int(t) - int(dip_bins) <= 0 else 0) | (TOO_LONG if too_long else 0)
    if n_active > 0 and kept_frames == 0:
        flags |= ALL_REJECTED
    return dict(threshold_bin=int(t), flags=flags, n_stretches=len(lengths), n_rejected=sum(1 for x in lengths if x > max_run),
                longest_run=max(lengths) if len(lengths) else 0, reserved=0, n_frames=int(n), n_active=int(n_active),
                n_kept=int(kept_frames))


def gate_sequential(levels, t, dip_bins, max_run):
    """(speech flags, record): the definition, one frame after the other."""
    active, quiet = classes(levels, t, dip_bins)
    n = active.size
    if n > MAX_FRAMES:
        return active.copy(), record(t, dip_bins, n, too_long=True)
    speech, lengths, state, b, e = np.zeros(n, bool), [], False, 0, 0
    for i in range(n + 1):
        if i == n or quiet[i]:
            if state:  # a fall, or the end of the file inside a stretch
                lengths.append(e - b + 1)
                if e - b + 1 <= max_run:
                    speech[b:e + 1] = active[b:e + 1]
                state = False
        elif active[i]:
            if not state:
                state, b = True, i
            e = i
    return speech, record(t, dip_bins, n, lengths, int(speech.sum()), int(active.sum()), max_run)


def gate_vectorised(levels, t, dip_bins, max_run):
    """The same from positions of the last setter: maximum.accumulate forward for the rise, backward for the end."""
    active, quiet = classes(levels, t, dip_bins)
    n = active.size
    if n > MAX_FRAMES:
        return active.copy(), record(t, dip_bins, n, too_long=True)
    if n == 0:
        return active.copy(), record(t, dip_bins, 0)
    idx = np.arange(n)
    last_q = np.maximum.accumulate(np.where(quiet, idx, -1))          # last quiet frame at or before i
    last_a = np.maximum.accumulate(np.where(active, idx, -1))         # last active frame at or before i
    prev_q, prev_a = np.concatenate([[-1], last_q[:-1]]), np.concatenate([[-1], last_a[:-1]])
    rise = active & (prev_a <= prev_q)                                # the last setter in front is quiet, or there is none
    b = np.maximum.accumulate(np.where(rise, idx, -1))                # the rise of the stretch an active frame lies in
    next_q = np.minimum.accumulate(np.where(quiet, idx, n)[::-1])[::-1]   # first quiet frame at or behind i
    e = last_a[next_q - 1]                                            # the last active frame in front of it
    length = e - b + 1
    speech = active & (length <= max_run)
    lengths = length[rise]
    return speech, record(t, dip_bins, n, [int(x) for x in lengths], int(speech.sum()), int(active.sum()), max_run)


# ---- the kernels' decomposition (csrc/ffs_vad_gate.h), with any tile and thread width ----------------------------------

GF_ID, GF_QUIET, GF_SINCE, GF_OPEN = 0, 1, 2, 3


def fwd_op(f, g):
    gk, fk = g & 3, f & 3
    if gk == GF_ID:
        return f
    if gk != GF_OPEN or fk == GF_ID:
        return g
    return (g & ~3) | GF_SINCE if fk == GF_QUIET else f


def bwd_op(right, left):
    if left & 1:
        return left
    return (max(left >> 1, right >> 1) << 1) | (right & 1)


def _thread_summary(a, q, pos0):
    qs, as_ = np.flatnonzero(q), np.flatnonzero(a)
    after = as_[as_ > qs[-1]] if qs.size else as_
    if after.size:
        fwd = ((pos0 + int(after[0])) << 2) | (GF_SINCE if qs.size else GF_OPEN)
    else:
        fwd = GF_QUIET if qs.size else GF_ID
    front = as_[as_ < qs[0]] if qs.size else as_
    la = pos0 + int(front[-1]) if front.size else -1
    return fwd, ((la + 1) << 1) | (1 if qs.size else 0)


def _walk(a, q, pos0, pre, suf, max_run):
    o = dict(kept=np.zeros(a.size, bool), fa_head=-1, head_cnt=0, tail_la=-1, tail_cnt=0, n_str=0, n_rej=0, longest=0, n_kept=0)
    st = dict(kind=pre & 3, p=pre >> 2, la=-1, mask=[], rise=False)

    def close(e, known):
        cnt = len(st["mask"])
        if st["kind"] == GF_OPEN:
            o["head_cnt"] += cnt
        elif not known:
            o["tail_cnt"] += cnt
            o["tail_la"] = e
        else:
            ln = e - st["p"] + 1
            if ln <= max_run:
                o["n_kept"] += cnt
                o["kept"][st["mask"]] = True
            if st["rise"]:
                o["n_str"] += 1
                o["n_rej"] += ln > max_run
                o["longest"] = max(o["longest"], ln)
        st["mask"], st["rise"] = [], False

    for j in range(a.size):
        if a[j]:
            if st["kind"] == GF_ID:
                st["kind"], st["p"] = GF_OPEN, pos0 + j
                o["fa_head"] = pos0 + j
            elif st["kind"] == GF_QUIET:
                st["kind"], st["p"], st["rise"] = GF_SINCE, pos0 + j, True
            st["mask"].append(j)
            st["la"] = pos0 + j
        elif q[j]:
            if st["mask"]:
                close(st["la"], True)
            st["kind"] = GF_QUIET
    if st["mask"]:
        close(max(st["la"], (suf >> 1) - 1), bool(suf & 1))
    return o


def _tile_threads(active, quiet, tile0, tile, fpt):
    out = []
    for f0 in range(tile0, tile0 + tile, fpt):
        a, q = active[f0:f0 + fpt], quiet[f0:f0 + fpt]
        out.append((a, q, f0) + _thread_summary(a, q, f0))
    return out


def _scans(threads, first, last):
    """Per thread: the forward function of everything in front (behind `first`), the backward pair of everything behind."""
    pre, suf, run = [], [None] * len(threads), first
    for th in threads:
        pre.append(run)
        run = fwd_op(run, th[3])
    runb = last
    for k in range(len(threads) - 1, -1, -1):
        suf[k] = runb
        runb = bwd_op(runb, threads[k][4])
    return pre, suf, run, runb


def gate_tiled(levels, t, dip_bins, max_run, tile=TILE, fpt=16):
    """(speech flags, record) the way the three kernels compute them: per-tile summaries with the undecided head and
    tail, one carry pass over the summaries, the labels per tile with the carries composed in."""
    active, quiet = classes(levels, t, dip_bins)
    n = active.size
    if n > MAX_FRAMES:
        return active.copy(), record(t, dip_bins, n, too_long=True)
    n_tiles = -(-n // tile)
    tiles = []
    for k in range(n_tiles):   # k_gate_tiles
        threads = _tile_threads(active, quiet, k * tile, tile, fpt)
        pre, suf, fwd_all, bwd_all = _scans(threads, 0, 0)
        s = dict(fwd=fwd_all, bwd=bwd_all, fa_head=-1, head_cnt=0, tail_la=-1, tail_cnt=0, n_str=0, n_rej=0, longest=0, kept=0,
                 n_active=int(active[k * tile:(k + 1) * tile].sum()))
        for th, p, u in zip(threads, pre, suf):
            o = _walk(th[0], th[1], th[2], p, u, max_run)
            for name in ("head_cnt", "tail_cnt", "n_str", "n_rej"):
                s[name] += o[name]
            s["kept"] += o["n_kept"]
            for name in ("fa_head", "tail_la", "longest"):
                s[name] = max(s[name], o[name])
        tiles.append(s)
    # k_gate_carry
    entry, run = [], GF_QUIET
    for s in tiles:
        entry.append(run)
        run = fwd_op(run, s["fwd"])
    exits, runb = [None] * n_tiles, 0
    for k in range(n_tiles - 1, -1, -1):
        exits[k] = runb | 1
        runb = bwd_op(runb, tiles[k]["bwd"])
    n_active = n_kept = n_str = n_rej = longest = 0
    for s, c_in, c_out in zip(tiles, entry, exits):
        behind = (c_out >> 1) - 1
        n_active, n_kept, n_str, n_rej, longest = (n_active + s["n_active"], n_kept + s["kept"], n_str + s["n_str"], n_rej + s["n_rej"],
                                                   max(longest, s["longest"]))
        if s["head_cnt"] > 0:
            opened = (c_in & 3) == GF_SINCE
            b = c_in >> 2 if opened else s["fa_head"]
            la = (s["bwd"] >> 1) - 1
            ln = (la if s["bwd"] & 1 else max(la, behind)) - b + 1
            n_kept += s["head_cnt"] if ln <= max_run else 0
            if not opened:
                n_str, n_rej, longest = n_str + 1, n_rej + (ln > max_run), max(longest, ln)
        if s["tail_cnt"] > 0:
            ln = max(s["tail_la"], behind) - (s["fwd"] >> 2) + 1
            n_kept += s["tail_cnt"] if ln <= max_run else 0
            n_str, n_rej, longest = n_str + 1, n_rej + (ln > max_run), max(longest, ln)
    rec = record(t, dip_bins, n, (), n_kept, n_active, max_run)
    rec.update(n_stretches=n_str, n_rejected=n_rej, longest_run=longest)
    # k_gate_labels
    speech = np.zeros(n_tiles * tile, bool)
    for k in range(n_tiles):
        threads = _tile_threads(active, quiet, k * tile, tile, fpt)
        pre, suf, _, _ = _scans(threads, entry[k], exits[k])
        for th, p, u in zip(threads, pre, suf):
            o = _walk(th[0], th[1], th[2], p, u, max_run)
            speech[th[2]:th[2] + th[0].size] = o["kept"]
    return speech[:n], rec


def remove_long_runs(ones, max_run):
    """`ones` without every run of ones longer than max_run: what the gate is at dip_bins = 0."""
    ones = np.asarray(ones, bool)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], ones.astype(np.int8), [0]])))
    out = ones.copy()
    for s, e in zip(edges[::2], edges[1::2]):
        if e - s > max_run:
            out[s:e] = False
    return out


def record_tuple(rec):
    return tuple(int(rec[f]) for f in FIELDS)


def workspace_bytes(n):
    return 0 if n <= 0 or n > MAX_FRAMES else -(-n // TILE) * WS_PER_TILE


# ---- case tables ---------------------------------------------------------------------------------------------------
# Levels use three values around t = 100: A = 120 (active), K = 95 (a keep frame at dip_bins >= 5, quiet below), Q = 10.
A, K, Q = 120, 95, 10
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 1)
OFFSETS = (0, 1, 3)


def _fill(n, base, *spans):
    lv = np.full(n, base, np.uint8)
    for s, e, v in spans:
        lv[s:e] = v
    return lv


def random_levels(rng, n, p_run=0.05):
    """Runs of A / K / Q frames with geometric lengths: stretches of every length up to a few hundred frames."""
    runs = np.maximum(1, rng.geometric(p_run, size=int(3 * n * p_run) + 64))
    out = np.repeat(rng.choice(np.array([A, K, Q], np.uint8), size=runs.size, p=[0.5, 0.3, 0.2]), runs)[:n]
    assert out.size == n
    return out


def stretch_cases():
    """(name, levels, t, dip_bins, max_run): stretches against tile edges, with t = 100."""
    T = TILE
    c = [
        ("rise on a tile's last frame, fall on the next one's first", _fill(2 * T + 5, Q, (T - 1, T, A)), 100, 0, 1),
        ("rise on the last frame, active first frame, fall on the second", _fill(2 * T + 5, Q, (T - 1, T + 1, A)), 100, 0, 1),
        ("across three tiles of keep frames", _fill(5 * T + 9, Q, (T - 3, T, A), (T, 4 * T, K), (4 * T, 4 * T + 2, A)), 100, 10, 3 * T + 5),
        ("the same, one frame too long", _fill(5 * T + 9, Q, (T - 3, T, A), (T, 4 * T, K), (4 * T, 4 * T + 2, A)), 100, 10, 3 * T + 4),
        ("across three all-active tiles", _fill(5 * T + 9, Q, (T - 3, 4 * T + 2, A)), 100, 0, 3 * T + 5),
        ("starts active", _fill(T + 40, Q, (0, 30, A), (50, 60, A)), 100, 0, 29),
        ("ends inside an open stretch", _fill(T + 40, Q, (T - 10, T + 40, A)), 100, 0, 50),
        ("ends inside an open stretch, too long", _fill(T + 40, Q, (T - 10, T + 40, A)), 100, 0, 49),
        ("ends in keep frames of an open stretch", _fill(T + 40, Q, (T - 10, T + 20, A), (T + 20, T + 40, K)), 100, 10, 30),
        ("all keep", _fill(T + 17, K), 100, 10, 5),
        ("all active", _fill(2 * T + 17, A), 100, 0, 2 * T + 17),
        ("all active, too long", _fill(2 * T + 17, A), 100, 0, 2 * T + 16),
        ("all quiet", _fill(T + 17, Q), 100, 0, 5),
        ("trailing keep frames before a fall, fall before the edge", _fill(2 * T, Q, (T - 20, T - 10, A), (T - 10, T - 1, K)), 100, 10, 10),
        ("trailing keep frames over the edge", _fill(2 * T, Q, (T - 20, T - 10, A), (T - 10, T + 9, K)), 100, 10, 10),
        ("trailing keep frames over the edge, one active frame too many", _fill(2 * T, Q, (T - 21, T - 10, A), (T - 10, T + 9, K)), 100, 10, 10),
        ("keep frames up to the edge, fall on the next tile's first", _fill(2 * T, Q, (T - 20, T - 10, A), (T - 10, T, K)), 100, 10, 10),
        ("exactly max_run", _fill(300, Q, (10, 110, A)), 100, 0, 100),
        ("max_run + 1", _fill(300, Q, (10, 111, A)), 100, 0, 100),
        ("max_run 1", _fill(300, Q, (10, 11, A), (20, 22, A), (30, 31, A), (31, 32, K), (32, 33, A)), 100, 0, 1),
        ("max_run 1 with keep frames inside", _fill(300, Q, (10, 11, A), (30, 31, A), (31, 32, K), (32, 33, A)), 100, 10, 1),
        ("dip one below t", _fill(300, 0, (10, 40, A), (40, 50, 1), (50, 60, A), (70, 80, A)), 100, 99, 50),
        ("dip t: NO_QUIET", _fill(300, 0, (10, 40, A), (50, 60, A)), 100, 100, 50),
        ("dip 255: NO_QUIET", _fill(300, 0, (10, 40, A), (50, 60, A)), 100, 255, 51),
        ("t 0: all active, NO_QUIET", _fill(300, 0, (10, 40, A)), 0, 0, 300),
        ("t 0 too long: ALL_REJECTED", _fill(300, 0, (10, 40, A)), 0, 0, 299),
        ("t 256: nothing active", _fill(300, 255), 256, 0, 5),
        ("t 256 with a dip", _fill(300, 255, (5, 9, 0)), 256, 1, 5),
    ]
    rng = np.random.RandomState(27)
    for k, n in enumerate((T + 1, 2 * T - 1, 3 * T + 5)):
        c.append(("random %d" % n, random_levels(rng, n), 100, (0, 10, 90)[k], (40, 64, 200)[k]))
    return c


def scan_cases():
    """65 and 257 tiles plus 17 frames: the carry scan passes one wave, and one trip of the workgroup.  Long stretches of
    keep frames carry a state through hundreds of summaries; the random part decides most tiles' heads and tails."""
    out = []
    rng = np.random.RandomState(28)
    for tiles in (65, 257):
        n, first = tiles * TILE + 17, max(3, tiles - 70)
        lv = random_levels(rng, n, 0.002)
        lv[first * TILE + 3] = lv[(tiles - 1) * TILE + 4] = Q
        lv[first * TILE + 4: first * TILE + 8] = A
        lv[first * TILE + 8: (tiles - 1) * TILE + 3] = K   # one stretch carried over a wave's and a trip's last summary ...
        lv[(tiles - 1) * TILE + 3] = A                     # ... that ends on an active frame in the last whole tile
        out.append((tiles, lv, 100, 10, 3000))
        out.append((tiles, lv, 100, 10, (tiles - 1 - first) * TILE))   # the carried stretch is exactly max_run long
    return out


def tone_file(frame_len=160, seed=5):
    """int16 PCM of a synthetic file: a noise floor, speech bursts of 0.3 .. 3 s separated by pauses, and one steady tone
    of 14 s with a burst of speech against each end; 40 s at 100 frames per second, a short last frame."""
    rng = np.random.RandomState(seed)
    n_frames = 4000
    amp = np.full(n_frames, 20.0)
    f = 50
    while f < n_frames - 400:
        ln = int(rng.randint(30, 300))
        if f + ln < 1300 or f >= 3000:   # a second of pause on either side of the tone
            amp[f:f + ln] = rng.uniform(2000.0, 6000.0)
        f += ln + int(rng.randint(20, 120))
    x = rng.standard_normal((n_frames, frame_len)) * amp[:, None]
    tone = 5000.0 * np.sin(2 * np.pi * 440.0 * np.arange(n_frames * frame_len) / (100.0 * frame_len)).reshape(n_frames, frame_len)
    x[1500:2900] = tone[1500:2900] + rng.standard_normal((1400, frame_len)) * 20.0
    x[1470:1500] = rng.standard_normal((30, frame_len)) * 4000.0   # speech that abuts the tone: dropped with it
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).ravel()[:-57], (1500, 2900)


# ---- refusals of the two exports -----------------------------------------------------------------------------------


def refusal_calls():
    """(keyword overrides of a valid call, a fragment of the message).  Pointers are never dereferenced: each call fails
    its checks first."""
    return [
        (dict(n=-1), b"negative"),
        (dict(thr_host=-1), b"threshold_host=-1 outside"),
        (dict(thr_host=257), b"threshold_host=257 outside"),
        (dict(dip=-1), b"dip_bins=-1 outside"),
        (dict(dip=256), b"dip_bins=256 outside"),
        (dict(max_run=0), b"max_run=0 outside"),
        (dict(max_run=1 << 31), b"max_run=2147483648 outside"),
        (dict(levels=None), b"null levels or record"),
        (dict(record=None), b"null levels or record"),
        (dict(thr_dev=0x1002), b"misaligned"),
        (dict(labels=0x1002), b"misaligned"),
        (dict(record=0x1004), b"misaligned"),
        (dict(ws=0x1004), b"misaligned"),
        (dict(ws_bytes=2 * WS_PER_TILE - 1), b"workspace of 111 bytes, 112 needed"),
        (dict(ws=None), b"workspace"),
        (dict(n=MAX_FRAMES, ws_bytes=2047 * WS_PER_TILE), b"workspace of 114632 bytes, 114688 needed"),
    ]


def check_refusals(lib):
    """Every refusal of ffs_vad_steady_gate with its message, before any launch (no device needed), and the workspace
    sizes of ffs_vad_steady_gate_workspace_bytes."""
    base = dict(levels=0x1000, n=TILE + 1, thr_dev=None, thr_host=100, dip=0, max_run=1000, label=0.0, labels=0x2000, bits=0x3000,
                record=0x4000, ws=0x5000, ws_bytes=2 * WS_PER_TILE)
    for over, fragment in refusal_calls():
        a = dict(base)
        a.update(over)
        rc = lib.ffs_vad_steady_gate(a["levels"], a["n"], a["thr_dev"], a["thr_host"], a["dip"], a["max_run"], a["label"], a["labels"],
                                     a["bits"], a["record"], a["ws"], a["ws_bytes"], None)
        assert rc == -1 and fragment in lib.ffs_last_error(), (over, rc, lib.ffs_last_error())
    for n in (-5, 0, 1, TILE, TILE + 1, MAX_FRAMES, MAX_FRAMES + 1):
        assert lib.ffs_vad_steady_gate_workspace_bytes(n) == workspace_bytes(n), n
