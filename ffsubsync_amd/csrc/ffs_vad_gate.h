// ffs_vad_gate.h -- steady-run gate behind the adaptive energy VAD (gfx950): the device side of
// adaptive_vad.steady_gate.  An energy rule labels music, hum and hiss as speech; a person does not talk
// for ten seconds without one 10 ms frame falling below the file's threshold, and no subtitle cue is longer than that,
// so a stretch of uninterrupted activity longer than max_run frames is dropped whole.  Integers only, pinned bit for
// bit against tests/steady_gate_model.py.  Contract (include/ffsubsync_amd.h, ffs_vad_steady_gate):
//   active(i) = level[i] >= t;  quiet(i) = (int)level[i] < t - dip_bins;  every other frame is a KEEP frame
//   s[i]      = class of the last active or quiet frame (a SETTER) at or before i, s[-1] = quiet
//   a stretch opens at a rise (i active, s[i-1] quiet), closes at the next fall (i quiet, s[i-1] active) or at the end of
//   the file; its extent is [b, e], b the rise, e the last active frame before the fall; speech(f) = active(f) and
//   e - b + 1 <= max_run for the stretch f lies in.
//
// A stretch can span the file, so the state is carried over the whole of it -- by three ORDERED LAUNCHES on the
// caller's stream, never by one workgroup waiting for another (no look-back, no flags, no cooperative grid):
//
// k_gate_tiles: one workgroup of 256 threads per tile of GATE_TILE = 4096 frames, a thread takes 16 level bytes (one
// 16-byte load where the address allows and all 16 frames exist, else byte by byte) and classifies them into a 16-bit
// active and a 16-bit quiet word.  What a run of frames does to the state is a FUNCTION of four kinds -- identity (no
// setter), "quiet", "active since p" (a quiet frame, then a rise at p) and "open at p" (no quiet frame: stays what it
// was if that was active, else active since p) -- closed under composition, packed into one int (p << 2 | kind) and
// scanned forward over the threads with the tokenizer's DPP wave scan.  The backward scan carries (a quiet frame
// exists, last active frame in front of the first quiet one), packed as (la + 1) << 1 | has_quiet.  With both a thread
// walks its 16 frames once and closes every PIECE (its active frames of one stretch): a piece whose rise follows a quiet
// frame of the tile and whose end precedes one is INTERIOR and decided here; the pieces in front of the tile's first
// quiet frame (HEAD) and behind its last (TAIL) belong to stretches that other tiles share.  The tile's summary (48
// bytes): the two packed scan totals, the head's first active frame and active count, the tail's last active frame and
// count (its rise is the forward total's p), and the interior's stretches, rejected stretches, longest run and kept
// frames, and the tile's active count.
//
// k_gate_carry: ONE workgroup scans the summaries, 256 per trip with a running carry: forward gives the state at each
// tile's entry (quiet, or active since b), backward the last active frame of the stretch open at each tile's exit.
// Both go to the workspace in the packed forms above.  A third loop decides each tile's head and tail, counts a stretch
// at the tile of its rise, and the workgroup's integer sums and maxima become the 48-byte record: no atomics, nothing
// depends on arrival order.  With no tiles (n_frames == 0, or more than VAD_MAX_FRAMES: the gate is skipped and
// k_vad_level_labels writes the outputs) it writes the record alone.
//
// k_gate_labels: k_gate_tiles' load, scans and walk again with the tile's entry state composed in front of the forward
// scan and its exit in front of the backward one, so every piece is decided; the 16-bit kept words go through LDS and
// leave as k_vad_level_labels' two forms: fp32 labels a frame a lane, coalesced, and the packed bits from the waves'
// ballots, a byte from each of lanes 0..7.  The unused high bits of the last byte are 0, nothing is written behind it.
#pragma once
#include "ffs_adaptive_vad.h"

namespace ffsa {

constexpr int GATE_TILE = 4096;                    // frames of a workgroup of k_gate_tiles / k_gate_labels
constexpr int GATE_THREADS = 256;
constexpr int GATE_FPT = GATE_TILE / GATE_THREADS;  // 16 frames (one 16-byte load) per thread
constexpr int32_t VAD_GATE_NO_QUIET = 1;            // FFS_VAD_GATE_NO_QUIET
constexpr int32_t VAD_GATE_ALL_REJECTED = 2;        // FFS_VAD_GATE_ALL_REJECTED
constexpr int32_t VAD_GATE_TOO_LONG = 4;            // FFS_VAD_GATE_TOO_LONG
static_assert(GATE_FPT == 16 && GATE_THREADS % 64 == 0, "a thread owns one 16-byte load of levels");
static_assert(VAD_MAX_FRAMES < (1ll << 28), "frame positions are packed into an int above two kind bits");

struct VadGate {  // = ffs_vad_gate
    int32_t threshold_bin, flags, n_stretches, n_rejected, longest_run, reserved;
    int64_t n_frames, n_active, n_kept;
};
static_assert(sizeof(VadGate) == 48, "VadGate must match ffs_vad_gate");

struct GateTile {  // a tile's summary, written by k_gate_tiles, read by k_gate_carry
    int32_t fwd;       // what the tile does to the state: p << 2 | kind
    int32_t bwd;       // (last active frame in front of the tile's first quiet frame + 1) << 1 | the tile has a quiet frame
    int32_t fa_head;   // first active frame in front of the first quiet frame, -1: none
    int32_t head_cnt;  // active frames in front of the first quiet frame
    int32_t tail_la;   // last active frame behind the last quiet frame, -1: none
    int32_t tail_cnt;  // active frames behind the last quiet frame (0 in a tile without one: they are the head)
    int32_t n_str, n_rej, longest, kept;  // interior stretches, those longer than max_run, the longest, their kept frames
    int32_t n_active, reserved;
};
static_assert(sizeof(GateTile) == 48, "12 ints");
constexpr int GATE_WS_PER_TILE = (int)sizeof(GateTile) + 8;  // + the tile's entry state and exit, two packed ints

// kinds of a state function; as a STATE (a function applied to a known state) only GF_QUIET and GF_SINCE occur
constexpr int GF_ID = 0, GF_QUIET = 1, GF_SINCE = 2, GF_OPEN = 3;

// f then g (f the earlier frames); 0 (GF_ID) is the identity on both sides
FFS_DEV int gate_fwd_op(int f, int g) {
    const int gk = g & 3, fk = f & 3;
    if (gk == GF_ID) return f;
    if (gk != GF_OPEN || fk == GF_ID) return g;
    return fk == GF_QUIET ? (g & ~3) | GF_SINCE : f;
}
// the backward pair of `left` frames followed by `right` frames, `right` scanned first; 0 is the identity
FFS_DEV int gate_bwd_op(int right, int left) {
    if (left & 1) return left;
    const int a = left >> 1, b = right >> 1;
    return ((a > b ? a : b) << 1) | (right & 1);
}

// inclusive scan over the 64 lanes from lane 63 DOWN; op(scanned earlier = higher lane, this lane)
template <class Op>
FFS_DEV int gate_wave_incl_scan_down(int v, Op op, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_down(v, d, 64);
        if (lane + d < 64) v = op(o, v);
    }
    return v;
}

// EXCLUSIVE scans of one packed value per thread over the GATE_THREADS threads; *total: all of them.  s_w: one int per
// wave, free again on return (the closing barrier).
FFS_DEV int gate_block_excl_fwd(int v, int* s_w, int lane, int wave, int* total) {
    const int incl = tok_wave_incl_scan(v, 0, [](int f, int g) { return gate_fwd_op(f, g); });
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int pre = 0, all = 0;
#pragma unroll
    for (int w = 0; w < GATE_THREADS / 64; ++w) {
        const int x = s_w[w];
        if (w < wave) pre = gate_fwd_op(pre, x);
        all = gate_fwd_op(all, x);
    }
    __syncthreads();
    const int up = __shfl_up(incl, 1, 64);
    *total = all;
    return gate_fwd_op(pre, lane ? up : 0);
}
FFS_DEV int gate_block_excl_bwd(int v, int* s_w, int lane, int wave, int* total) {
    const int incl = gate_wave_incl_scan_down(v, [](int r, int l) { return gate_bwd_op(r, l); }, lane);
    if (lane == 0) s_w[wave] = incl;
    __syncthreads();
    int pre = 0, all = 0;
#pragma unroll
    for (int w = GATE_THREADS / 64 - 1; w >= 0; --w) {
        const int x = s_w[w];
        if (w > wave) pre = gate_bwd_op(pre, x);
        all = gate_bwd_op(all, x);
    }
    __syncthreads();
    const int down = __shfl_down(incl, 1, 64);
    *total = all;
    return gate_bwd_op(pre, lane < 63 ? down : 0);
}

// the thread's 16 frames as an active and a quiet bit word (bit j: frame f0 + j; a frame behind the file is neither)
FFS_DEV void gate_classify(const unsigned char* __restrict__ levels, long long n_frames, long long f0, int thr, int quiet_below,
                           unsigned* active, unsigned* quiet) {
    unsigned a = 0, q = 0;
    if (f0 + GATE_FPT <= n_frames && (reinterpret_cast<uintptr_t>(levels + f0) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(levels + f0);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lv = (int)((w[k] >> (8 * i)) & 255u);
                a |= (unsigned)(lv >= thr) << (4 * k + i);
                q |= (unsigned)(lv < quiet_below) << (4 * k + i);
            }
    } else {
        for (int j = 0; j < GATE_FPT && f0 + j < n_frames; ++j) {
            const int lv = (int)levels[f0 + j];
            a |= (unsigned)(lv >= thr) << j;
            q |= (unsigned)(lv < quiet_below) << j;
        }
    }
    *active = a;
    *quiet = q;
}

// what the thread's frames do to the state (forward) and the backward pair, from its two bit words at frame pos0
FFS_DEV void gate_thread_summary(unsigned a, unsigned q, int pos0, int* fwd, int* bwd) {
    const int lq = q ? 31 - __builtin_clz(q) : -1;                 // last quiet frame
    const unsigned a_after = lq >= 0 ? a & (~1u << lq) : a;         // active frames behind it
    if (a_after)
        *fwd = ((pos0 + __builtin_ctz(a_after)) << 2) | (q ? GF_SINCE : GF_OPEN);
    else
        *fwd = q ? GF_QUIET : GF_ID;
    const unsigned a_front = q ? a & ((1u << __builtin_ctz(q)) - 1u) : a;  // active frames in front of the first quiet one
    const int la = a_front ? pos0 + 31 - __builtin_clz(a_front) : -1;
    *bwd = ((la + 1) << 1) | (q ? 1 : 0);
}

struct GateWalk {
    unsigned kept_mask;  // the thread's active frames in kept stretches (decided pieces only)
    int fa_head, head_cnt, tail_la, tail_cnt, n_str, n_rej, longest, kept;
};

// One pass over the thread's 16 frames: `pre` is the state function of everything in front of them, `suf` the backward
// pair of everything behind.  With a known state in front (GF_QUIET / GF_SINCE) and a closed pair behind (bit 0 set)
// every piece is decided; else the undecided ones are counted as the tile's head and tail.
FFS_DEV GateWalk gate_walk(unsigned a, unsigned q, int pos0, int pre, int suf, int max_run) {
    GateWalk o = {0u, -1, 0, -1, 0, 0, 0, 0, 0};
    int kind = pre & 3, p = pre >> 2, la = -1;
    unsigned mask = 0;
    bool rise = false;
    auto close = [&](int e, bool e_known) {
        const int cnt = __builtin_popcount(mask);
        if (kind == GF_OPEN) {
            o.head_cnt += cnt;
        } else if (!e_known) {
            o.tail_cnt += cnt;
            o.tail_la = e;
        } else {
            const int len = e - p + 1;
            const bool ok = len <= max_run;
            if (ok) {
                o.kept += cnt;
                o.kept_mask |= mask;
            }
            if (rise) {
                o.n_str += 1;
                o.n_rej += ok ? 0 : 1;
                o.longest = len > o.longest ? len : o.longest;
            }
        }
        mask = 0;
        rise = false;
    };
#pragma unroll
    for (int j = 0; j < GATE_FPT; ++j) {
        if ((a >> j) & 1u) {
            if (kind == GF_ID) {
                kind = GF_OPEN;
                p = pos0 + j;
                o.fa_head = p;
            } else if (kind == GF_QUIET) {
                kind = GF_SINCE;
                p = pos0 + j;
                rise = true;
            }
            mask |= 1u << j;
            la = pos0 + j;
        } else if ((q >> j) & 1u) {
            if (mask) close(la, true);
            kind = GF_QUIET;
        }
    }
    if (mask) {
        const int behind = (suf >> 1) - 1;
        close(la > behind ? la : behind, (suf & 1) != 0);
    }
    return o;
}

FFS_DEV int gate_wave_sum(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}
FFS_DEV int gate_wave_max(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(GATE_THREADS) void k_gate_tiles(const unsigned char* __restrict__ levels, long long n_frames,
                                                             const int* __restrict__ thr_dev, int thr_host, int dip_bins,
                                                             int max_run, GateTile* __restrict__ tiles) {
    __shared__ int s_w[GATE_THREADS / 64];
    __shared__ int s_red[GATE_THREADS / 64][9];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int thr = thr_dev ? *thr_dev : thr_host;
    const long long f0 = (long long)blockIdx.x * GATE_TILE + (long long)threadIdx.x * GATE_FPT;
    unsigned a, q;
    gate_classify(levels, n_frames, f0, thr, thr - dip_bins, &a, &q);
    int fwd, bwd, fwd_all, bwd_all;
    gate_thread_summary(a, q, (int)f0, &fwd, &bwd);
    const int pre = gate_block_excl_fwd(fwd, s_w, lane, wave, &fwd_all);
    const int suf = gate_block_excl_bwd(bwd, s_w, lane, wave, &bwd_all);
    const GateWalk o = gate_walk(a, q, (int)f0, pre, suf, max_run);
    // sums and maxima over the workgroup (fa_head has one writer: a maximum over -1 elsewhere)
    const int sums[6] = {o.head_cnt, o.tail_cnt, o.n_str, o.n_rej, o.kept, (int)__builtin_popcount(a)};
    const int maxs[3] = {o.fa_head, o.tail_la, o.longest};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int s = gate_wave_sum(sums[k]);
        if (lane == 0) s_red[wave][k] = s;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int m = gate_wave_max(maxs[k]);
        if (lane == 0) s_red[wave][6 + k] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int r[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            r[k] = s_red[0][k];
#pragma unroll
            for (int w = 1; w < GATE_THREADS / 64; ++w) r[k] = k < 6 ? r[k] + s_red[w][k] : (s_red[w][k] > r[k] ? s_red[w][k] : r[k]);
        }
        GateTile t;
        t.fwd = fwd_all;
        t.bwd = bwd_all;
        t.head_cnt = r[0];
        t.tail_cnt = r[1];
        t.n_str = r[2];
        t.n_rej = r[3];
        t.kept = r[4];
        t.n_active = r[5];
        t.fa_head = r[6];
        t.tail_la = r[7];
        t.longest = r[8];
        t.reserved = 0;
        tiles[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(GATE_THREADS) void k_gate_carry(const GateTile* __restrict__ tiles, int n_tiles, long long n_frames,
                                                             const int* __restrict__ thr_dev, int thr_host, int dip_bins,
                                                             int max_run, int too_long, int2* __restrict__ carry,
                                                             VadGate* __restrict__ record) {
    __shared__ int s_w[GATE_THREADS / 64];
    __shared__ long long s_sum[GATE_THREADS / 64][4];
    __shared__ int s_max[GATE_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int thr = thr_dev ? *thr_dev : thr_host;
    const int trips = (n_tiles + GATE_THREADS - 1) / GATE_THREADS;
    // forward: the state at each tile's entry; the file starts quiet
    int run = GF_QUIET;
    for (int k = 0; k < trips; ++k) {
        const int i = k * GATE_THREADS + (int)threadIdx.x;
        int all;
        const int pre = gate_block_excl_fwd(i < n_tiles ? tiles[i].fwd : 0, s_w, lane, wave, &all);
        if (i < n_tiles) carry[i].x = gate_fwd_op(run, pre);
        run = gate_fwd_op(run, all);
    }
    // backward: the last active frame, in front of the next quiet one, behind each tile's exit; the end of the file
    // closes a stretch, so every pair is stored closed (bit 0 set)
    int runb = 0;
    for (int k = trips - 1; k >= 0; --k) {
        const int i = k * GATE_THREADS + (int)threadIdx.x;
        int all;
        const int suf = gate_block_excl_bwd(i < n_tiles ? tiles[i].bwd : 0, s_w, lane, wave, &all);
        if (i < n_tiles) carry[i].y = gate_bwd_op(runb, suf) | 1;
        runb = gate_bwd_op(runb, all);
    }
    // heads and tails: a stretch is counted at the tile of its rise, its frames at the tiles that hold them (a thread
    // reads back the carries it wrote itself: tile i is thread i % GATE_THREADS's in all three loops)
    long long n_active = 0, n_kept = 0, n_str = 0, n_rej = 0;
    int longest = 0;
    for (int i = (int)threadIdx.x; i < n_tiles; i += GATE_THREADS) {
        const GateTile t = tiles[i];
        const int2 c = carry[i];
        const int behind = (c.y >> 1) - 1;
        n_active += t.n_active;
        n_kept += t.kept;
        n_str += t.n_str;
        n_rej += t.n_rej;
        longest = t.longest > longest ? t.longest : longest;
        if (t.head_cnt > 0) {
            const bool open = (c.x & 3) == GF_SINCE;  // the head continues a stretch of an earlier tile
            const int b = open ? c.x >> 2 : t.fa_head;
            const int la = (t.bwd >> 1) - 1;
            const int e = (t.bwd & 1) ? la : (la > behind ? la : behind);
            const int len = e - b + 1;
            if (len <= max_run) n_kept += t.head_cnt;
            if (!open) {
                n_str += 1;
                n_rej += len <= max_run ? 0 : 1;
                longest = len > longest ? len : longest;
            }
        }
        if (t.tail_cnt > 0) {  // always behind a quiet frame of the tile: it holds its rise
            const int b = t.fwd >> 2;
            const int e = t.tail_la > behind ? t.tail_la : behind;
            const int len = e - b + 1;
            if (len <= max_run) n_kept += t.tail_cnt;
            n_str += 1;
            n_rej += len <= max_run ? 0 : 1;
            longest = len > longest ? len : longest;
        }
    }
    long long tot[4];
    wave_excl_scan(n_active, lane, &tot[0]);
    wave_excl_scan(n_kept, lane, &tot[1]);
    wave_excl_scan(n_str, lane, &tot[2]);
    wave_excl_scan(n_rej, lane, &tot[3]);
    longest = gate_wave_max(longest);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_sum[wave][k] = tot[k];
        s_max[wave] = longest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < GATE_THREADS / 64; ++w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tot[k] += s_sum[w][k];
            longest = s_max[w] > longest ? s_max[w] : longest;
        }
        VadGate r;
        r.threshold_bin = thr;
        r.flags = (thr - dip_bins <= 0 ? VAD_GATE_NO_QUIET : 0) | (too_long ? VAD_GATE_TOO_LONG : 0) |
                  (tot[0] > 0 && tot[1] == 0 ? VAD_GATE_ALL_REJECTED : 0);
        r.n_stretches = (int32_t)tot[2];
        r.n_rejected = (int32_t)tot[3];
        r.longest_run = longest;
        r.reserved = 0;
        r.n_frames = n_frames;
        r.n_active = tot[0];
        r.n_kept = tot[1];
        *record = r;
    }
}

__global__ __launch_bounds__(GATE_THREADS) void k_gate_labels(const unsigned char* __restrict__ levels, long long n_frames,
                                                              const int* __restrict__ thr_dev, int thr_host, int dip_bins,
                                                              int max_run, const int2* __restrict__ carry, float non_speech,
                                                              float* __restrict__ labels, unsigned char* __restrict__ bits) {
    __shared__ int s_w[GATE_THREADS / 64];
    __shared__ unsigned s_kept[GATE_THREADS];  // the threads' 16-bit kept words
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int thr = thr_dev ? *thr_dev : thr_host;
    const long long tile0 = (long long)blockIdx.x * GATE_TILE;
    const long long f0 = tile0 + (long long)threadIdx.x * GATE_FPT;
    const int2 c = carry[blockIdx.x];
    unsigned a, q;
    gate_classify(levels, n_frames, f0, thr, thr - dip_bins, &a, &q);
    int fwd, bwd, all;
    gate_thread_summary(a, q, (int)f0, &fwd, &bwd);
    const int pre = gate_fwd_op(c.x, gate_block_excl_fwd(fwd, s_w, lane, wave, &all));
    const int suf = gate_bwd_op(c.y, gate_block_excl_bwd(bwd, s_w, lane, wave, &all));
    s_kept[threadIdx.x] = gate_walk(a, q, (int)f0, pre, suf, max_run).kept_mask;
    __syncthreads();
    for (int base = wave * 64; base < GATE_TILE; base += GATE_THREADS) {  // a wave's 64 frames per trip: wave-uniform
        if (tile0 + base >= n_frames) break;
        const int i = base + lane;
        const long long f = tile0 + i;
        const bool speech = (s_kept[i >> 4] >> (i & 15)) & 1u;  // (0 behind the file: no frame there is active)
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(speech);
        if (labels && f < n_frames) labels[f] = speech ? 1.0f : non_speech;
        if (bits && lane < 8 && tile0 + base + 8 * lane < n_frames) bits[(tile0 + base) / 8 + lane] = (unsigned char)(mask >> (8 * lane));
    }
}

}  // namespace ffsa
