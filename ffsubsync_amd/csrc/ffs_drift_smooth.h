// ffs_drift_smooth.h -- smooth drift fit (gfx950): inside every segment of a drift solve, replace the DP's staircase by a
// polyline through a few knots whose lags are searched in a small radius around the path, scored on the same block
// counts and penalised only for BENDING.  The contract is this library's own, pinned against the numpy model
// tests/drift_smooth_model.py.
//
// Segment [f, e) of a pair (a maximal run of blocks with no jump inside, as ffs_drift_report.h), n = e - 1 - f.  A
// one-block segment is returned as it is.  Otherwise I = max(1, (n + M/2) / M) intervals, knot blocks k_i = f + i M for
// i < I and k_I = e - 1; interval i has n_i = k_{i+1} - k_i blocks and holds k_i <= b < k_{i+1}, the last one b = k_I too.
// Knot i may sit at c_i = o_{k_i} + u, u in [-R, R], where that lag is inside the window.  Block b of interval i gets the
// lag of the digital line d_b = c_i + floor((2 (c_{i+1} - c_i)(b - k_i) + n_i) / (2 n_i)).  Line score T_i(c_i, c_{i+1}):
// ov / n11 / n1x / nx1 of the interval's blocks at their lags summed in uint32 -- order-free -- then ONE split_mix, 0.0
// where the overlap is empty, -inf where an end is outside the window.  Bend cost at an interior knot:
// g = |D2 n_a - D1 n_b|, then ((lambda * g) * M) / (n_a n_b), every fp64 operation rounded on its own.  Viterbi over the
// state (c_{i-1}, c_i): V_1 = T_0, V_{i+1}(c_i, c_{i+1}) = max over c_{i-1} of (V_i - bend_i) + T_i.  Ties: candidates are
// tried in the order u = 0, +1, -1, +2, -2, ... and one replaces the best so far only when strictly greater -- over the
// predecessor at every step, over the final state with u_I as the outer and u_{I-1} as the inner loop.
//
// Three kernels after k_drift_dp (the counts and prefix popcounts are still in the workspace); nothing is read back:
//   k_smooth_intervals   one workgroup per pair: numbers the segments with a workgroup scan over the jump flags (wave
//                        ballots, as k_drift_segments), scans the segments' interval counts, then one thread per block
//                        writes the interval table, the knot flags and the path as the initial smooth offsets.
//   k_drift_line_sums    SMOOTH_LINE_GROUPS workgroups per pair, each taking every SMOOTH_LINE_GROUPS-th interval: a
//                        thread owns the lines q, q + 256, ... of the (2R+1)^2, neighbouring threads neighbouring
//                        c_{i+1} (neighbouring lags of one count row); the block's sample range and its n1x are
//                        wave-uniform, nx1 two prefix reads; four uint32 accumulators, one split_mix and one fp64 store
//                        per line.
//   k_drift_knot_dp      SMOOTH_DP_GROUPS workgroups per pair, each taking every SMOOTH_DP_GROUPS-th segment: the
//                        (2R+1)^2 Viterbi states in two LDS buffers, one back-pointer byte per state and interval to the
//                        workspace, thread 0's final maximum, backtrack and sums, then all threads write the segment's
//                        smooth offsets.
#pragma once
#include "ffs_drift.h"

namespace ffsa {

constexpr int SMOOTH_MAX_KNOT_BLOCKS = 256;      // FFS_SMOOTH_MAX_KNOT_BLOCKS
constexpr int SMOOTH_MAX_RADIUS = 16;            // FFS_SMOOTH_MAX_RADIUS
constexpr int SMOOTH_MAX_STATES = (2 * SMOOTH_MAX_RADIUS + 1) * (2 * SMOOTH_MAX_RADIUS + 1);  // 1089
constexpr int SMOOTH_INT_THREADS = 1024;         // k_smooth_intervals workgroup (one per pair)
constexpr int SMOOTH_LINE_THREADS = 256;         // k_drift_line_sums workgroup
constexpr int SMOOTH_LINE_GROUPS = 64;           // ... workgroups per pair
constexpr int SMOOTH_DP_THREADS = 256;           // k_drift_knot_dp workgroup
constexpr int SMOOTH_DP_GROUPS = 4;              // ... workgroups per pair

struct SmoothSegment {  // = ffs_smooth_segment
    double fit_total, line_score, bend_total;
    int32_t n_knots, reserved;
};
static_assert(sizeof(SmoothSegment) == 32, "SmoothSegment must match ffs_smooth_segment");

struct SmoothSeg {  // workspace: one per segment
    int32_t first, end;      // blocks [first, end)
    int32_t n_int, int_base; // intervals (0 for a one-block segment), index of the first in the pair's interval table
};
struct SmoothInt {  // workspace: one per interval
    int32_t k, n;            // first knot block, blocks to the next knot
    int32_t seg, last;       // segment, 1 when it is the segment's last interval (it holds block k + n too)
};

struct SmoothWs {
    SmoothSeg* seg;          // [slot][max_blocks]
    SmoothInt* iv;           // [slot][max_blocks]
    int32_t* seg_of;         // [slot][max_blocks]: segment of every block
    int32_t* n_int;          // [slot]
    double* T;               // [slot][max_blocks][states] line scores
    uint8_t* back;           // [slot][max_blocks][states] predecessor candidate index of every state
    int64_t stride;          // max_blocks
};

// the u of rank r in the order candidates are tried: 0, +1, -1, +2, -2, ...
FFS_DEV int smooth_tie_u(int r) { return (r & 1) ? (r + 1) >> 1 : -(r >> 1); }

// floor(num / den), den > 0
FFS_DEV int32_t smooth_floor_div(int32_t num, int32_t den) {
    int32_t q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}

// ((lambda * g) * M) / (n_a n_b), g = |D2 n_a - D1 n_b|
FFS_DEV double smooth_bend(double lambda, int M, int64_t d1, int64_t d2, int64_t na, int64_t nb) {
#pragma clang fp contract(off)
    int64_t g = d2 * na - d1 * nb;
    g = g < 0 ? -g : g;
    return ((lambda * (double)g) * (double)M) / (double)(na * nb);
}

// segment and interval tables of one pair per workgroup; knot flags and the path as the initial smooth offsets
__global__ void __launch_bounds__(SMOOTH_INT_THREADS) k_smooth_intervals(const SplitDesc* __restrict__ desc, SmoothWs sw,
                                                                        int K, int M, int64_t out_stride,
                                                                        const int32_t* __restrict__ block_offset,
                                                                        const uint8_t* __restrict__ block_jump,
                                                                        int32_t* __restrict__ smooth_offset,
                                                                        uint8_t* __restrict__ knot,
                                                                        SmoothSegment* __restrict__ records,
                                                                        int32_t* __restrict__ n_segments_out) {
    constexpr int NW = SMOOTH_INT_THREADS / 64;
    __shared__ int s_cnt[NW];
    __shared__ int s_scan[SMOOTH_INT_THREADS];
    const int slot = blockIdx.x;
    const SplitDesc d = desc[slot];
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint8_t* jump = block_jump + d.out_row * out_stride;
    SmoothSeg* seg = sw.seg + slot * sw.stride;
    SmoothInt* iv = sw.iv + slot * sw.stride;
    int32_t* seg_of = sw.seg_of + slot * sw.stride;
    SmoothSegment* rec = records + d.out_row * out_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int n_seg = 0;  // segments that start before this chunk of blocks
    for (int64_t b0 = 0; b0 < B; b0 += SMOOTH_INT_THREADS) {
        const int64_t b = b0 + t;
        const bool in = b < B;
        const bool start = in && (b == 0 || jump[b] != 0);
        const bool last = in && (b == B - 1 || jump[b + 1] != 0);
        const unsigned long long m = __ballot(start);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = n_seg, chunk = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            chunk += s_cnt[w];
        }
        const int idx = before + __popcll(m & ((2ull << lane) - 1ull)) - 1;  // the starts at or before b, minus one
        if (start) seg[idx].first = (int32_t)b;
        if (last) seg[idx].end = (int32_t)(b + 1);
        if (in) seg_of[b] = idx;
        n_seg += chunk;
        __syncthreads();  // before the next chunk rewrites s_cnt
    }
    __threadfence_block();  // the block ranges written above are read by other threads below
    __syncthreads();
    int n_int = 0;  // intervals of the segments before this chunk of segments
    for (int s0 = 0; s0 < n_seg; s0 += SMOOTH_INT_THREADS) {
        const int s = s0 + t;
        int cnt = 0;
        if (s < n_seg) {
            const int n = seg[s].end - 1 - seg[s].first;
            const int by_m = (n + M / 2) / M;
            cnt = n < 1 ? 0 : (by_m > 1 ? by_m : 1);
        }
        s_scan[t] = cnt;
        __syncthreads();
        for (int off = 1; off < SMOOTH_INT_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan
            const int add = t >= off ? s_scan[t - off] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        if (s < n_seg) {
            seg[s].n_int = cnt;
            seg[s].int_base = n_int + s_scan[t] - cnt;
            rec[s].fit_total = 0.0;
            rec[s].line_score = 0.0;
            rec[s].bend_total = 0.0;
            rec[s].n_knots = cnt + 1;
            rec[s].reserved = 0;
        }
        n_int += s_scan[SMOOTH_INT_THREADS - 1];
        __syncthreads();  // before the next chunk rewrites s_scan
    }
    unsigned long long* words = (unsigned long long*)rec;
    constexpr int RW = (int)(sizeof(SmoothSegment) / 8);
    for (int64_t q = (int64_t)n_seg * RW + t; q < out_stride * RW; q += SMOOTH_INT_THREADS) words[q] = 0ull;
    if (t == 0) {
        n_segments_out[d.out_row] = n_seg;
        sw.n_int[slot] = n_int;
    }
    __threadfence_block();
    __syncthreads();
    int32_t* sm = smooth_offset + d.out_row * out_stride;
    uint8_t* kn = knot + d.out_row * out_stride;
    for (int64_t b = t; b < out_stride; b += SMOOTH_INT_THREADS) {
        if (b >= B) {
            sm[b] = 0;
            kn[b] = 0;
            continue;
        }
        const int s = seg_of[b];
        const SmoothSeg g = seg[s];
        const int j = (int)b - g.first, i = j / M;
        const bool is_start = g.n_int > 0 && j % M == 0 && i < g.n_int;
        if (is_start) {
            SmoothInt v;
            v.k = (int32_t)b;
            v.last = i == g.n_int - 1;
            v.n = v.last ? g.end - 1 - (int32_t)b : M;
            v.seg = s;
            iv[g.int_base + i] = v;
        }
        sm[b] = o[b];
        kn[b] = (g.n_int == 0 || is_start || b == g.end - 1) ? 1 : 0;
    }
}

// T of every line of the intervals blockIdx.x % SMOOTH_LINE_GROUPS, + SMOOTH_LINE_GROUPS, ... of one pair;
// grid.x = pairs * SMOOTH_LINE_GROUPS
__global__ void __launch_bounds__(SMOOTH_LINE_THREADS) k_drift_line_sums(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                                        SmoothWs sw, int K, int64_t W, int R,
                                                                        int64_t out_stride,
                                                                        const int32_t* __restrict__ block_offset) {
    const int slot = blockIdx.x / SMOOTH_LINE_GROUPS;
    const SplitDesc d = desc[slot];
    const int n_int = sw.n_int[slot];
    const int S1 = 2 * R + 1, S2 = S1 * S1;
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint16_t* counts = ws.counts + slot * ws.counts_slot;
    const SmoothInt* ivs = sw.iv + slot * sw.stride;
    for (int q = blockIdx.x % SMOOTH_LINE_GROUPS; q < n_int; q += SMOOTH_LINE_GROUPS) {  // (uniform)
        const SmoothInt v = ivs[q];
        const int nb = v.n + v.last;  // blocks of the interval
        const int32_t o0 = o[v.k], o1 = o[v.k + v.n];
        double* out = sw.T + ((int64_t)slot * sw.stride + q) * S2;
        for (int line = threadIdx.x; line < S2; line += SMOOTH_LINE_THREADS) {
            const int32_t c0 = o0 + line / S1 - R, c1 = o1 + line % S1 - R;
            if (c0 < -W + 1 || c0 > W || c1 < -W + 1 || c1 > W) {
                out[line] = -INFINITY;
                continue;
            }
            const int32_t two_d = 2 * (c1 - c0), two_n = 2 * v.n;
            uint32_t ov = 0u, n11 = 0u, n1x = 0u, nx1 = 0u;
            for (int j = 0; j < nb; ++j) {
                const int64_t b = v.k + j;
                const int64_t lag = c0 + smooth_floor_div(two_d * j + v.n, two_n);  // inside the window: between c0 and c1
                const int64_t blo = b * K, bhi = (blo + K < d.S) ? blo + K : d.S;
                const int64_t a = blo > -lag ? blo : -lag;
                const int64_t e = bhi < d.R - lag ? bhi : d.R - lag;
                if (e <= a) continue;
                ov += (uint32_t)(e - a);
                n11 += counts[b * ws.counts_row + (lag + W - 1)];
                n1x += (uint32_t)(split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a));
                nx1 += (uint32_t)(split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag));
            }
            out[line] = ov ? split_mix(d, ov, n11, n1x, nx1) : 0.0;
        }
    }
}

// the Viterbi pass, backtrack and smooth offsets of the segments blockIdx.x % SMOOTH_DP_GROUPS, + SMOOTH_DP_GROUPS, ...
// of one pair; grid.x = pairs * SMOOTH_DP_GROUPS
__global__ void __launch_bounds__(SMOOTH_DP_THREADS) k_drift_knot_dp(const SplitDesc* __restrict__ desc, SmoothWs sw, int M,
                                                                    int R, double lambda, int64_t out_stride,
                                                                    const int32_t* __restrict__ block_offset,
                                                                    const int32_t* __restrict__ n_segments,
                                                                    int32_t* __restrict__ smooth_offset,
                                                                    SmoothSegment* __restrict__ records) {
#pragma clang fp contract(off)
    __shared__ double s_v[2][SMOOTH_MAX_STATES];
    const int slot = blockIdx.x / SMOOTH_DP_GROUPS;
    const SplitDesc d = desc[slot];
    const int n_seg = n_segments[d.out_row];
    const int S1 = 2 * R + 1, S2 = S1 * S1;
    const int32_t* o = block_offset + d.out_row * out_stride;
    int32_t* sm = smooth_offset + d.out_row * out_stride;
    const SmoothSeg* segs = sw.seg + slot * sw.stride;
    const SmoothInt* ivs = sw.iv + slot * sw.stride;
    const int t = threadIdx.x;
    for (int s = blockIdx.x % SMOOTH_DP_GROUPS; s < n_seg; s += SMOOTH_DP_GROUPS) {  // (uniform)
        const SmoothSeg g = segs[s];
        if (g.n_int == 0) continue;  // (uniform) a one-block segment stays as it is
        const double* T = sw.T + ((int64_t)slot * sw.stride + g.int_base) * S2;
        uint8_t* back = sw.back + ((int64_t)slot * sw.stride + g.int_base) * S2;
        int cur = 0;
        for (int q = t; q < S2; q += SMOOTH_DP_THREADS) s_v[0][q] = T[q];
        __syncthreads();
        for (int i = 1; i < g.n_int; ++i) {
            const SmoothInt va = ivs[g.int_base + i - 1], vb = ivs[g.int_base + i];
            const int64_t oa = o[va.k], ob = o[vb.k], oc = o[vb.k + vb.n];
            const double* vp = s_v[cur];
            double* vn = s_v[cur ^ 1];
            const double* Ti = T + (int64_t)i * S2;
            for (int q = t; q < S2; q += SMOOTH_DP_THREADS) {
                const int bi = q / S1, ci = q % S1;
                const int64_t d2 = (oc + ci) - (ob + bi);  // the two - R cancel
                double best = 0.0;
                int arg = 0;
                for (int r = 0; r < S1; ++r) {
                    const int ai = smooth_tie_u(r) + R;
                    const double cand = vp[ai * S1 + bi] - smooth_bend(lambda, M, (ob + bi) - (oa + ai), d2, va.n, vb.n);
                    if (r == 0 || cand > best) {  // strict: ties keep the earlier candidate
                        best = cand;
                        arg = ai;
                    }
                }
                vn[q] = best + Ti[q];
                back[(int64_t)i * S2 + q] = (uint8_t)arg;
            }
            cur ^= 1;
            __syncthreads();
        }
        if (t == 0) {
            const double* v = s_v[cur];
            double best = 0.0;
            int ai = 0, bi = 0;
            for (int rb = 0; rb < S1; ++rb)
                for (int ra = 0; ra < S1; ++ra) {
                    const int b = smooth_tie_u(rb) + R, a = smooth_tie_u(ra) + R;
                    const double cand = v[a * S1 + b];
                    if ((rb == 0 && ra == 0) || cand > best) {
                        best = cand;
                        ai = a;
                        bi = b;
                    }
                }
            // backtrack: knot i sits at o_{k_i} + (index - R); the knots' own smooth offsets are written here
            const SmoothInt vl = ivs[g.int_base + g.n_int - 1];
            sm[vl.k + vl.n] = o[vl.k + vl.n] + bi - R;
            sm[vl.k] = o[vl.k] + ai - R;
            for (int i = g.n_int - 1; i >= 1; --i) {
                const int pa = back[(int64_t)i * S2 + ai * S1 + bi];
                bi = ai;
                ai = pa;
                const int32_t k = ivs[g.int_base + i - 1].k;
                sm[k] = o[k] + ai - R;
            }
            double line = 0.0, bend = 0.0;
            for (int i = 0; i < g.n_int; ++i) {
                const SmoothInt vi = ivs[g.int_base + i];
                const int a = sm[vi.k] - o[vi.k] + R, b = sm[vi.k + vi.n] - o[vi.k + vi.n] + R;
                line = line + T[(int64_t)i * S2 + a * S1 + b];
                if (i >= 1) {
                    const SmoothInt vh = ivs[g.int_base + i - 1];
                    bend = bend + smooth_bend(lambda, M, (int64_t)sm[vi.k] - sm[vh.k], (int64_t)sm[vi.k + vi.n] - sm[vi.k], vh.n,
                                              vi.n);
                }
            }
            SmoothSegment* rec = records + d.out_row * out_stride + s;
            rec->fit_total = best;
            rec->line_score = line;
            rec->bend_total = bend;
        }
        __threadfence_block();  // the knots' lags written by thread 0 are read by every thread below
        __syncthreads();
        for (int b = g.first + t; b < g.end - 1; b += SMOOTH_DP_THREADS) {
            const int j = b - g.first;
            if (j % M == 0 && j / M < g.n_int) continue;  // a knot: written above
            const int i = j / M < g.n_int ? j / M : g.n_int - 1;
            const SmoothInt vi = ivs[g.int_base + i];
            const int32_t c0 = sm[vi.k], c1 = sm[vi.k + vi.n];
            sm[b] = c0 + smooth_floor_div(2 * (c1 - c0) * (b - vi.k) + vi.n, 2 * vi.n);
        }
        __syncthreads();  // before the next segment rewrites s_v
    }
}

}  // namespace ffsa
