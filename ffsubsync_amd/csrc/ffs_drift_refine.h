// ffs_drift_refine.h -- sample-exact jumps of a drift solve (gfx950).  ffs_split_refine.h refines the breaks of a
// piecewise-CONSTANT path; a drift path changes offset at almost every block, so here the refined positions are the
// path's JUMPS and each side of a jump is scored along its own segment's per-block lags.  The contract is this
// library's own, pinned against the numpy model tests/drift_refine_model.py, bit for bit.
//
// Per pair: ffs_split_refine.h's inputs plus the jump flags j_b (uint8, b < B).  Jumps are the blocks f_j >= 1 with
// j_{f_j} != 0 (j_0 is ignored), whether or not the offset changes there; cut c_j = f_j K, the window [L_j, U_j] as in
// ffs_split_refine.h (clipped at the midpoints to the neighbouring jumps, so only the two segments around the jump are
// read).  For a subtitle sample x with b(x) = floor(x / K):
//     lag_a(x) = o[min(b(x), f_j - 1)],  lag_b(x) = o[max(b(x), f_j)]
// -- each segment's own lag where the segment exists, held at its last (first) block's value past the coarse cut.
// A(t): split_mix of the counts of [L, t) at lag_a(x); B(t): of [t, U) at lag_b(x); a sample whose partner x + lag(x)
// lies outside [0, R) is absent.  N, F, G, t1, t2, beta = NaN, the tie rules, the flags and the record are
// ffs_split_refine.h's; offset_prev = o[f_j - 1], offset_next = o[f_j].  On offsets constant inside every segment with
// j_b set exactly where the offset changes, every byte equals ffs_split_refine_batch's.
//
// Two kernels per sub-batch of pairs, as ffs_split_refine.h:
//   k_drift_refine_jumps  k_refine_breaks with the predicate j_b != 0.
//   k_drift_refine_cut    k_refine_cut's three passes with the two lags of a word looked up per block (K is a multiple
//                         of 32, so a word lies in one block; its presence mask uses its own lag).  The window's block
//                         offsets are staged in LDS once per workgroup: a window of <= 2 * 131072 samples at K >= 256
//                         touches <= 1026 blocks, 4.1 KB of int32.
#pragma once
#include "ffs_split_refine.h"

namespace ffsa {

constexpr int DRIFT_REFINE_MAX_BLOCKS = (int)(2 * REFINE_MAX_RADIUS / 256) + 2;  // blocks of the widest window at K = 256

// one workgroup per pair: jump table, windows, zeroed tail, jump count, null-score constants.
// KEEP IN STEP with k_refine_breaks (ffs_split_refine.h): the same code but for the predicate `jf[b] != 0`; a fix to the
// numbering, the windows or the popcount there belongs here too (the byte identity on flat paths is tested on the device).
__global__ void __launch_bounds__(REFINE_TABLE_THREADS) k_drift_refine_jumps(const RefineDesc* __restrict__ desc, int K,
                                                                             int64_t out_stride, int64_t radius,
                                                                             double beta,
                                                                             const int32_t* __restrict__ block_offset,
                                                                             const uint8_t* __restrict__ block_jump,
                                                                             BreakRefine* __restrict__ out,
                                                                             int32_t* __restrict__ n_jumps_out) {
#pragma clang fp contract(off)
    constexpr int NW = REFINE_TABLE_THREADS / 64;
    __shared__ int s_cnt[NW];
    __shared__ unsigned long long s_pop[NW];
    const RefineDesc d = desc[blockIdx.x];
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint8_t* jf = block_jump + d.out_row * out_stride;
    BreakRefine* rec = out + d.out_row * out_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;  // jumps before this chunk of blocks
    for (int64_t b0 = 0; b0 < B; b0 += REFINE_TABLE_THREADS) {
        const int64_t b = b0 + t;
        const bool brk = b >= 1 && b < B && jf[b] != 0;
        const unsigned long long m = __ballot(brk);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = carry, chunk = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            chunk += s_cnt[w];
        }
        if (brk) {
            const int idx = before + __popcll(m & ((1ull << lane) - 1ull));
            rec[idx].block = b;
            rec[idx].cut = b * K;
            rec[idx].offset_prev = o[b - 1];
            rec[idx].offset_next = o[b];
        }
        carry += chunk;
        __syncthreads();  // before the next chunk rewrites s_cnt
    }
    __threadfence_block();
    __syncthreads();  // the cuts of every jump are written
    const int n = carry;
    for (int j = t; j < n; j += REFINE_TABLE_THREADS) {
        const int64_t c = rec[j].cut;
        int32_t flags = 0;
        int64_t lo = c - radius, hi = c + radius;
        if (j == 0) {
            lo = lo > 0 ? lo : 0;
        } else {
            const int64_t mid = (rec[j - 1].cut + c) / 2;  // non-negative: floor
            if (mid > lo) {
                lo = mid;
                flags |= REFINE_CLIPPED;
            }
        }
        if (j + 1 == n) {
            hi = hi < d.S ? hi : d.S;
        } else {
            const int64_t mid = (c + rec[j + 1].cut) / 2;
            if (mid < hi) {
                hi = mid;
                flags |= REFINE_CLIPPED;
            }
        }
        rec[j].lo = lo;
        rec[j].hi = hi;
        rec[j].t1 = rec[j].t2 = 0;
        rec[j].coarse_score = rec[j].refined_score = 0.0;
        rec[j].flags = flags;
        rec[j].reserved = 0;
    }
    unsigned long long* words = (unsigned long long*)rec;
    constexpr int RW = (int)(sizeof(BreakRefine) / 8);
    for (int64_t q = (int64_t)n * RW + t; q < out_stride * RW; q += REFINE_TABLE_THREADS) words[q] = 0ull;
    // popcount of the whole reference
    unsigned long long pop = 0;
    const int64_t nw = (d.R + 31) >> 5;
    for (int64_t g = t; g < nw; g += REFINE_TABLE_THREADS) pop += __popc(split_word(d.r, d.R, g));
    for (int s = 32; s >= 1; s >>= 1) pop += __shfl_xor(pop, s, 64);
    if (lane == 0) s_pop[wave] = pop;
    __syncthreads();
    if (t == 0) {
        unsigned long long p1 = 0;
        for (int w = 0; w < NW; ++w) p1 += s_pop[w];
        const double rbar = ((double)(d.R - (int64_t)p1) * d.r0 + (double)(int64_t)p1 * d.r1) / (double)d.R;
        const double bz = beta == beta ? beta : 0.0;  // NaN (single cut): the null score is never read
        d.pair_ws[0] = d.s0 * rbar + bz * fabs(d.s0);
        d.pair_ws[1] = d.s1 * rbar + bz * fabs(d.s1);
        d.pair_ws[2] = rbar;
        n_jumps_out[d.out_row] = n;
    }
}

// one workgroup per (pair, jump slot): t1, t2, the coarse and refined scores, the edge / unmatched flags.
// KEEP IN STEP with k_refine_cut (ffs_split_refine.h): the same three passes, scans and argmax; what differs is the LDS
// staging of the block offsets and `lags()`, which replace the two constant lags.  A fix to either kernel's scan, walk or
// tie handling belongs in both.
__global__ void __launch_bounds__(REFINE_THREADS) k_drift_refine_cut(const RefineDesc* __restrict__ desc, int n_slots,
                                                                     int K, int64_t out_stride, bool single,
                                                                     const int32_t* __restrict__ block_offset,
                                                                     const int32_t* __restrict__ n_jumps,
                                                                     BreakRefine* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int NW = REFINE_THREADS / 64;
    __shared__ int32_t s_off[DRIFT_REFINE_MAX_BLOCKS];
    __shared__ int32_t s_wsum[NW][REFINE_NC];
    __shared__ double s_wv[NW];
    __shared__ int s_wi[NW], s_wj[NW];
    __shared__ double s_coarse;
    const int jb = blockIdx.x % n_slots;
    const int slot = blockIdx.x / n_slots;
    const RefineDesc d = desc[slot];
    if (jb >= n_jumps[d.out_row]) return;  // (uniform)
    BreakRefine* rec = out + d.out_row * out_stride + jb;
    const int64_t L = rec->lo, U = rec->hi, c = rec->cut;
    const double z0 = d.pair_ws[0], z1 = d.pair_ws[1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // the window's blocks [bL, bU] (U = S on a block boundary belongs to no block: held at the last), their offsets in LDS
    const int wpb = K >> 5;  // words per block
    const int f = (int)rec->block;
    const int bL = (int)(L / K);
    const int b_last = (int)((d.S + K - 1) / K) - 1;
    int bU = (int)(U / K);
    bU = bU < b_last ? bU : b_last;
    bU = bU < bL + DRIFT_REFINE_MAX_BLOCKS - 1 ? bU : bL + DRIFT_REFINE_MAX_BLOCKS - 1;  // (never binds: the radius limit)
    {
        const int32_t* o = block_offset + d.out_row * out_stride;
        for (int i = t; i <= bU - bL; i += REFINE_THREADS) s_off[i] = o[bL + i];
    }
    __syncthreads();
    // the two lags of word g: its block's offset on the segment's own side, the nearest block's past the coarse cut
    auto lags = [&](int64_t g, int64_t& la, int64_t& lb) {
        int b = (int)((uint32_t)g / (uint32_t)wpb);
        b = b < bL ? bL : (b > bU ? bU : b);
        const int ba = b < f - 1 ? b : f - 1, bb = b > f ? b : f;
        la = s_off[ba - bL];
        lb = s_off[bb - bL];
    };
    // words [gL, gU] hold the samples t in [L, U]; thread t owns [w0, w1)
    const int64_t gL = L >> 5, gU = U >> 5;
    const int64_t per = (gU - gL + 1 + REFINE_THREADS - 1) / REFINE_THREADS;
    const int64_t w0 = gL + t * per, w1 = (w0 + per < gU + 1) ? w0 + per : gU + 1;
    uint32_t m[REFINE_NC];
    // pass 1: the thread's sums, exclusive workgroup scan
    int32_t run[REFINE_NC], tot[REFINE_NC];
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) run[x] = 0;
    for (int64_t g = w0; g < w1; ++g) {
        int64_t la, lb;
        lags(g, la, lb);
        refine_masks(d, g, L, U, la, lb, m);
#pragma unroll
        for (int x = 0; x < REFINE_NC; ++x) run[x] += __popc(m[x]);
    }
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) {
        const int32_t own = run[x];
        int32_t inc = own;
        for (int s = 1; s < 64; s <<= 1) {
            const int32_t up = __shfl_up(inc, s, 64);
            if (lane >= s) inc += up;
        }
        if (lane == 63) s_wsum[wave][x] = inc;
        run[x] = inc - own;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) {
        int32_t before = 0, all = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_wsum[w][x] : 0;
            all += s_wsum[w][x];
        }
        run[x] += before;
        tot[x] = all;
    }
    // every sample t in [L, U] of the thread's words, in order, with its counts over [L, t)
    auto walk = [&](auto&& visit) {
        int32_t cur[REFINE_NC];
#pragma unroll
        for (int x = 0; x < REFINE_NC; ++x) cur[x] = run[x];
        for (int64_t g = w0; g < w1; ++g) {
            int64_t la, lb;
            lags(g, la, lb);
            refine_masks(d, g, L, U, la, lb, m);
            for (int k = 0; k < 32; ++k) {
                const int64_t ts = g * 32 + k;
                if (ts < L || ts > U) continue;
                const uint32_t low = (1u << k) - 1u;
                int32_t p[REFINE_NC];
#pragma unroll
                for (int x = 0; x < REFINE_NC; ++x) p[x] = cur[x] + __popc(m[x] & low);
                const double A = refine_mix(d, p[0], p[1], p[2], p[3]);
                const double Bv = refine_mix(d, tot[4] - p[4], tot[5] - p[5], tot[6] - p[6], tot[7] - p[7]);
                const int32_t n1 = p[8], n0 = (int32_t)(ts - L) - n1;
                const double N = (double)n0 * z0 + (double)n1 * z1;
                visit((int)ts, A, Bv, N);
            }
#pragma unroll
            for (int x = 0; x < REFINE_NC; ++x) cur[x] += __popc(m[x]);
        }
    };
    // pass 2 (two cuts): the prefix maximum of F entering the thread's samples
    double mv = -INFINITY;
    int mi = INT_MAX;
    if (!single) {
        walk([&](int ts, double A, double Bv, double N) { refine_pmax(mv, mi, A - N, ts); });
        for (int s = 1; s < 64; s <<= 1) {  // inclusive scan, earlier lanes on the left
            const double uv = __shfl_up(mv, s, 64);
            const int ui = __shfl_up(mi, s, 64);
            if (lane >= s) {
                double lv = uv;
                int li = ui;
                refine_pmax(lv, li, mv, mi);
                mv = lv;
                mi = li;
            }
        }
        if (lane == 63) {
            s_wv[wave] = mv;
            s_wi[wave] = mi;
        }
        double ev = __shfl_up(mv, 1, 64);  // exclusive within the wave
        int ei = __shfl_up(mi, 1, 64);
        if (lane == 0) {
            ev = -INFINITY;
            ei = INT_MAX;
        }
        __syncthreads();
        double pv = -INFINITY;
        int pi = INT_MAX;
        for (int w = 0; w < wave; ++w) refine_pmax(pv, pi, s_wv[w], s_wi[w]);
        refine_pmax(pv, pi, ev, ei);
        mv = pv;
        mi = pi;
        __syncthreads();  // s_wv / s_wi are reused below
    }
    // pass 3: the objective at every t, the thread's first maximiser
    double hv = -INFINITY;
    int h2 = INT_MAX, h1 = INT_MAX;
    walk([&](int ts, double A, double Bv, double N) {
        double h;
        int i1;
        if (single) {
            h = A + Bv;
            i1 = ts;
        } else {
            refine_pmax(mv, mi, A - N, ts);
            h = (N + Bv) + mv;
            i1 = mi;
        }
        if (h > hv) {
            hv = h;
            h2 = ts;
            h1 = i1;
        }
        if (ts == c) s_coarse = A + Bv;
    });
    // workgroup argmax, smallest t2 on ties
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(hv, s, 64);
        const int o2 = __shfl_xor(h2, s, 64), o1 = __shfl_xor(h1, s, 64);
        if (ov > hv || (ov == hv && o2 < h2)) {
            hv = ov;
            h2 = o2;
            h1 = o1;
        }
    }
    if (lane == 0) {
        s_wv[wave] = hv;
        s_wi[wave] = h2;
        s_wj[wave] = h1;
    }
    __syncthreads();
    if (t == 0) {
        double v = s_wv[0];
        int i2 = s_wi[0], i1 = s_wj[0];
        for (int w = 1; w < NW; ++w) {
            if (s_wv[w] > v || (s_wv[w] == v && s_wi[w] < i2)) {
                v = s_wv[w];
                i2 = s_wi[w];
                i1 = s_wj[w];
            }
        }
        int32_t flags = rec->flags;
        if ((i1 == L && L > 0) || (i2 == U && U < d.S)) flags |= REFINE_AT_EDGE;
        if (i1 < i2) flags |= REFINE_UNMATCHED;
        rec->t1 = i1;
        rec->t2 = i2;
        rec->coarse_score = s_coarse;
        rec->refined_score = v;
        rec->flags = flags;
    }
}

}  // namespace ffsa
