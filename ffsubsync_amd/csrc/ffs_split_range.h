// ffs_split_range.h -- split-aware alignment over any contiguous lag range [lag_lo, lag_hi], up to the full overlap
// range (gfx950).  The contract is ffs_split.h's with the lag set d = lag_lo + j, j in [0, L), L = lag_hi - lag_lo + 1
// (lags without overlap score 0); at [-W+1, W] the records are bit-identical to k_split_dp's.  Pinned against the numpy
// model tests/cut_model.py.
//
// k_split_dp runs one workgroup per pair and stores every (block, lag) count: at the full range of a 2 h pair (1.44 M
// lags, 704 blocks) that is 2 GB of counts and one CU walking 1e9 cells.  Here one pair's lag row is spread over many
// workgroups instead, one plain launch per block step covering every pair in flight (no co-residency, nothing to wait
// on inside a kernel: the stream orders the steps):
//   k_split_prefix    (ffs_split.h) word prefix popcounts of s and of all of r.
//   k_range_step      block b, one RANGE_TILE-lag tile per workgroup: the tile's n11 from LDS-staged words (the
//                     k_split_counts funnel-shift scheme, counts never stored), the score, the V update in place (each
//                     lag belongs to one thread), one stay-bit ballot per 64 lags, and the tile's (max, largest argmax)
//                     partial.  T_{b-1} = J_{b-1} - P comes from the previous step's partials, which every workgroup of
//                     the pair reduces itself (the order-free max with the largest-lag tie rule: deterministic); the
//                     partials are double-buffered by the parity of b.
//   k_range_backtrack one workgroup per pair: the last step's partials give the total and the end lag; thread 0 walks
//                     the stay bits back.
//   k_range_scores    one wave per block: n11 at the chosen lag, the block score, the lag into the int32 output.
#pragma once
#include "ffs_split.h"

namespace ffsa {

constexpr int RANGE_THREADS = 256;
constexpr int RANGE_LPT = 8;                             // lags per thread in k_range_step
constexpr int RANGE_TILE = RANGE_THREADS * RANGE_LPT;    // 2048 lags per workgroup (64 words of reference bits)
constexpr int RANGE_SCORE_THREADS = 256;                 // k_range_scores: one wave per block

struct RangeLag {
    int64_t lag_lo;  // lag of lag index 0
    int64_t L;       // lags in the range (>= 1)
};

struct RangeWs {
    unsigned long long* stay;  // [slot][max_blocks][stay_row]
    double* V;                 // [slot][v_slot]
    double* pv;                // [slot][2][part_row]: per-tile row maxima, double-buffered by step parity
    int32_t* pj;               // [slot][2][part_row]: their lag indices
    int32_t* arg;              // [slot][max_blocks]: lag index of the row maximum after block b
    int64_t stay_row, stay_slot, v_slot, part_row, arg_slot;
};

// the pair's row maximum of step `b` (largest lag index on ties) from its n_tiles partials; every thread gets it
FFS_DEV void range_reduce(const RangeWs& ws, int slot, int64_t b, int64_t n_tiles, double* s_v, int* s_j, double& best,
                          int& bestj) {
    constexpr int NW = RANGE_THREADS / 64;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t base = ((int64_t)slot * 2 + (b & 1)) * ws.part_row;
    best = -INFINITY;
    bestj = -1;
    for (int64_t i = t; i < n_tiles; i += RANGE_THREADS) split_max_pair(best, bestj, ws.pv[base + i], ws.pj[base + i]);
    for (int s = 32; s >= 1; s >>= 1) split_max_pair(best, bestj, __shfl_xor(best, s, 64), __shfl_xor(bestj, s, 64));
    if (lane == 0) {
        s_v[wave] = best;
        s_j[wave] = bestj;
    }
    __syncthreads();
    best = s_v[0];
    bestj = s_j[0];
    for (int w = 1; w < NW; ++w) split_max_pair(best, bestj, s_v[w], s_j[w]);
    __syncthreads();  // s_v / s_j are reused by the caller
}

// m_b(lag) from n11 and the prefix popcounts: split_score's expression with the lag given directly
FFS_DEV double range_score(const SplitDesc& d, int64_t b, int64_t lag, int64_t n11, int K) {
    const int64_t blo = b * K, bhi = (blo + K < d.S) ? blo + K : d.S;
    const int64_t a = blo > -lag ? blo : -lag;
    const int64_t e = bhi < d.R - lag ? bhi : d.R - lag;
    int64_t ov = 0, c11 = 0, n1x = 0, nx1 = 0;
    if (e > a) {
        ov = e - a;
        c11 = n11;
        n1x = split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a);
        nx1 = split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag);
    }
    return split_mix(d, ov, c11, n1x, nx1);
}

// one DP step (block b) of every pair in flight; grid = (max tiles, pairs)
__global__ void __launch_bounds__(RANGE_THREADS) k_range_step(const SplitDesc* __restrict__ desc,
                                                             const RangeLag* __restrict__ lags, RangeWs ws, int K,
                                                             int64_t b, double P) {
#pragma clang fp contract(off)
    constexpr int NW = RANGE_THREADS / 64;
    __shared__ uint32_t s_sub[SPLIT_MAX_K / 32];
    __shared__ uint32_t s_ref[SPLIT_MAX_K / 32 + RANGE_TILE / 32 + 1];
    __shared__ double s_v[NW];
    __shared__ int s_j[NW];
    const int slot = blockIdx.y;
    const int64_t tile = blockIdx.x;
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int64_t B = (d.S + K - 1) / K;
    const int64_t n_tiles = (lg.L + RANGE_TILE - 1) / RANGE_TILE;
    if (b >= B || tile >= n_tiles) return;  // (uniform)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double T = 0.0;
    if (b > 0) {
        double J;
        int aj;
        range_reduce(ws, slot, b - 1, n_tiles, s_v, s_j, J, aj);
        T = J - P;
        if (tile == 0 && t == 0) ws.arg[(int64_t)slot * ws.arg_slot + b - 1] = aj;
    }
    const int kw = K >> 5;
    const int n_ref_words = kw + RANGE_TILE / 32 + 1;
    const int64_t j_tile = tile * RANGE_TILE;
    const int64_t base = b * K + lg.lag_lo + j_tile;  // reference sample met by the block's first sample at the tile's first lag
    const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
    const int bsh = (int)(base - gbase * 32);
    for (int q = t; q < n_ref_words; q += RANGE_THREADS) {
        const uint32_t lo = split_word(d.r, d.R, gbase + q), hi = split_word(d.r, d.R, gbase + q + 1);
        s_ref[q] = __builtin_amdgcn_alignbit(hi, lo, bsh);
    }
    for (int q = t; q < kw; q += RANGE_THREADS) s_sub[q] = split_word(d.s, d.S, b * kw + q);
    __syncthreads();
    // lag offset t + 256k inside the tile: reference word q0 + 8k + w of the staged window, shifted by sh
    const int q0 = t >> 5, sh = t & 31;
    uint32_t lo[RANGE_LPT], acc[RANGE_LPT];
#pragma unroll
    for (int k = 0; k < RANGE_LPT; ++k) {
        lo[k] = s_ref[q0 + 8 * k];
        acc[k] = 0;
    }
    for (int w = 0; w < kw; ++w) {
        const uint32_t sw = s_sub[w];  // (one address per wave: broadcast)
#pragma unroll
        for (int k = 0; k < RANGE_LPT; ++k) {
            const uint32_t hi = s_ref[q0 + 8 * k + w + 1];
            acc[k] += __popc(__builtin_amdgcn_alignbit(hi, lo[k], sh) & sw);
            lo[k] = hi;
        }
    }
    double* V = ws.V + (int64_t)slot * ws.v_slot;
    unsigned long long* stay = ws.stay + (int64_t)slot * ws.stay_slot + b * ws.stay_row;
    double best = -INFINITY;
    int bestj = -1;
#pragma unroll
    for (int k = 0; k < RANGE_LPT; ++k) {
        const int64_t j0 = j_tile + RANGE_THREADS * k + 64 * wave;  // the wave's first lag index: a multiple of 64
        const int64_t j = j0 + lane;
        bool st = false;
        if (j < lg.L) {
            const double m = range_score(d, b, lg.lag_lo + j, acc[k], K);
            double v;
            if (b == 0) {
                v = m;
            } else {
                const double vp = V[j];
                st = vp >= T;  // ties stay
                v = (st ? vp : T) + m;
            }
            V[j] = v;
            split_max_pair(best, bestj, v, (int)j);
        }
        const unsigned long long bits = __ballot(st);
        if (b > 0 && lane == 0 && j0 < lg.L) stay[j0 >> 6] = bits;
    }
    for (int s = 32; s >= 1; s >>= 1) split_max_pair(best, bestj, __shfl_xor(best, s, 64), __shfl_xor(bestj, s, 64));
    if (lane == 0) {
        s_v[wave] = best;
        s_j[wave] = bestj;
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < NW; ++w) split_max_pair(best, bestj, s_v[w], s_j[w]);  // thread 0's own is s_v[0]
        const int64_t o = ((int64_t)slot * 2 + (b & 1)) * ws.part_row + tile;
        ws.pv[o] = best;
        ws.pj[o] = bestj;
    }
}

// one workgroup per pair: total, end lag and the backtrack (lag indices into the offset output for now)
__global__ void __launch_bounds__(RANGE_THREADS) k_range_backtrack(const SplitDesc* __restrict__ desc,
                                                                  const RangeLag* __restrict__ lags, RangeWs ws, int K,
                                                                  int64_t out_stride, int32_t* __restrict__ block_offset_out,
                                                                  double* __restrict__ total_out) {
    constexpr int NW = RANGE_THREADS / 64;
    __shared__ double s_v[NW];
    __shared__ int s_j[NW];
    const int slot = blockIdx.x;
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int64_t B = (d.S + K - 1) / K;
    const int64_t n_tiles = (lg.L + RANGE_TILE - 1) / RANGE_TILE;
    double best;
    int bestj;
    range_reduce(ws, slot, B - 1, n_tiles, s_v, s_j, best, bestj);
    if (threadIdx.x != 0) return;
    total_out[d.out_row] = best;
    const unsigned long long* stay = ws.stay + (int64_t)slot * ws.stay_slot;
    const int32_t* arg = ws.arg + (int64_t)slot * ws.arg_slot;
    int32_t* boff = block_offset_out + d.out_row * out_stride;
    int o = bestj;
    for (int64_t b = B - 1; b >= 0; --b) {
        boff[b] = o;
        if (b > 0 && !((stay[b * ws.stay_row + (o >> 6)] >> (o & 63)) & 1ull)) o = arg[b - 1];
    }
}

// one wave per block b < out_stride: n11 at the chosen lag (one subtitle word per lane and step), m_b, the int32 lag;
// entries b >= B are written as 0.  grid = (ceil(out_stride / waves), pairs)
__global__ void __launch_bounds__(RANGE_SCORE_THREADS) k_range_scores(const SplitDesc* __restrict__ desc,
                                                                     const RangeLag* __restrict__ lags, int K,
                                                                     int64_t out_stride,
                                                                     int32_t* __restrict__ block_offset_out,
                                                                     double* __restrict__ block_score_out) {
    const int slot = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (RANGE_SCORE_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= out_stride) return;  // (uniform per wave)
    const SplitDesc d = desc[slot];
    const int64_t B = (d.S + K - 1) / K;
    int32_t* boff = block_offset_out + d.out_row * out_stride;
    double* bsc = block_score_out + d.out_row * out_stride;
    if (b >= B) {
        if (lane == 0) {
            boff[b] = 0;
            bsc[b] = 0.0;
        }
        return;
    }
    const int64_t lag = lags[slot].lag_lo + boff[b];
    const int kw = K >> 5;
    int32_t n11 = 0;
    for (int w = lane; w < kw; w += 64) {
        const int64_t x = b * K + 32 * (int64_t)w + lag;  // reference sample of the word's first subtitle sample
        const int64_t g = x >= 0 ? (x >> 5) : -((31 - x) >> 5);
        const uint32_t ref = __builtin_amdgcn_alignbit(split_word(d.r, d.R, g + 1), split_word(d.r, d.R, g), (int)(x - g * 32));
        n11 += __popc(ref & split_word(d.s, d.S, b * kw + w));
    }
    for (int s = 32; s >= 1; s >>= 1) n11 += __shfl_xor(n11, s, 64);
    if (lane == 0) {
        bsc[b] = range_score(d, b, lag, n11, K);
        boff[b] = (int32_t)lag;
    }
}

}  // namespace ffsa
