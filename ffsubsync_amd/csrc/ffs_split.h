// ffs_split.h -- split-aware alignment: piecewise-constant offsets for subtitle files whose video has breaks or cuts
// (gfx950).  Upstream has no equivalent: the reference finds ONE offset per file (its README's "Limitations"); the
// contract below is this library's own, pinned against the numpy model tests/split_model.py.
//
// Problem (per pair): two-level reference r (R samples) and subtitle vector s (S samples), block length K (multiple of
// 32), lag window d in [-W+1, W] (lag index j = d + W - 1 in [0, L), L = 2W).  Block b = subtitle samples
// [bK, min((b+1)K, S)).  For each (b, d), over the samples i of block b with 0 <= i+d < R (samples outside the reference
// are absent, not zeros), count ov, n11 (both bits set), n1x (subtitle bit set), nx1 (reference bit set), and score
//     m_b(d) = ((n00*c00 + n01*c01) + n10*c10) + n11*c11,   c_xy = (2 lvl_s[x] - 1) * (2 lvl_r[y] - 1)
// in fp64, every product and sum rounded on its own (no FMA: the model reproduces every value bit for bit).
// Dynamic programme: V_0 = m_0; V_b(d) = (V_{b-1}(d) >= J_{b-1} - P ? V_{b-1}(d) : J_{b-1} - P) + m_b(d), J = max of the
// row (largest lag on ties), one stay bit per (b, d); backtrack from the largest argmax of the last row.
//
// Three kernels per sub-batch of pairs (the plan's pairs_in_flight):
//   k_split_prefix  per vector (s, and the part of r the window can reach): exclusive popcount prefix per 32-bit word,
//                   so the DP derives ov / n1x / nx1 of any (block, lag) from four prefix reads -- nothing but n11 is stored.
//   k_split_counts  n11 of every (block, lag) as uint16 (K <= 32 768): a workgroup stages one block's subtitle words and
//                   the reference window of a 1024-lag tile in LDS and walks SPLIT_BPW blocks; each thread holds four
//                   lags, the reference word of a lag is a funnel shift (v_alignbit) of two staged words, reused by the
//                   next word step, the count a v_bcnt accumulate.
//   k_split_dp      one workgroup per pair walks the blocks in order: V (fp64, one row of L) lives in the workspace,
//                   each block step scores its lags, writes one stay bit per lag (a wave ballot = 64 lags per store) and
//                   reduces the row maximum with the largest-lag tie rule (shuffles, then LDS across the waves); thread 0
//                   backtracks through the stay bits, then all threads score the chosen lag of every block.
#pragma once
#include "ffs_kernels.h"

namespace ffsa {

constexpr int SPLIT_CNT_THREADS = 256;              // k_split_counts workgroup
constexpr int SPLIT_LPT = 4;                        // lags per thread
constexpr int SPLIT_TILE = SPLIT_CNT_THREADS * SPLIT_LPT;  // lags per workgroup (1024 = 32 words of reference bits)
constexpr int SPLIT_BPW = 4;                        // blocks walked per workgroup
constexpr int SPLIT_MAX_K = 32768;
constexpr int SPLIT_DP_THREADS = 1024;              // k_split_dp workgroup (one per pair)
constexpr int SPLIT_PREFIX_THREADS = 1024;

struct SplitDesc {
    const uint32_t* r;  // reference bits (FFS_DTYPE_U1)
    const uint32_t* s;  // subtitle bits
    int64_t R, S;
    double c00, c01, c10, c11;  // (2 lvl_s - 1) * (2 lvl_r - 1) for (s bit, r bit) = (0,0), (0,1), (1,0), (1,1)
    int32_t* pre_r;     // workspace: exclusive word prefix popcounts of r over its first min(R, S+W) samples
    int32_t* pre_s;     // ... of s
    int64_t out_row;    // pair index in the caller's outputs
};

struct SplitWs {
    uint16_t* counts;   // [slot][max_blocks][Lpad]
    unsigned long long* stay;  // [slot][max_blocks][Lpad / 64]
    double* V;          // [slot][Lpad]
    int32_t* arg;       // [slot][max_blocks]: lag index of the row maximum after block b
    int64_t counts_row, stay_row;  // per-block strides in elements (Lpad, Lpad / 64)
    int64_t counts_slot, stay_slot, v_slot, arg_slot;  // per-slot strides in elements
};

// word g of a bit vector of n samples: 0 outside [0, ceil(n/32)), tail bits of the last word cleared
FFS_DEV uint32_t split_word(const uint32_t* v, int64_t n, int64_t g) {
    if (g < 0 || g >= ((n + 31) >> 5)) return 0u;
    uint32_t w = v[g];
    const int tail = (int)(n & 31);
    if (g == (n >> 5) && tail) w &= (1u << tail) - 1u;
    return w;
}

// popcount of samples [0, x) from the exclusive word prefix (x in [0, n])
FFS_DEV int32_t split_prefix_at(const int32_t* pre, const uint32_t* v, int64_t x) {
    const int64_t g = x >> 5;
    const int sh = (int)(x & 31);
    int32_t c = pre[g];
    if (sh) c += __popc(v[g] & ((1u << sh) - 1u));  // bits below x are inside the vector: no tail mask needed
    return c;
}

// one vector per workgroup: pre[g] = popcount of words [0, g) for g in [0, ceil(n/32)]
__global__ void __launch_bounds__(SPLIT_PREFIX_THREADS) k_split_prefix(const SplitDesc* __restrict__ desc, int64_t W) {
    __shared__ int32_t s_part[SPLIT_PREFIX_THREADS];
    const SplitDesc d = desc[blockIdx.x >> 1];
    const bool is_ref = blockIdx.x & 1;
    const uint32_t* v = is_ref ? d.r : d.s;
    const int64_t n = is_ref ? (d.R < d.S + W ? d.R : d.S + W) : d.S;
    int32_t* pre = is_ref ? d.pre_r : d.pre_s;
    const int64_t nw = (n + 31) >> 5;
    const int64_t per = (nw + SPLIT_PREFIX_THREADS - 1) / SPLIT_PREFIX_THREADS;
    const int t = threadIdx.x;
    const int64_t w0 = t * per, w1 = (w0 + per < nw) ? w0 + per : nw;
    int32_t sum = 0;
    for (int64_t g = w0; g < w1; ++g) sum += __popc(split_word(v, n, g));
    s_part[t] = sum;
    __syncthreads();
    for (int off = 1; off < SPLIT_PREFIX_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan of the chunk sums
        const int32_t add = t >= off ? s_part[t - off] : 0;
        __syncthreads();
        s_part[t] += add;
        __syncthreads();
    }
    int32_t run = s_part[t] - sum;
    for (int64_t g = w0; g < w1; ++g) {
        pre[g] = run;
        run += __popc(split_word(v, n, g));
    }
    if (t == SPLIT_PREFIX_THREADS - 1) pre[nw] = s_part[t];
}

// n11 of (block b, lag index j) for SPLIT_BPW blocks x one 1024-lag tile; grid.x = pairs * block groups * tiles
__global__ void __launch_bounds__(SPLIT_CNT_THREADS) k_split_counts(const SplitDesc* __restrict__ desc, SplitWs ws, int K,
                                                                    int64_t W, int n_tiles, int n_bgroups) {
    __shared__ uint32_t s_sub[SPLIT_MAX_K / 32];
    __shared__ uint32_t s_ref[SPLIT_MAX_K / 32 + SPLIT_TILE / 32 + 1];
    const int tile = blockIdx.x % n_tiles;
    const int bgroup = (blockIdx.x / n_tiles) % n_bgroups;
    const int slot = blockIdx.x / (n_tiles * n_bgroups);
    const SplitDesc d = desc[slot];
    const int64_t L = 2 * W;
    const int64_t B = (d.S + K - 1) / K;
    const int kw = K >> 5;
    const int n_ref_words = kw + SPLIT_TILE / 32 + 1;
    const int t = threadIdx.x;
    const int q0 = t >> 5, sh = t & 31;
    const int64_t j_tile = (int64_t)tile * SPLIT_TILE;
    const int64_t d_tile = j_tile - (W - 1);  // lag of the tile's first lag index
    uint16_t* out_slot = ws.counts + slot * ws.counts_slot;
    for (int bi = 0; bi < SPLIT_BPW; ++bi) {
        const int64_t b = (int64_t)bgroup * SPLIT_BPW + bi;
        if (b >= B) break;  // (uniform)
        // reference bits [b*K + d_tile + 32 q, +32) for q < n_ref_words, zero outside [0, R)
        const int64_t base = b * K + d_tile;
        const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
        const int bsh = (int)(base - gbase * 32);
        for (int q = t; q < n_ref_words; q += SPLIT_CNT_THREADS) {
            const uint32_t lo = split_word(d.r, d.R, gbase + q), hi = split_word(d.r, d.R, gbase + q + 1);
            s_ref[q] = __builtin_amdgcn_alignbit(hi, lo, bsh);
        }
        for (int q = t; q < kw; q += SPLIT_CNT_THREADS) s_sub[q] = split_word(d.s, d.S, b * kw + q);
        __syncthreads();
        // lag offset t + 256k inside the tile: reference word q0 + 8k + w of the staged window, shifted by sh
        uint32_t lo[SPLIT_LPT], acc[SPLIT_LPT];
#pragma unroll
        for (int k = 0; k < SPLIT_LPT; ++k) {
            lo[k] = s_ref[q0 + 8 * k];
            acc[k] = 0;
        }
        for (int w = 0; w < kw; ++w) {
            const uint32_t sw = s_sub[w];  // (one address per wave: broadcast)
#pragma unroll
            for (int k = 0; k < SPLIT_LPT; ++k) {
                const uint32_t hi = s_ref[q0 + 8 * k + w + 1];
                acc[k] += __popc(__builtin_amdgcn_alignbit(hi, lo[k], sh) & sw);
                lo[k] = hi;
            }
        }
        uint16_t* row = out_slot + b * ws.counts_row;
#pragma unroll
        for (int k = 0; k < SPLIT_LPT; ++k) {
            const int64_t j = j_tile + t + SPLIT_CNT_THREADS * k;
            if (j < L) row[j] = (uint16_t)acc[k];
        }
        __syncthreads();  // before the next block restages the LDS
    }
}

// ((n00*c00 + n01*c01) + n10*c10) + n11*c11 of the counts of an overlap of ov samples
FFS_DEV double split_mix(const SplitDesc& d, int64_t ov, int64_t n11, int64_t n1x, int64_t nx1) {
#pragma clang fp contract(off)
    const int64_t n10 = n1x - n11, n01 = nx1 - n11, n00 = ov - n11 - n10 - n01;
    // plain operators under the pragma: __dmul_rn / __dadd_rn are defined where contraction is on, and once inlined
    // their products fuse with the sums (v_fmac_f64)
    return (((double)n00 * d.c00 + (double)n01 * d.c01) + (double)n10 * d.c10) + (double)n11 * d.c11;
}

// m_b(d) of lag index j (d = j - W + 1): n11 from the counts, ov / n1x / nx1 from the prefix popcounts
FFS_DEV double split_score(const SplitDesc& d, const uint16_t* counts_row, int64_t b, int64_t j, int K, int64_t W) {
    const int64_t lag = j - (W - 1);
    const int64_t blo = b * K, bhi = (blo + K < d.S) ? blo + K : d.S;
    const int64_t a = blo > -lag ? blo : -lag;
    const int64_t e = bhi < d.R - lag ? bhi : d.R - lag;
    int64_t ov = 0, n11 = 0, n1x = 0, nx1 = 0;
    if (e > a) {
        ov = e - a;
        n11 = counts_row[j];
        n1x = split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a);
        nx1 = split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag);
    }
    return split_mix(d, ov, n11, n1x, nx1);
}

// (value, lag index) maximum with the largest index on ties
FFS_DEV void split_max_pair(double& v, int& j, double ov, int oj) {
    if (ov > v || (ov == v && oj > j)) {
        v = ov;
        j = oj;
    }
}

// one workgroup per pair: the DP over the blocks, backtrack, per-block outputs
__global__ void __launch_bounds__(SPLIT_DP_THREADS) k_split_dp(const SplitDesc* __restrict__ desc, SplitWs ws, int K,
                                                              int64_t W, double P, int64_t out_stride,
                                                              int32_t* __restrict__ block_offset_out,
                                                              double* __restrict__ block_score_out,
                                                              double* __restrict__ total_out) {
#pragma clang fp contract(off)
    constexpr int NW = SPLIT_DP_THREADS / 64;
    __shared__ double s_v[NW];
    __shared__ int s_j[NW];
    __shared__ double s_best;
    __shared__ int s_bestj;
    const int slot = blockIdx.x;
    const SplitDesc d = desc[slot];
    const int64_t L = 2 * W;
    const int64_t words = ws.stay_row;  // 64-lag words per block row
    const int64_t B = (d.S + K - 1) / K;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint16_t* counts = ws.counts + slot * ws.counts_slot;
    unsigned long long* stay = ws.stay + slot * ws.stay_slot;
    double* V = ws.V + slot * ws.v_slot;
    int32_t* arg = ws.arg + slot * ws.arg_slot;
    double T = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const uint16_t* crow = counts + b * ws.counts_row;
        double best = -INFINITY;
        int bestj = -1;
        for (int64_t j0 = (int64_t)wave * 64; j0 < words * 64; j0 += SPLIT_DP_THREADS) {  // whole waves: the ballot is exact
            const int64_t j = j0 + lane;
            bool st = false;
            if (j < L) {
                const double m = split_score(d, crow, b, j, K, W);
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
            if (b > 0 && lane == 0) stay[b * words + (j0 >> 6)] = bits;
        }
        for (int s = 32; s >= 1; s >>= 1) split_max_pair(best, bestj, __shfl_xor(best, s, 64), __shfl_xor(bestj, s, 64));
        if (lane == 0) {
            s_v[wave] = best;
            s_j[wave] = bestj;
        }
        __syncthreads();
        if (t == 0) {
            double v = s_v[0];
            int jj = s_j[0];
            for (int w = 1; w < NW; ++w) split_max_pair(v, jj, s_v[w], s_j[w]);
            s_best = v;
            s_bestj = jj;
            arg[b] = jj;
        }
        __syncthreads();
        T = s_best - P;
    }
    int32_t* boff = block_offset_out + d.out_row * out_stride;
    double* bsc = block_score_out + d.out_row * out_stride;
    if (t == 0) {
        total_out[d.out_row] = s_best;
        int o = s_bestj;
        for (int64_t b = B - 1; b >= 0; --b) {
            boff[b] = o;  // lag index for now; turned into the lag below
            if (b > 0 && !((stay[b * words + (o >> 6)] >> (o & 63)) & 1ull)) o = arg[b - 1];
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int64_t b = t; b < out_stride; b += SPLIT_DP_THREADS) {
        if (b < B) {
            const int j = boff[b];
            bsc[b] = split_score(d, counts + b * ws.counts_row, b, j, K, W);
            boff[b] = (int32_t)(j - (W - 1));
        } else {
            boff[b] = 0;
            bsc[b] = 0.0;
        }
    }
}

}  // namespace ffsa
