// ffs_drift_range.h -- drift-tolerant alignment over any contiguous lag range [lag_lo, lag_hi], up to the full overlap
// range (gfx950): ffs_drift.h's DP (STAY, the moves +1, -1, ..., +s, -s at c_a = Q * a, JUMP; every comparison strict,
// the largest lag index on every maximum) over ffs_split_range.h's lag set and block scores (range_score: absent
// samples, split_mix without FMA).  At max_step = 0 the outputs are k_range_step's bit for bit, at [-W+1, W] they are
// k_drift_dp's.  Pinned against the numpy model tests/drift_range_model.py.
//
// The structure is ffs_split_range.h's: one plain launch per block step covering every pair in flight, one RANGE_TILE-lag
// tile per workgroup, the previous step's tile partials reduced by every workgroup itself (double-buffered by the parity
// of b), nothing to wait on inside a kernel.  What the moves change:
//   two V rows      a cell reads up to 2s + 1 cells of row b-1, cells of the neighbouring tile among them, so the row is
//                   no longer updated in place: ws.V holds two fp64 rows per pair (ws.v_slot = 2 row strides) used
//                   alternately by the parity of b.  Row b-1 was written by the previous launch, so V[j - e] is a plain
//                   global load, correct across wave and tile edges (coalesced, shifted by e: the lines are the ones the
//                   wave's own V[j] loads bring in).
//   codes           0 STAY, 2a-1 = +a, 2a = -a, 2s+1 JUMP (block b-1 sat at lag index j - e), stored as bit planes: one
//                   ballot per plane, wave and 64 lags, the planes of one 64-lag word next to each other
//                   ([slot][block][word][plane]; lanes 0..planes-1 store them).  A call at max_step = s uses
//                   ceil(log2(2s + 2)) planes (1, 2, 3, 3, 4, 4, 4, 4) and lays the rows out at that stride; the plan
//                   holds room for its max_step_cap.
//   k_range_drift_step       block b of every pair in flight.
//   k_range_drift_backtrack  one workgroup per pair: the last partials give the total and the end lag; thread 0 follows
//                            the codes back and writes lag indices and the jump flags.
// k_split_prefix before and k_range_scores after run unchanged.
#pragma once
#include "ffs_split_range.h"

namespace ffsa {

constexpr int DRIFT_RANGE_MAX_STEP = 7;

// bit planes that hold the codes 0 .. 2s + 1
constexpr int drift_range_planes(int s) { return s == 0 ? 1 : s == 1 ? 2 : s <= 3 ? 3 : 4; }

// one DP step (block b) of every pair in flight; grid = (max tiles, pairs).  ws.stay holds the code planes
// ([slot][block][ws.stay_row][planes]), ws.V two rows per slot.
__global__ void __launch_bounds__(RANGE_THREADS) k_range_drift_step(const SplitDesc* __restrict__ desc,
                                                                   const RangeLag* __restrict__ lags, RangeWs ws, int K,
                                                                   int64_t b, double P, int max_step, double Q,
                                                                   int planes) {
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
    const int64_t v_row = ws.v_slot >> 1;
    const double* Vp = ws.V + (int64_t)slot * ws.v_slot + ((b & 1) ^ 1) * v_row;  // row b-1: the previous launch wrote it
    double* Vc = ws.V + (int64_t)slot * ws.v_slot + (b & 1) * v_row;
    unsigned long long* codes = ws.stay + (int64_t)slot * ws.stay_slot + b * ws.stay_row * planes;
    const int code_jump = 2 * max_step + 1;
    double best = -INFINITY;
    int bestj = -1;
#pragma unroll
    for (int k = 0; k < RANGE_LPT; ++k) {
        const int64_t j0 = j_tile + RANGE_THREADS * k + 64 * wave;  // the wave's first lag index: a multiple of 64
        const int64_t j = j0 + lane;
        int code = 0;
        if (j < lg.L) {
            const double m = range_score(d, b, lg.lag_lo + j, acc[k], K);
            double v;
            if (b == 0) {
                v = m;
            } else {
                double top = Vp[j];
                for (int a = 1; a <= max_step; ++a) {  // smaller moves first, +a before -a; ties keep the earlier option
                    const double c = Q * (double)a;
                    if (j - a >= 0) {
                        const double cand = Vp[j - a] - c;
                        if (cand > top) {
                            top = cand;
                            code = 2 * a - 1;
                        }
                    }
                    if (j + a < lg.L) {
                        const double cand = Vp[j + a] - c;
                        if (cand > top) {
                            top = cand;
                            code = 2 * a;
                        }
                    }
                }
                if (T > top) {  // ties do not jump
                    top = T;
                    code = code_jump;
                }
                v = top + m;
            }
            Vc[j] = v;
            split_max_pair(best, bestj, v, (int)j);
        }
        if (b > 0) {  // (uniform)
            unsigned long long mine = 0;
            for (int pl = 0; pl < planes; ++pl) {
                const unsigned long long bits = __ballot((code >> pl) & 1);
                if (lane == pl) mine = bits;
            }
            if (lane < planes && j0 < lg.L) codes[(j0 >> 6) * planes + lane] = mine;
        }
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

// one workgroup per pair: total, end lag, the backtrack through the code planes (lag indices into the offset output
// for now: k_range_scores turns them into lags) and the jump flags; flags of blocks b >= B are written as 0
__global__ void __launch_bounds__(RANGE_THREADS) k_range_drift_backtrack(const SplitDesc* __restrict__ desc,
                                                                        const RangeLag* __restrict__ lags, RangeWs ws,
                                                                        int K, int64_t out_stride, int max_step, int planes,
                                                                        int32_t* __restrict__ block_offset_out,
                                                                        uint8_t* __restrict__ block_jump_out,
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
    uint8_t* bjump = block_jump_out + d.out_row * out_stride;
    for (int64_t b = B + threadIdx.x; b < out_stride; b += RANGE_THREADS) bjump[b] = 0;
    if (threadIdx.x != 0) return;
    total_out[d.out_row] = best;
    const unsigned long long* codes = ws.stay + (int64_t)slot * ws.stay_slot;
    const int32_t* arg = ws.arg + (int64_t)slot * ws.arg_slot;
    int32_t* boff = block_offset_out + d.out_row * out_stride;
    const int code_jump = 2 * max_step + 1;
    int o = bestj;
    for (int64_t b = B - 1; b >= 0; --b) {
        boff[b] = o;
        int code = 0;
        if (b > 0) {
            const unsigned long long* pl = codes + (b * ws.stay_row + (o >> 6)) * planes;
            for (int k = 0; k < planes; ++k) code |= (int)((pl[k] >> (o & 63)) & 1ull) << k;
        }
        bjump[b] = code == code_jump;
        if (code == code_jump) {
            o = arg[b - 1];
        } else if (code) {
            const int a = (code + 1) >> 1;
            o -= (code & 1) ? a : -a;  // block b-1 sat at lag index o - e
        }
    }
}

}  // namespace ffsa
