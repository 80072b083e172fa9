// ffs_drift.h -- drift-tolerant alignment: the split DP of ffs_split.h with small offset steps between blocks (gfx950).
// Upstream has no equivalent; the contract is this library's own, pinned against the numpy model tests/drift_model.py.
//
// Everything before the DP is ffs_split.h's, unchanged: k_split_prefix, k_split_counts, split_score (the no-FMA fp64
// block score m_b(d)).  The DP gains one kind of move.  With s = max_step in [0, 7], Q = step_cost >= 0 and
// c_a = Q * a (one fp64 product):  V_0 = m_0;  for b >= 1, J = max of row b-1 (largest lag index on ties), T = J - P,
//     best, code = V_{b-1}(j), STAY
//     for a = 1..s, for e in (+a, -a):  if 0 <= j-e < L and V_{b-1}(j-e) - c_a > best: best, code = that, e
//     if T > best: best, code = T, JUMP
//     V_b(j) = best + m_b(j)
// every comparison strict (ties keep the earlier option), every fp64 operation rounded on its own.  Backtrack from the
// largest argmax of the last row: JUMP -> argmax of row b-1, else o_{b-1} = o_b - e.  At s = 0 this is k_split_dp.
//
//   k_drift_dp   one workgroup per pair, as k_split_dp.  V is two rows of the workspace used alternately (a cell reads
//                cells of the previous row that other threads wrote; the block step's barrier orders them).  A wave holds
//                64 neighbouring lags of the previous row, one per lane, and the s cells beyond either end of its span in
//                one more register (lanes < s: V[j + 64], lanes >= 64 - s: V[j - 64] -- one extra load per sweep); the
//                neighbour at distance a is ONE 64-bit rotate of the wave (ds_bpermute) whose wrapped-around lanes
//                offer their edge value instead of their own.  The 4-bit code of a cell (0 STAY, 2a-1 = +a, 2a = -a,
//                15 JUMP) is stored as four bit planes: four wave ballots = 64 lags x 4 bits in four 64-bit words, written
//                by lanes 0..3 in one store.  Thread 0 backtracks through the planes and writes the jump flags.
#pragma once
#include "ffs_split.h"

namespace ffsa {

constexpr int DRIFT_MAX_STEP = 7;
constexpr int DRIFT_CODE_JUMP = 15;
constexpr int DRIFT_PLANES = 4;  // 64-bit words per 64 lags of one block's codes

// one workgroup per pair: the DP over the blocks, backtrack, per-block outputs.  ws.V holds two rows per slot
// (ws.v_slot = 2 * row stride), ws.stay is not used; codes: [slot][block][ws.stay_row][DRIFT_PLANES]
__global__ void __launch_bounds__(SPLIT_DP_THREADS) k_drift_dp(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                              unsigned long long* __restrict__ codes_base,
                                                              int64_t codes_slot, int K, int64_t W, double P, int max_step,
                                                              double Q, int64_t out_stride,
                                                              int32_t* __restrict__ block_offset_out,
                                                              double* __restrict__ block_score_out,
                                                              uint8_t* __restrict__ block_jump_out,
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
    unsigned long long* codes = codes_base + slot * codes_slot;
    const int64_t v_row = ws.v_slot >> 1;
    double* V = ws.V + slot * ws.v_slot;
    int32_t* arg = ws.arg + slot * ws.arg_slot;
    const bool is_edge = lane < max_step || lane >= 64 - max_step;  // (max_step <= 7: the two sets are disjoint)
    double T = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const uint16_t* crow = counts + b * ws.counts_row;
        const double* Vp = V + ((b & 1) ^ 1) * v_row;  // row b-1
        double* Vc = V + (b & 1) * v_row;
        double best = -INFINITY;
        int bestj = -1;
        for (int64_t j0 = (int64_t)wave * 64; j0 < words * 64; j0 += SPLIT_DP_THREADS) {  // whole waves: shuffles and ballots are exact
            const int64_t j = j0 + lane;
            const bool in = j < L;
            int code = 0;
            if (b == 0) {
                if (in) {
                    const double v = split_score(d, crow, b, j, K, W);
                    Vc[j] = v;
                    split_max_pair(best, bestj, v, (int)j);
                }
                continue;  // (uniform)
            }
            const double m = in ? split_score(d, crow, b, j, K, W) : 0.0;
            const double vp = in ? Vp[j] : 0.0;
            double top = vp;
            if (max_step > 0) {  // (uniform)
                const int64_t je = lane < max_step ? j + 64 : j - 64;
                const double edge = (is_edge && je >= 0 && je < L) ? Vp[je] : 0.0;
                for (int a = 1; a <= max_step; ++a) {
                    const double c = Q * (double)a;
                    // V[j - a]: lane - a, the a lanes that wrap offer V[their j - 64]; V[j + a] likewise
                    const double up = __shfl(lane >= 64 - a ? edge : vp, (lane - a) & 63, 64);
                    const double dn = __shfl(lane < a ? edge : vp, (lane + a) & 63, 64);
                    if (j - a >= 0) {
                        const double cand = up - c;
                        if (cand > top) {
                            top = cand;
                            code = 2 * a - 1;
                        }
                    }
                    if (j + a < L) {
                        const double cand = dn - c;
                        if (cand > top) {
                            top = cand;
                            code = 2 * a;
                        }
                    }
                }
            }
            if (T > top) {  // ties do not jump
                top = T;
                code = DRIFT_CODE_JUMP;
            }
            if (in) {
                const double v = top + m;
                Vc[j] = v;
                split_max_pair(best, bestj, v, (int)j);
            } else {
                code = 0;
            }
            const unsigned long long p0 = __ballot(code & 1), p1 = __ballot(code & 2), p2 = __ballot(code & 4),
                                     p3 = __ballot(code & 8);
            if (lane < DRIFT_PLANES)
                codes[(b * words + (j0 >> 6)) * DRIFT_PLANES + lane] = lane == 0 ? p0 : lane == 1 ? p1 : lane == 2 ? p2 : p3;
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
    uint8_t* bjump = block_jump_out + d.out_row * out_stride;
    if (t == 0) {
        total_out[d.out_row] = s_best;
        int o = s_bestj;
        for (int64_t b = B - 1; b >= 0; --b) {
            boff[b] = o;  // lag index for now; turned into the lag below
            int code = 0;
            if (b > 0) {
                const unsigned long long* pl = codes + (b * words + (o >> 6)) * DRIFT_PLANES;
                const int sh = o & 63;
                code = (int)(((pl[0] >> sh) & 1ull) | (((pl[1] >> sh) & 1ull) << 1) | (((pl[2] >> sh) & 1ull) << 2) |
                             (((pl[3] >> sh) & 1ull) << 3));
            }
            bjump[b] = code == DRIFT_CODE_JUMP;
            if (code == DRIFT_CODE_JUMP) {
                o = arg[b - 1];
            } else if (code) {
                const int a = (code + 1) >> 1;
                o -= (code & 1) ? a : -a;  // block b-1 sat at lag index o - e
            }
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
            bjump[b] = 0;
        }
    }
}

}  // namespace ffsa
