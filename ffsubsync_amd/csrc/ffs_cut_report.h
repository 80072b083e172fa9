// ffs_cut_report.h -- per-piece quality report of a split solve over any lag range [lag_lo, lag_hi], up to the full
// overlap range (gfx950).  The contract is ffs_split_report.h's with the lag set d = lag_lo + j, j in [0, L),
// L = lag_hi - lag_lo + 1 (lags without overlap score exactly 0.0 and count in the moments); at [-W+1, W] the records
// are bit-identical to k_split_piece_report's.  Pinned against the numpy model tests/cut_report_model.py and against the
// independent reference tests/report_reference.py (interval correlations from their definition).
//
// k_split_piece_sums sums the split's stored block counts; the range split stores none (3.8), and storing them at the
// full range would take 4 GB per 2 h pair.  Here each piece's n11 row is counted from the bits instead, for the pieces
// of one round at a time (CUT_ROUND_PIECES slots per pair: the row workspace does not depend on the piece count):
//   k_split_pieces      (ffs_split_report.h) the piece table into the caller's records, as for the windowed report.
//   k_cut_piece_counts  one work item (a chunk of at most CUT_CHUNK_WORDS subtitle words inside one piece of the round)
//                       x one 4096-lag tile per workgroup: k_quality_counts' scheme -- the chunk and the reference window
//                       it meets staged in LDS, thread q holds the 32 lags 32q..32q+31 of the tile (v_alignbit +
//                       v_bcnt), an LDS transpose, integer atomicAdd into the piece's row (exact, order-free).  The work
//                       items come from the host, which reads the block offsets back once per call.
//   k_cut_piece_report  one workgroup per (pair, piece slot of the round; slots past the piece count return at once):
//                       k_split_piece_report with the lag of index j at lag_lo + j.
#pragma once
#include "ffs_kernels.h"
#include "ffs_quality.h"
#include "ffs_split.h"
#include "ffs_split_range.h"
#include "ffs_split_report.h"

namespace ffsa {

constexpr int CUT_ROUND_PIECES = 8;    // piece rows per pair and round
constexpr int CUT_CHUNK_WORDS = 512;   // subtitle words per work item (at most)
constexpr int CUT_MAX_ITEMS = 65535;   // work items per k_cut_piece_counts launch (grid.y)

struct CutItem {
    int64_t g0;    // first subtitle word of the chunk
    int32_t row;   // slot * CUT_ROUND_PIECES + the piece's place in the round
    int32_t nw;    // words in the chunk (1 .. CUT_CHUNK_WORDS)
};

// n11 of one piece chunk over one 4096-lag tile of its pair's range; grid = (tiles, items of this launch)
__global__ void __launch_bounds__(QUAL_CNT_THREADS) k_cut_piece_counts(const SplitDesc* __restrict__ desc,
                                                                       const RangeLag* __restrict__ lags,
                                                                       const CutItem* __restrict__ items,
                                                                       uint32_t* __restrict__ rows, int64_t row_stride) {
    __shared__ uint32_t s_sub[CUT_CHUNK_WORDS];
    __shared__ uint32_t s_ref[CUT_CHUNK_WORDS + QUAL_CNT_THREADS + 1];
    __shared__ uint32_t s_acc[QUAL_CNT_THREADS * 33];  // [q][sh], rows padded to 33 words against bank conflicts
    const CutItem it = items[blockIdx.y];
    const int slot = it.row / CUT_ROUND_PIECES;
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int64_t l0 = (int64_t)blockIdx.x * QUAL_TILE;  // first lag index of the tile
    if (l0 >= lg.L) return;                              // (uniform)
    const int nw = it.nw;
    // reference bits [base + 32 q, +32) for q <= nw + QUAL_CNT_THREADS meet subtitle word g0 + w at tile lag 32 q' + sh
    const int64_t base = 32 * it.g0 + lg.lag_lo + l0;
    if (base + 32 * (int64_t)(nw + QUAL_CNT_THREADS + 1) <= 0 || base >= d.R) return;  // no reference sample reachable
    const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
    const int bsh = (int)(base - gbase * 32);
    const int t = threadIdx.x;
    for (int q = t; q <= nw + QUAL_CNT_THREADS; q += QUAL_CNT_THREADS) {
        const uint32_t lo = split_word(d.r, d.R, gbase + q), hi = split_word(d.r, d.R, gbase + q + 1);
        s_ref[q] = __builtin_amdgcn_alignbit(hi, lo, bsh);
    }
    for (int w = t; w < nw; w += QUAL_CNT_THREADS) s_sub[w] = split_word(d.s, d.S, it.g0 + w);
    __syncthreads();
    uint32_t acc[32];
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) acc[sh] = 0;
    uint32_t lo = s_ref[t];
    for (int w = 0; w < nw; ++w) {
        const uint32_t sw = s_sub[w];  // (one address per wave: broadcast)
        const uint32_t hi = s_ref[t + w + 1];
#pragma unroll
        for (int sh = 0; sh < 32; ++sh) acc[sh] += __popc(__builtin_amdgcn_alignbit(hi, lo, sh) & sw);
        lo = hi;
    }
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) s_acc[t * 33 + sh] = acc[sh];
    __syncthreads();
    uint32_t* out = rows + (int64_t)it.row * row_stride + l0;
    const int64_t n_here = lg.L - l0 < QUAL_TILE ? lg.L - l0 : QUAL_TILE;
    for (int l = t; l < n_here; l += QUAL_CNT_THREADS) {
        const uint32_t v = s_acc[(l >> 5) * 33 + (l & 31)];
        if (v) atomicAdd(out + l, v);
    }
}

// one workgroup per (pair, piece slot of the round): the piece's moments, peaks and own / neighbour scores over its
// pair's lag range; grid.x = pairs * CUT_ROUND_PIECES
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_cut_piece_report(const SplitDesc* __restrict__ desc,
                                                                        const RangeLag* __restrict__ lags,
                                                                        const uint32_t* __restrict__ rows,
                                                                        int64_t row_stride, int first_piece,
                                                                        int64_t out_stride, int top_k, int64_t exclusion,
                                                                        const int32_t* __restrict__ n_pieces,
                                                                        PieceReport* __restrict__ report) {
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    const int g = blockIdx.x % CUT_ROUND_PIECES;
    const int slot = blockIdx.x / CUT_ROUND_PIECES;
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int n = n_pieces[d.out_row];
    const int i = first_piece + g;
    if (i >= n) return;  // (uniform)
    PieceReport* pr = report + d.out_row * out_stride;
    const int64_t lo = pr[i].start_sample, hi = pr[i].end_sample, off = pr[i].offset;
    const uint32_t* cv = rows + (int64_t)blockIdx.x * row_stride;
    // (the host has checked every block offset against the range: the own and neighbour lag indices are in [0, L))
    auto score = [&](int64_t j) { return split_piece_score(d, lo, hi, cv[j], j + lg.lag_lo); };
    double mean, sd;
    bool flat;
    quality_curve_moments(lg.L, score, score, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(lg.L, score, top_k, exclusion, s_peak, s_pscore);
    if (threadIdx.x == 0) {
        PieceReport* rec = pr + i;
        rec->own_score = score(off - lg.lag_lo);
        rec->prev_score = i > 0 ? score(pr[i - 1].offset - lg.lag_lo) : __builtin_nan("");
        rec->next_score = i + 1 < n ? score(pr[i + 1].offset - lg.lag_lo) : __builtin_nan("");
        for (int k = 0; k < QUAL_MAX_PEAKS; ++k) {
            rec->peak_score[k] = k < n_peaks ? s_pscore[k] : 0.0;
            rec->peak_offset[k] = k < n_peaks ? s_peak[k] + lg.lag_lo : 0;
        }
        rec->mean = mean;
        rec->std = sd;
        rec->n_lags = lg.L;
        rec->n_peaks = n_peaks;
        rec->flags = (flat ? QUAL_FLAT : 0) | (n_peaks == 0 || s_peak[0] + lg.lag_lo != off ? PIECE_OWN_NOT_PEAK : 0);
    }
}

}  // namespace ffsa
