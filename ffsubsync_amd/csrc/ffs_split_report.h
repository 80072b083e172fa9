// ffs_split_report.h -- per-piece quality report of a split solve (gfx950): for every piece of the split DP's answer, the
// correlation curve of the piece's own subtitle samples over the whole lag window, its moments and greedy peaks, and the
// piece's score at its neighbours' offsets (break evidence).  The contract is this library's own, pinned against the
// numpy model tests/split_report_model.py.
//
// Piece i of a pair: a maximal run [f_i, e_i) of equal block offsets o_b of the DP's backtrack, subtitle samples
// [f_i K, min(e_i K, S)), offset o_i.  Its curve c_i(d), d in [-W+1, W] (lag index j = d + W - 1): the counts of the
// piece's samples i with 0 <= i+d < R, n11 = sum over the piece's blocks of the split's uint16 block counts (exact, in
// uint32), and split_mix's fp64 expression -- every operation rounded on its own -- or exactly 0.0 where the overlap is
// empty.  Moments and peaks follow k_quality_peaks (quality_curve_moments / quality_curve_peaks: two-pass mean and
// population std, greedy peaks with exclusion distance E, largest lag on ties).
//
// Three kernels per sub-batch of pairs, after k_split_dp (the counts and prefix popcounts are still in the workspace):
//   k_split_pieces       one workgroup per pair: marks the blocks where o_b changes, numbers the pieces with a
//                        workgroup scan (wave ballots), writes each piece's first / end block and sample and offset into
//                        its report record, zeroes the records past the last piece and stores the piece count.
//   k_split_piece_sums   each thread owns two lags and walks the blocks in order, summing the uint16 counts (one 32-bit
//                        load per block) into uint32; at every piece end it stores the piece's n11 row.  Rows are indexed
//                        by piece, so the workspace is one uint32 row per block (2x the counts) whatever the piece count.
//   k_split_piece_report one workgroup per (pair, piece slot; slots past the piece count return at once): scores the
//                        piece's lags on the fly from its n11 row and the prefix popcounts, twice for the moments and
//                        once per peak round, then scores the own and the two neighbour offsets.
#pragma once
#include "ffs_kernels.h"
#include "ffs_quality.h"
#include "ffs_split.h"

namespace ffsa {

constexpr int PIECE_SCAN_THREADS = 1024;        // k_split_pieces workgroup (one per pair)
constexpr int PIECE_SUM_THREADS = 256;          // k_split_piece_sums workgroup
constexpr int PIECE_SUM_TILE = 2 * PIECE_SUM_THREADS;  // lags per workgroup (two per thread)
constexpr int32_t PIECE_OWN_NOT_PEAK = 4;       // FFS_PIECE_OWN_NOT_PEAK

struct PieceReport {  // = ffs_piece_report
    int64_t first_block, end_block;
    int64_t start_sample, end_sample;
    int64_t offset;
    double own_score, prev_score, next_score;
    double mean, std;
    int64_t n_lags;
    double peak_score[QUAL_MAX_PEAKS];
    int64_t peak_offset[QUAL_MAX_PEAKS];
    int32_t n_peaks, flags;
};
static_assert(sizeof(PieceReport) == 224, "PieceReport must match ffs_piece_report");

// piece table of one pair per workgroup: records [0, n) get their block / sample range and offset, [n, out_stride) zero
__global__ void __launch_bounds__(PIECE_SCAN_THREADS) k_split_pieces(const SplitDesc* __restrict__ desc, int K,
                                                                     int64_t out_stride,
                                                                     const int32_t* __restrict__ block_offset,
                                                                     PieceReport* __restrict__ report,
                                                                     int32_t* __restrict__ n_pieces_out) {
    constexpr int NW = PIECE_SCAN_THREADS / 64;
    __shared__ int s_cnt[NW];
    const SplitDesc d = desc[blockIdx.x];
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    PieceReport* rec = report + d.out_row * out_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;  // pieces that start before this chunk of blocks
    for (int64_t b0 = 0; b0 < B; b0 += PIECE_SCAN_THREADS) {
        const int64_t b = b0 + t;
        const bool in = b < B;
        const bool start = in && (b == 0 || o[b] != o[b - 1]);
        const bool last = in && (b == B - 1 || o[b + 1] != o[b]);
        const unsigned long long m = __ballot(start);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = carry, chunk = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            chunk += s_cnt[w];
        }
        // piece of block b: the starts at or before it, minus one
        const int idx = before + __popcll(m & ((2ull << lane) - 1ull)) - 1;
        if (start) {
            rec[idx].first_block = b;
            rec[idx].start_sample = b * K;
            rec[idx].offset = o[b];
        }
        if (last) {
            rec[idx].end_block = b + 1;
            rec[idx].end_sample = (b + 1) * K < d.S ? (b + 1) * K : d.S;
        }
        carry += chunk;
        __syncthreads();  // before the next chunk rewrites s_cnt
    }
    unsigned long long* words = (unsigned long long*)rec;
    constexpr int RW = (int)(sizeof(PieceReport) / 8);
    for (int64_t q = (int64_t)carry * RW + t; q < out_stride * RW; q += PIECE_SCAN_THREADS) words[q] = 0ull;
    if (t == 0) n_pieces_out[d.out_row] = carry;
}

// n11 of every piece at lag indices j, j+1 (j = 2 * thread of a 512-lag tile); grid.x = pairs * n_tiles
__global__ void __launch_bounds__(PIECE_SUM_THREADS) k_split_piece_sums(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                                        uint32_t* __restrict__ curves, int K, int64_t W,
                                                                        int n_tiles, int64_t out_stride,
                                                                        const int32_t* __restrict__ block_offset) {
    const int tile = blockIdx.x % n_tiles;
    const int slot = blockIdx.x / n_tiles;
    const SplitDesc d = desc[slot];
    const int64_t j = (int64_t)tile * PIECE_SUM_TILE + 2 * threadIdx.x;
    if (j >= 2 * W) return;  // (L = 2W is even: j + 1 < L too)
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    // lag pair (j, j+1) of each row: one aligned 32-bit load (rows of Lpad = 64k elements, j even), little-endian halves
    const uint32_t* crow = (const uint32_t*)(ws.counts + slot * ws.counts_slot + j);
    uint32_t* out = curves + slot * ws.counts_slot + j;
    const int64_t row32 = ws.counts_row / 2;
    uint32_t a0 = 0, a1 = 0;
    int64_t piece = 0;
    int32_t oc = o[0];
    for (int64_t b = 0; b < B; ++b) {
        const uint32_t v = crow[b * row32];
        a0 += v & 0xffffu;
        a1 += v >> 16;
        const bool end = b + 1 == B || o[b + 1] != oc;  // (uniform)
        if (end) {
            *(uint2*)(out + piece * ws.counts_row) = make_uint2(a0, a1);
            ++piece;
            a0 = a1 = 0;
            if (b + 1 < B) oc = o[b + 1];
        }
    }
}

// c_i at lag d: the counts of the piece's subtitle samples [lo, hi) that meet the reference; exactly 0.0 without any
FFS_DEV double split_piece_score(const SplitDesc& d, int64_t lo, int64_t hi, uint32_t n11, int64_t lag) {
    const int64_t a = lo > -lag ? lo : -lag;
    const int64_t e = hi < d.R - lag ? hi : d.R - lag;
    if (e <= a) return 0.0;
    const int64_t n1x = split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a);
    const int64_t nx1 = split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag);
    return split_mix(d, e - a, (int64_t)n11, n1x, nx1);
}

// one workgroup per (pair, piece slot): the piece's moments, peaks and own / neighbour scores; grid.x = pairs * n_slots
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_split_piece_report(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                                          const uint32_t* __restrict__ curves, int64_t W,
                                                                          int n_slots, int64_t out_stride, int top_k,
                                                                          int64_t exclusion,
                                                                          const int32_t* __restrict__ n_pieces,
                                                                          PieceReport* __restrict__ report) {
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    const int i = blockIdx.x % n_slots;
    const int slot = blockIdx.x / n_slots;
    const SplitDesc d = desc[slot];
    const int n = n_pieces[d.out_row];
    if (i >= n) return;  // (uniform)
    PieceReport* pr = report + d.out_row * out_stride;
    const int64_t lo = pr[i].start_sample, hi = pr[i].end_sample, off = pr[i].offset;
    const uint32_t* cv = curves + slot * ws.counts_slot + (int64_t)i * ws.counts_row;
    const int64_t L = 2 * W;
    auto score = [&](int64_t j) { return split_piece_score(d, lo, hi, cv[j], j - (W - 1)); };
    double mean, sd;
    bool flat;
    quality_curve_moments(L, score, score, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(L, score, top_k, exclusion, s_peak, s_pscore);
    if (threadIdx.x == 0) {
        PieceReport* rec = pr + i;
        rec->own_score = score(off + W - 1);
        rec->prev_score = i > 0 ? score(pr[i - 1].offset + W - 1) : __builtin_nan("");
        rec->next_score = i + 1 < n ? score(pr[i + 1].offset + W - 1) : __builtin_nan("");
        for (int k = 0; k < QUAL_MAX_PEAKS; ++k) {
            rec->peak_score[k] = k < n_peaks ? s_pscore[k] : 0.0;
            rec->peak_offset[k] = k < n_peaks ? s_peak[k] - (W - 1) : 0;
        }
        rec->mean = mean;
        rec->std = sd;
        rec->n_lags = L;
        rec->n_peaks = n_peaks;
        rec->flags = (flat ? QUAL_FLAT : 0) | (n_peaks == 0 || s_peak[0] - (W - 1) != off ? PIECE_OWN_NOT_PEAK : 0);
    }
}

}  // namespace ffsa
