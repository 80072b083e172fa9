// ffs_drift_report.h -- per-segment path report of a drift solve (gfx950): for every segment of the drift DP's answer, the
// correlation curve of the segment's own subtitle samples over every SHIFT of its whole path that stays inside the lag
// window, its moments and greedy peaks, the curve at the shifts that would continue a neighbouring segment without a
// jump (jump evidence) and the best CONSTANT lag among those the path visits (drift evidence).  The contract is this
// library's own, pinned against the numpy model tests/drift_report_model.py and, independently of the count table and the
// row indexing below, against tests/report_reference.py (sums of block scores from their definition).
//
// Segment i of a pair: a maximal run [f_i, e_i) of blocks with no jump inside (block_jump of k_drift_dp), subtitle samples
// [f_i K, min(e_i K, S)), block offsets o_b with o_min / o_max over the run.  Shift set delta in [-W+1-o_min, W-o_max]
// (n = 2W - (o_max - o_min) >= 1 shifts, shift index t = delta - delta_lo): exactly the shifts for which every block's
// lag o_b + delta stays inside the window, so block b reads its count row at lag index t + (o_b - o_min).  Path curve
// p_i(delta): ov / n11 / n1x / nx1 of every block at its lag (split_score's, absent samples absent) summed over the
// segment in uint32 -- order-free -- then ONE split_mix expression, or exactly 0.0 where the overlap is empty.  Moments
// and peaks over the n shifts follow k_quality_peaks (quality_curve_moments / quality_curve_peaks); peaks are reported as
// shifts, 0 being the path itself.  At max_step = 0 a segment is a piece and its record equals ffs_split_report.h's.
//
// Three kernels after k_drift_dp (the counts and prefix popcounts are still in the workspace); segments are reported
// DRIFT_ROUND_SEGMENTS per pair and round, so the workspace is that many fp64 rows per pair whatever the segment count:
//   k_drift_segments        one workgroup per pair: numbers the segments with a workgroup scan over the jump flags (wave
//                           ballots), writes each segment's block / sample range and first / last offset, zeroes the
//                           records past the last segment, stores the count; then one wave per segment reduces o_min /
//                           o_max over its blocks.
//   k_drift_path_sums       one workgroup per (pair, segment slot of the round, tile of 1024 shifts): a thread owns four
//                           shifts 256 apart and walks the segment's blocks in order -- the block's offset is
//                           wave-uniform, its count a 2-byte load contiguous across the wave, ov / n1x are per-block
//                           constants and nx1 one prefix difference while the block's partners all lie inside the
//                           reference -- into sixteen uint32 accumulators; one split_mix and one fp64 store per shift.
//   k_drift_segment_report  one 1024-thread workgroup per (pair, segment slot): moments and peaks over the stored row,
//                           own / prev / next read from it, and the flat maximum: the waves share the segment's blocks,
//                           lanes take the lags of [o_min, o_max] (1024 at a time, summed in LDS), then one
//                           split_piece_score per lag and a block argmax with the largest lag on ties.
#pragma once
#include "ffs_drift.h"
#include "ffs_quality.h"
#include "ffs_split_report.h"

namespace ffsa {

constexpr int DRIFT_ROUND_SEGMENTS = 8;          // segments reported per pair and round
constexpr int DRIFT_SEG_THREADS = 1024;          // k_drift_segments workgroup (one per pair)
constexpr int DRIFT_SUM_THREADS = 256;           // k_drift_path_sums workgroup
constexpr int DRIFT_SUM_SPT = 4;                 // shifts per thread
constexpr int DRIFT_SUM_TILE = DRIFT_SUM_THREADS * DRIFT_SUM_SPT;  // shifts per workgroup
constexpr int DRIFT_FLAT_CHUNK = 1024;           // lags of [o_min, o_max] summed in LDS at a time
constexpr int32_t SEGMENT_OWN_NOT_PEAK = 4;      // FFS_SEGMENT_OWN_NOT_PEAK

struct SegmentReport {  // = ffs_segment_report
    int64_t first_block, end_block;
    int64_t start_sample, end_sample;
    int64_t first_offset, last_offset, min_offset, max_offset;
    double own_score, prev_score, next_score, flat_score;
    int64_t flat_offset;
    double mean, std;
    int64_t n_lags;
    double peak_score[QUAL_MAX_PEAKS];
    int64_t peak_shift[QUAL_MAX_PEAKS];
    int32_t n_peaks, flags;
};
static_assert(sizeof(SegmentReport) == 264, "SegmentReport must match ffs_segment_report");

// segment table of one pair per workgroup: records [0, n) get their block / sample range and offsets, [n, out_stride) zero
__global__ void __launch_bounds__(DRIFT_SEG_THREADS) k_drift_segments(const SplitDesc* __restrict__ desc, int K,
                                                                     int64_t out_stride,
                                                                     const int32_t* __restrict__ block_offset,
                                                                     const uint8_t* __restrict__ block_jump,
                                                                     SegmentReport* __restrict__ report,
                                                                     int32_t* __restrict__ n_segments_out) {
    constexpr int NW = DRIFT_SEG_THREADS / 64;
    __shared__ int s_cnt[NW];
    const SplitDesc d = desc[blockIdx.x];
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint8_t* jump = block_jump + d.out_row * out_stride;
    SegmentReport* rec = report + d.out_row * out_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;  // segments that start before this chunk of blocks
    for (int64_t b0 = 0; b0 < B; b0 += DRIFT_SEG_THREADS) {
        const int64_t b = b0 + t;
        const bool in = b < B;
        const bool start = in && (b == 0 || jump[b] != 0);
        const bool last = in && (b == B - 1 || jump[b + 1] != 0);
        const unsigned long long m = __ballot(start);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = carry, chunk = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            chunk += s_cnt[w];
        }
        // segment of block b: the starts at or before it, minus one
        const int idx = before + __popcll(m & ((2ull << lane) - 1ull)) - 1;
        if (start) {
            rec[idx].first_block = b;
            rec[idx].start_sample = b * K;
            rec[idx].first_offset = o[b];
        }
        if (last) {
            rec[idx].end_block = b + 1;
            rec[idx].end_sample = (b + 1) * K < d.S ? (b + 1) * K : d.S;
            rec[idx].last_offset = o[b];
        }
        carry += chunk;
        __syncthreads();  // before the next chunk rewrites s_cnt
    }
    unsigned long long* words = (unsigned long long*)rec;
    constexpr int RW = (int)(sizeof(SegmentReport) / 8);
    for (int64_t q = (int64_t)carry * RW + t; q < out_stride * RW; q += DRIFT_SEG_THREADS) words[q] = 0ull;
    if (t == 0) n_segments_out[d.out_row] = carry;
    __threadfence_block();  // the block ranges written above are read by other waves below
    __syncthreads();
    for (int i = wave; i < carry; i += NW) {
        const int64_t f = rec[i].first_block, e = rec[i].end_block;
        int32_t mn = INT32_MAX, mx = INT32_MIN;
        for (int64_t b = f + lane; b < e; b += 64) {
            const int32_t v = o[b];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const int32_t on = __shfl_xor(mn, s, 64), ox = __shfl_xor(mx, s, 64);
            mn = on < mn ? on : mn;
            mx = ox > mx ? ox : mx;
        }
        if (lane == 0) {
            rec[i].min_offset = mn;
            rec[i].max_offset = mx;
        }
    }
}

// p_i at the shift indices t0 + 256 k (k < 4) of one 1024-shift tile; grid.x = pairs * DRIFT_ROUND_SEGMENTS * n_tiles.
// rows: [slot][DRIFT_ROUND_SEGMENTS][row_stride] fp64
__global__ void __launch_bounds__(DRIFT_SUM_THREADS) k_drift_path_sums(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                                       double* __restrict__ rows, int64_t row_stride, int K,
                                                                       int64_t W, int n_tiles, int first_segment,
                                                                       int64_t out_stride,
                                                                       const int32_t* __restrict__ block_offset,
                                                                       const int32_t* __restrict__ n_segments,
                                                                       const SegmentReport* __restrict__ report) {
    const int tile = blockIdx.x % n_tiles;
    const int g = (blockIdx.x / n_tiles) % DRIFT_ROUND_SEGMENTS;
    const int slot = blockIdx.x / (n_tiles * DRIFT_ROUND_SEGMENTS);
    const SplitDesc d = desc[slot];
    const int i = first_segment + g;
    if (i >= n_segments[d.out_row]) return;  // (uniform)
    const SegmentReport* rec = report + d.out_row * out_stride + i;
    const int64_t fb = rec->first_block, eb = rec->end_block, o_min = rec->min_offset;
    const int64_t n = 2 * W - (rec->max_offset - o_min);  // shifts
    const int64_t t0 = (int64_t)tile * DRIFT_SUM_TILE + threadIdx.x;
    if ((int64_t)tile * DRIFT_SUM_TILE >= n) return;  // (uniform)
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint16_t* counts = ws.counts + slot * ws.counts_slot;
    uint32_t ov[DRIFT_SUM_SPT], n11[DRIFT_SUM_SPT], n1x[DRIFT_SUM_SPT], nx1[DRIFT_SUM_SPT];
#pragma unroll
    for (int k = 0; k < DRIFT_SUM_SPT; ++k) ov[k] = n11[k] = n1x[k] = nx1[k] = 0u;
    for (int64_t b = fb; b < eb; ++b) {
        const int64_t sh = o[b] - o_min;  // (uniform) 0 <= sh <= o_max - o_min, so t + sh < 2W for every t < n
        const uint16_t* crow = counts + b * ws.counts_row + sh;
        const int64_t blo = b * K, bhi = (blo + K < d.S) ? blo + K : d.S;
        const uint32_t full1x = (uint32_t)(split_prefix_at(d.pre_s, d.s, bhi) - split_prefix_at(d.pre_s, d.s, blo));
#pragma unroll
        for (int k = 0; k < DRIFT_SUM_SPT; ++k) {
            const int64_t t = t0 + DRIFT_SUM_THREADS * k;
            if (t >= n) continue;
            const int64_t lag = t + sh - (W - 1);
            const int64_t a = blo > -lag ? blo : -lag;
            const int64_t e = bhi < d.R - lag ? bhi : d.R - lag;
            if (e <= a) continue;
            ov[k] += (uint32_t)(e - a);
            n11[k] += crow[t];
            n1x[k] += (a == blo && e == bhi)
                          ? full1x
                          : (uint32_t)(split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a));
            nx1[k] += (uint32_t)(split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag));
        }
    }
    double* out = rows + ((int64_t)slot * DRIFT_ROUND_SEGMENTS + g) * row_stride;
#pragma unroll
    for (int k = 0; k < DRIFT_SUM_SPT; ++k) {
        const int64_t t = t0 + DRIFT_SUM_THREADS * k;
        if (t < n) out[t] = ov[k] ? split_mix(d, ov[k], n11[k], n1x[k], nx1[k]) : 0.0;
    }
}

// one workgroup per (pair, segment slot): the segment's moments, peaks, own / neighbour scores and flat maximum;
// grid.x = pairs * DRIFT_ROUND_SEGMENTS
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_drift_segment_report(const SplitDesc* __restrict__ desc, SplitWs ws,
                                                                            const double* __restrict__ rows,
                                                                            int64_t row_stride, int64_t W,
                                                                            int first_segment, int64_t out_stride, int top_k,
                                                                            int64_t exclusion,
                                                                            const int32_t* __restrict__ n_segments,
                                                                            SegmentReport* __restrict__ report) {
    static_assert(DRIFT_FLAT_CHUNK == QUAL_PEAK_THREADS, "one lag of a chunk per thread");
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    __shared__ int64_t s_fpeak[1];
    __shared__ double s_fscore[1];
    __shared__ uint32_t s_sum[DRIFT_FLAT_CHUNK];
    const int g = blockIdx.x % DRIFT_ROUND_SEGMENTS;
    const int slot = blockIdx.x / DRIFT_ROUND_SEGMENTS;
    const SplitDesc d = desc[slot];
    const int n_seg = n_segments[d.out_row];
    const int i = first_segment + g;
    if (i >= n_seg) return;  // (uniform)
    SegmentReport* pr = report + d.out_row * out_stride;
    const int64_t fb = pr[i].first_block, eb = pr[i].end_block, lo = pr[i].start_sample, hi = pr[i].end_sample;
    const int64_t o_min = pr[i].min_offset, o_max = pr[i].max_offset;
    const int64_t n = 2 * W - (o_max - o_min);
    const int64_t shift_lo = -W + 1 - o_min;  // the shift of index 0
    const double* row = rows + ((int64_t)slot * DRIFT_ROUND_SEGMENTS + g) * row_stride;
    auto score = [&](int64_t t) { return row[t]; };
    double mean, sd;
    bool flat;
    quality_curve_moments(n, score, score, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(n, score, top_k, exclusion, s_peak, s_pscore);
    // the best constant lag of [o_min, o_max] over the segment's samples: uint32 sums of the block counts, 1024 lags at a
    // time (wave w takes blocks fb + w, fb + w + 16, ...; a lane takes lags 64 apart), then split_piece_score per lag
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    constexpr int NW = QUAL_PEAK_THREADS / 64;
    const uint16_t* counts = ws.counts + slot * ws.counts_slot;
    double fbest = -INFINITY;
    int64_t flag = 0;
    for (int64_t c0 = o_min; c0 <= o_max; c0 += DRIFT_FLAT_CHUNK) {
        const int64_t nc = o_max - c0 + 1 < DRIFT_FLAT_CHUNK ? o_max - c0 + 1 : DRIFT_FLAT_CHUNK;
        s_sum[t] = 0u;
        __syncthreads();
        const uint16_t* cbase = counts + (c0 + W - 1);  // lag index of c0
        for (int64_t b = fb + wave; b < eb; b += NW)
            for (int64_t l = lane; l < nc; l += 64) atomicAdd(&s_sum[l], (uint32_t)cbase[b * ws.counts_row + l]);
        __syncthreads();
        const int got = quality_curve_peaks(
            nc, [&](int64_t l) { return split_piece_score(d, lo, hi, s_sum[l], c0 + l); }, 1, 1, s_fpeak, s_fscore);
        if (got && s_fscore[0] >= fbest) {  // (uniform) a later chunk holds larger lags: ties go to it
            fbest = s_fscore[0];
            flag = c0 + s_fpeak[0];
        }
        __syncthreads();  // before the next chunk rewrites s_sum / s_fpeak
    }
    if (t == 0) {
        SegmentReport* rec = pr + i;
        auto at = [&](int64_t shift) {
            const int64_t q = shift - shift_lo;
            return q >= 0 && q < n ? row[q] : __builtin_nan("");
        };
        rec->own_score = at(0);
        rec->prev_score = i > 0 ? at(pr[i - 1].last_offset - pr[i].first_offset) : __builtin_nan("");
        rec->next_score = i + 1 < n_seg ? at(pr[i + 1].first_offset - pr[i].last_offset) : __builtin_nan("");
        rec->flat_score = fbest;
        rec->flat_offset = flag;
        for (int k = 0; k < QUAL_MAX_PEAKS; ++k) {
            rec->peak_score[k] = k < n_peaks ? s_pscore[k] : 0.0;
            rec->peak_shift[k] = k < n_peaks ? s_peak[k] + shift_lo : 0;
        }
        rec->mean = mean;
        rec->std = sd;
        rec->n_lags = n;
        rec->n_peaks = n_peaks;
        rec->flags = (flat ? QUAL_FLAT : 0) | (n_peaks == 0 || s_peak[0] + shift_lo != 0 ? SEGMENT_OWN_NOT_PEAK : 0);
    }
}

}  // namespace ffsa
