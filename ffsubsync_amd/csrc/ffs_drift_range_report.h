// ffs_drift_range_report.h -- per-segment path report of a drift solve over any lag range [lag_lo, lag_hi], up to the full
// overlap range (gfx950).  The contract is ffs_drift_report.h's with the lag set d = lag_lo + j, j in [0, L),
// L = lag_hi - lag_lo + 1: shift set delta in [lag_lo - o_min, lag_hi - o_max] (n_lags = L - (o_max - o_min) shifts, shift
// index t puts block b at the lag lag_lo + t + (o_b - o_min)), ov / n11 / n1x / nx1 of every block at its lag summed over
// the segment as exact integers, ONE split_mix expression per shift (exactly 0.0 where the summed overlap is empty),
// quality_curve_moments / quality_curve_peaks over the shifts, own / prev / next from the curve, and the flat maximum
// over the constant lags [o_min, o_max] (split_piece_score, the largest lag on ties).  At [-W+1, W] the records are
// bit-identical to k_drift_segment_report's, at max_step = 0 to k_cut_piece_report's in the shared fields.  Pinned against
// the numpy model tests/drift_range_report_model.py and the independent reference tests/report_reference.py.
//
// The range drift solve stores no block counts (3.14), so this is a post-pass over a finished path that counts n11 from
// the bits, for the segments of one round at a time (RPATH_ROUND_SEGMENTS slots per pair: the row workspace does not
// depend on the segment count).  Per slot one uint32 row of L + 1 cells (the n_lags path counts, then the
// o_max - o_min + 1 constant-lag counts: together exactly L + 1) and one fp64 row of the n_lags path scores.
//   k_drift_segments       (ffs_drift_report.h) the segment table into the caller's records, unchanged.
//   k_range_path_counts    k_cut_piece_counts' scheme with a lag origin per work item: one item (at most
//                          RPATH_CHUNK_WORDS subtitle words inside one RUN of equal-offset blocks of a segment, or
//                          inside the segment for the flat cells) x one 4096-lag tile per workgroup -- the chunk and the
//                          reference window it meets staged in LDS, thread q holds the 32 lags 32q..32q+31 of the tile
//                          (v_alignbit + v_bcnt), an LDS transpose, integer atomicAdd into the row (exact, order-free).
//                          A run is exact as one unit: the per-block sample ranges of consecutive blocks at one lag
//                          concatenate (ffs_drift_range_sched.h, which builds the items on the host).
//   k_range_path_scores    one workgroup per (pair, segment slot, tile of 1024 shifts): a thread owns four shifts 256
//                          apart and walks the segment's runs -- ov and n1x are per-run constants and nx1 one prefix
//                          difference while every partner lies inside the reference -- then reads n11 from the row and
//                          stores one split_mix per shift.
//   k_range_segment_report k_drift_segment_report over those rows with shift_lo = lag_lo - o_min; the flat maximum is
//                          one block argmax of split_piece_score over the flat cells (largest lag on ties).
#pragma once
#include "ffs_cut_report.h"
#include "ffs_drift_range_sched.h"
#include "ffs_drift_report.h"

namespace ffsa {

constexpr int RPATH_MAX_ITEMS = 65535;  // work items per k_range_path_counts launch (grid.y)
static_assert(RPATH_ROUND_SEGMENTS == DRIFT_ROUND_SEGMENTS, "the rounds follow ffs_drift_report.h's");

// n11 of one item over one 4096-lag tile of its n lags; grid = (tiles, items of this launch)
__global__ void __launch_bounds__(QUAL_CNT_THREADS) k_range_path_counts(const SplitDesc* __restrict__ desc,
                                                                        const RangePathItem* __restrict__ items,
                                                                        uint32_t* __restrict__ rows, int64_t row_stride) {
    __shared__ uint32_t s_sub[RPATH_CHUNK_WORDS];
    __shared__ uint32_t s_ref[RPATH_CHUNK_WORDS + QUAL_CNT_THREADS + 1];
    __shared__ uint32_t s_acc[QUAL_CNT_THREADS * 33];  // [q][sh], rows padded to 33 words against bank conflicts
    const RangePathItem it = items[blockIdx.y];
    const SplitDesc d = desc[it.row / RPATH_ROUND_SEGMENTS];
    const int64_t l0 = (int64_t)blockIdx.x * QUAL_TILE;  // first lag index of the tile, relative to the item's lag0
    if (l0 >= it.n) return;                              // (uniform)
    const int nw = it.nw;
    // reference bits [base + 32 q, +32) for q <= nw + QUAL_CNT_THREADS meet subtitle word g0 + w at tile lag 32 q' + sh
    const int64_t base = 32 * it.g0 + it.lag0 + l0;
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
    uint32_t* out = rows + (int64_t)it.row * row_stride + it.col + l0;
    const int64_t n_here = it.n - l0 < QUAL_TILE ? it.n - l0 : QUAL_TILE;
    for (int l = t; l < n_here; l += QUAL_CNT_THREADS) {
        const uint32_t v = s_acc[(l >> 5) * 33 + (l & 31)];
        if (v) atomicAdd(out + l, v);
    }
}

// p_i at the shift indices t0 + 256 k (k < 4) of one 1024-shift tile; grid.x = pairs * RPATH_ROUND_SEGMENTS * n_tiles.
// rows: [slot][RPATH_ROUND_SEGMENTS][row_stride] uint32 (the path counts in cells [0, n)); scores: the same shape, fp64
__global__ void __launch_bounds__(DRIFT_SUM_THREADS) k_range_path_scores(const SplitDesc* __restrict__ desc,
                                                                         const RangeLag* __restrict__ lags,
                                                                         const uint32_t* __restrict__ rows,
                                                                         double* __restrict__ scores, int64_t row_stride,
                                                                         int K, int n_tiles, int first_segment,
                                                                         int64_t out_stride,
                                                                         const int32_t* __restrict__ block_offset,
                                                                         const int32_t* __restrict__ n_segments,
                                                                         const SegmentReport* __restrict__ report) {
    const int tile = blockIdx.x % n_tiles;
    const int g = (blockIdx.x / n_tiles) % RPATH_ROUND_SEGMENTS;
    const int slot = blockIdx.x / (n_tiles * RPATH_ROUND_SEGMENTS);
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int i = first_segment + g;
    if (i >= n_segments[d.out_row]) return;  // (uniform)
    const SegmentReport* rec = report + d.out_row * out_stride + i;
    const int64_t fb = rec->first_block, eb = rec->end_block, o_min = rec->min_offset;
    const int64_t n = lg.L - (rec->max_offset - o_min);  // shifts
    const int64_t t0 = (int64_t)tile * DRIFT_SUM_TILE + threadIdx.x;
    if ((int64_t)tile * DRIFT_SUM_TILE >= n) return;  // (uniform)
    const int32_t* o = block_offset + d.out_row * out_stride;
    uint32_t ov[DRIFT_SUM_SPT], n1x[DRIFT_SUM_SPT], nx1[DRIFT_SUM_SPT];
#pragma unroll
    for (int k = 0; k < DRIFT_SUM_SPT; ++k) ov[k] = n1x[k] = nx1[k] = 0u;
    for (int64_t b = fb; b < eb;) {
        const int32_t ob = o[b];
        int64_t b1 = b + 1;
        while (b1 < eb && o[b1] == ob) ++b1;  // (uniform) the run [b, b1) of one offset
        // lag of shift t: 0 <= sh <= o_max - o_min, so lag_lo <= lag <= lag_hi for every t < n
        const int64_t lag_first = lg.lag_lo + (ob - o_min);
        const int64_t rlo = b * K, rhi = (b1 * K < d.S) ? b1 * K : d.S;
        const uint32_t full1x = (uint32_t)(split_prefix_at(d.pre_s, d.s, rhi) - split_prefix_at(d.pre_s, d.s, rlo));
#pragma unroll
        for (int k = 0; k < DRIFT_SUM_SPT; ++k) {
            const int64_t t = t0 + DRIFT_SUM_THREADS * k;
            if (t >= n) continue;
            const int64_t lag = lag_first + t;
            const int64_t a = rlo > -lag ? rlo : -lag;
            const int64_t e = rhi < d.R - lag ? rhi : d.R - lag;
            if (e <= a) continue;
            ov[k] += (uint32_t)(e - a);
            n1x[k] += (a == rlo && e == rhi)
                          ? full1x
                          : (uint32_t)(split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a));
            nx1[k] += (uint32_t)(split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag));
        }
        b = b1;
    }
    const int64_t row0 = ((int64_t)slot * RPATH_ROUND_SEGMENTS + g) * row_stride;
    const uint32_t* cnt = rows + row0;
    double* out = scores + row0;
#pragma unroll
    for (int k = 0; k < DRIFT_SUM_SPT; ++k) {
        const int64_t t = t0 + DRIFT_SUM_THREADS * k;
        if (t < n) out[t] = ov[k] ? split_mix(d, ov[k], cnt[t], n1x[k], nx1[k]) : 0.0;
    }
}

// one workgroup per (pair, segment slot): the segment's moments, peaks, own / neighbour scores and flat maximum;
// grid.x = pairs * RPATH_ROUND_SEGMENTS
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_range_segment_report(const SplitDesc* __restrict__ desc,
                                                                            const RangeLag* __restrict__ lags,
                                                                            const uint32_t* __restrict__ rows,
                                                                            const double* __restrict__ scores,
                                                                            int64_t row_stride, int first_segment,
                                                                            int64_t out_stride, int top_k, int64_t exclusion,
                                                                            const int32_t* __restrict__ n_segments,
                                                                            SegmentReport* __restrict__ report) {
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    __shared__ int64_t s_fpeak[1];
    __shared__ double s_fscore[1];
    const int g = blockIdx.x % RPATH_ROUND_SEGMENTS;
    const int slot = blockIdx.x / RPATH_ROUND_SEGMENTS;
    const SplitDesc d = desc[slot];
    const RangeLag lg = lags[slot];
    const int n_seg = n_segments[d.out_row];
    const int i = first_segment + g;
    if (i >= n_seg) return;  // (uniform)
    SegmentReport* pr = report + d.out_row * out_stride;
    const int64_t lo = pr[i].start_sample, hi = pr[i].end_sample;
    const int64_t o_min = pr[i].min_offset, o_max = pr[i].max_offset;
    const int64_t n = lg.L - (o_max - o_min);
    const int64_t shift_lo = lg.lag_lo - o_min;  // the shift of index 0
    const double* row = scores + (int64_t)blockIdx.x * row_stride;
    const uint32_t* flat_cnt = rows + (int64_t)blockIdx.x * row_stride + n;  // the lags o_min .. o_max
    auto score = [&](int64_t t) { return row[t]; };
    double mean, sd;
    bool flat;
    quality_curve_moments(n, score, score, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(n, score, top_k, exclusion, s_peak, s_pscore);
    // the best constant lag of [o_min, o_max] over the segment's samples (at least one lag: always one peak)
    quality_curve_peaks(
        o_max - o_min + 1, [&](int64_t l) { return split_piece_score(d, lo, hi, flat_cnt[l], o_min + l); }, 1, 1, s_fpeak,
        s_fscore);
    if (threadIdx.x == 0) {
        SegmentReport* rec = pr + i;
        auto at = [&](int64_t shift) {
            const int64_t q = shift - shift_lo;
            return q >= 0 && q < n ? row[q] : __builtin_nan("");
        };
        rec->own_score = at(0);
        rec->prev_score = i > 0 ? at(pr[i - 1].last_offset - pr[i].first_offset) : __builtin_nan("");
        rec->next_score = i + 1 < n_seg ? at(pr[i + 1].first_offset - pr[i].last_offset) : __builtin_nan("");
        rec->flat_score = s_fscore[0];
        rec->flat_offset = o_min + s_fpeak[0];
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
