// ffs_drift_range_smooth.h -- ffs_drift_smooth.h's knot fit behind the lag-range drift solve of ffs_drift_range.h
// (gfx950).  The fit is that header's word for word -- segments, knot blocks, digital lines, uint32 sums scored once by
// split_mix, the bend cost, the Viterbi pass and its tie rule -- with ONE change: a knot candidate c_i = o_{k_i} + u is
// valid where lag_lo <= c_i <= lag_hi (the pair's range) instead of -W + 1 <= c_i <= W.  Block terms are the range
// path's (range_score's a, e, prefixes, absent samples; lags without overlap contribute nothing).  Pinned against the
// numpy model tests/drift_range_smooth_model.py.
//
// k_drift_line_sums reads the uint16 table counts[block][lag] of the windowed plan; the range solve never stores one
// (704 x 1.44 M cells at 2 h over the full range).  The fit needs n11 only near the path: for interval i with knots at
// o0 = o[k], o1 = o[k + n], every line between two candidates stays inside [min(o0, o1) - R, max(o0, o1) + R], and
// inside a segment |o1 - o0| <= n max_step with n <= ceil(3M / 2), so a row of
//     range_band_row = max_step * ceil(3M / 2) + 2R + 1   cells per block
// (81 at max_step 2, M = 16, R = 16; 2721 at 7, 256, 16) holds every count the interval's lines can ask for.
//
// The steps after k_range_scores (the offsets are lags by then), in the same sub-batch, nothing read back:
//   k_smooth_intervals   (ffs_drift_smooth.h, unchanged) segment and interval tables, knot flags, the path as the initial
//                        smooth offsets.
//   k_range_band_counts  one workgroup per block and pair: the block's K/32 subtitle words and the reference words its
//                        band can meet staged in LDS (words outside [0, R) read as zero through split_word), a thread
//                        owns the band lags t, t + 256, ...: n11 by funnel shift and popcount as k_range_step, one
//                        uint16 cell per lag (n11 <= K <= 32768).  A workgroup owns its row: no atomics, no memset.
//   k_range_line_sums    k_drift_line_sums with the band lookup in place of the count table and the range test in
//                        place of the window test: the same thread-to-line mapping, the same four uint32 accumulators,
//                        one split_mix and one fp64 store per line.
//   k_drift_knot_dp      (ffs_drift_smooth.h, unchanged).
#pragma once
#include "ffs_drift_range.h"
#include "ffs_drift_smooth.h"

namespace ffsa {

constexpr int RBAND_THREADS = 256;  // k_range_band_counts workgroup (one per block and pair)

// cells of one block's band row: the longest interval has fewer than ceil(3M / 2) blocks
constexpr int range_band_row(int max_step, int M, int R) { return max_step * ((3 * M + 1) / 2) + 2 * R + 1; }
constexpr int RBAND_MAX_ROW = range_band_row(DRIFT_RANGE_MAX_STEP, SMOOTH_MAX_KNOT_BLOCKS, SMOOTH_MAX_RADIUS);  // 2721

struct RangeBand {
    uint16_t* cells;  // [slot][SmoothWs::stride blocks][row]: n11 of block b at the lags band_lo(interval of b) + x
    int64_t row;      // cells per block: this call's range_band_row
};

// the band of the interval with path lags o0, o1 at its knots: first lag and width
FFS_DEV int64_t range_band_lo(int32_t o0, int32_t o1, int R) { return (int64_t)(o0 < o1 ? o0 : o1) - R; }
FFS_DEV int64_t range_band_width(int32_t o0, int32_t o1, int R) {
    const int64_t span = (int64_t)o1 - o0;
    return (span < 0 ? -span : span) + 2 * R + 1;
}

// n11 of block blockIdx.x of pair blockIdx.y at every lag of its interval's band; grid = (max blocks, pairs)
__global__ void __launch_bounds__(RBAND_THREADS) k_range_band_counts(const SplitDesc* __restrict__ desc, SmoothWs sw,
                                                                    RangeBand band, int K, int M, int R,
                                                                    int64_t out_stride,
                                                                    const int32_t* __restrict__ block_offset) {
    __shared__ uint32_t s_sub[SPLIT_MAX_K / 32];
    __shared__ uint32_t s_ref[SPLIT_MAX_K / 32 + (RBAND_MAX_ROW + 31) / 32 + 1];
    const int slot = blockIdx.y;
    const int64_t b = blockIdx.x;
    const SplitDesc d = desc[slot];
    const int64_t B = (d.S + K - 1) / K;
    if (b >= B) return;  // (uniform)
    const SmoothSeg g = sw.seg[slot * sw.stride + sw.seg_of[slot * sw.stride + b]];
    if (g.n_int == 0) return;  // (uniform) a one-block segment has no line
    const int i = ((int)b - g.first) / M < g.n_int ? ((int)b - g.first) / M : g.n_int - 1;
    const SmoothInt v = sw.iv[slot * sw.stride + g.int_base + i];
    const int32_t* o = block_offset + d.out_row * out_stride;
    const int32_t o0 = o[v.k], o1 = o[v.k + v.n];
    const int64_t lo = range_band_lo(o0, o1, R);
    const int width = (int)range_band_width(o0, o1, R);
    if (width > band.row) return;  // (uniform) never inside a segment (|o1 - o0| <= n max_step): every store stays in the row
    const int t = threadIdx.x;
    const int kw = K >> 5;
    const int n_ref_words = kw + ((width - 1) >> 5) + 1;
    const int64_t base = b * K + lo;  // reference sample met by the block's first sample at the band's first lag
    const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
    const int bsh = (int)(base - gbase * 32);
    for (int q = t; q < n_ref_words; q += RBAND_THREADS) {
        const uint32_t wlo = split_word(d.r, d.R, gbase + q), whi = split_word(d.r, d.R, gbase + q + 1);
        s_ref[q] = __builtin_amdgcn_alignbit(whi, wlo, bsh);
    }
    for (int q = t; q < kw; q += RBAND_THREADS) s_sub[q] = split_word(d.s, d.S, b * kw + q);
    __syncthreads();
    uint16_t* row = band.cells + ((int64_t)slot * sw.stride + b) * band.row;
    for (int x = t; x < width; x += RBAND_THREADS) {  // band lag x: reference word (x >> 5) + w, shifted by x & 31
        const int q0 = x >> 5, sh = x & 31;
        uint32_t wlo = s_ref[q0], acc = 0;
        for (int w = 0; w < kw; ++w) {
            const uint32_t whi = s_ref[q0 + w + 1];
            acc += __popc(__builtin_amdgcn_alignbit(whi, wlo, sh) & s_sub[w]);  // (s_sub: one address per wave)
            wlo = whi;
        }
        row[x] = (uint16_t)acc;
    }
}

// T of every line of the intervals blockIdx.x % SMOOTH_LINE_GROUPS, + SMOOTH_LINE_GROUPS, ... of one pair, n11 from the
// band rows; grid.x = pairs * SMOOTH_LINE_GROUPS
__global__ void __launch_bounds__(SMOOTH_LINE_THREADS) k_range_line_sums(const SplitDesc* __restrict__ desc,
                                                                        const RangeLag* __restrict__ lags, SmoothWs sw,
                                                                        RangeBand band, int K, int R, int64_t out_stride,
                                                                        const int32_t* __restrict__ block_offset) {
    const int slot = blockIdx.x / SMOOTH_LINE_GROUPS;
    const SplitDesc d = desc[slot];
    const int64_t lag_lo = lags[slot].lag_lo, lag_hi = lag_lo + lags[slot].L - 1;
    const int n_int = sw.n_int[slot];
    const int S1 = 2 * R + 1, S2 = S1 * S1;
    const int32_t* o = block_offset + d.out_row * out_stride;
    const uint16_t* cells = band.cells + (int64_t)slot * sw.stride * band.row;
    const SmoothInt* ivs = sw.iv + slot * sw.stride;
    for (int q = blockIdx.x % SMOOTH_LINE_GROUPS; q < n_int; q += SMOOTH_LINE_GROUPS) {  // (uniform)
        const SmoothInt v = ivs[q];
        const int nb = v.n + v.last;  // blocks of the interval
        const int32_t o0 = o[v.k], o1 = o[v.k + v.n];
        const int64_t lo = range_band_lo(o0, o1, R);
        const bool held = range_band_width(o0, o1, R) <= band.row;  // (uniform) always, as in k_range_band_counts
        double* out = sw.T + ((int64_t)slot * sw.stride + q) * S2;
        for (int line = threadIdx.x; line < S2; line += SMOOTH_LINE_THREADS) {
            const int64_t c0 = (int64_t)o0 + line / S1 - R, c1 = (int64_t)o1 + line % S1 - R;
            if (!held || c0 < lag_lo || c0 > lag_hi || c1 < lag_lo || c1 > lag_hi) {
                out[line] = -INFINITY;
                continue;
            }
            const int32_t two_d = 2 * (int32_t)(c1 - c0), two_n = 2 * v.n;
            uint32_t ov = 0u, n11 = 0u, n1x = 0u, nx1 = 0u;
            for (int j = 0; j < nb; ++j) {
                const int64_t b = v.k + j;
                const int64_t lag = c0 + smooth_floor_div(two_d * j + v.n, two_n);  // between c0 and c1: inside the band
                const int64_t blo = b * K, bhi = (blo + K < d.S) ? blo + K : d.S;
                const int64_t a = blo > -lag ? blo : -lag;
                const int64_t e = bhi < d.R - lag ? bhi : d.R - lag;
                if (e <= a) continue;
                ov += (uint32_t)(e - a);
                n11 += cells[b * band.row + (lag - lo)];
                n1x += (uint32_t)(split_prefix_at(d.pre_s, d.s, e) - split_prefix_at(d.pre_s, d.s, a));
                nx1 += (uint32_t)(split_prefix_at(d.pre_r, d.r, e + lag) - split_prefix_at(d.pre_r, d.r, a + lag));
            }
            out[line] = ov ? split_mix(d, ov, n11, n1x, nx1) : 0.0;
        }
    }
}

}  // namespace ffsa
