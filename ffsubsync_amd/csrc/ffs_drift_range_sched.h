// ffs_drift_range_sched.h -- the host's tables for the segment path report over a lag range (ffs_drift_range_report.h):
// the segments of a pair's path, their runs of equal block offsets and the work items of k_range_path_counts.  Plain
// C++ with no HIP includes: ffsalign.hip calls it, and tests/drift_range_sched_check.cpp builds it alone under the host
// sanitizers (tests/test_drift_range_report_host.py), because an off-by-one here becomes an out-of-bounds LDS index in
// the kernel.
//
// A segment is a maximal run [f, e) of blocks with no flagged block after the first (k_drift_segments' rule), o_min /
// o_max over its block offsets, n_lags = L - (o_max - o_min) shifts.  A RUN is a maximal stretch of consecutive blocks of
// one segment that share one offset o: at shift index t every block of it sits at the lag lag_lo + t + (o - o_min), and
// the per-block sample ranges [max(bK, -d), min((b+1)K, S, R-d)) of consecutive blocks at one lag d concatenate to
// [max(f'K, -d), min(e'K, S, R-d)) (empty ones at the ends contribute nothing), so the run's ov / n11 / n1x / nx1 are the
// sums of its blocks' and the run is exact as one unit.
//
// The n11 row of a segment slot has row_len >= L + 1 uint32 cells: the path counts of the n_lags shifts at [0, n_lags),
// the constant-lag counts of the o_max - o_min + 1 lags of [o_min, o_max] behind them at [n_lags, L + 1).  An item is at
// most RPATH_CHUNK_WORDS subtitle words inside one run (path items, lag0 = lag_lo + (o - o_min), n = n_lags, col = 0) or
// inside one segment (flat items, lag0 = o_min, n = o_max - o_min + 1, col = n_lags); the kernel adds the item's n11 at
// the lags lag0 + l, l in [0, n), into cells col + l.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ffsa {

constexpr int RPATH_ROUND_SEGMENTS = 8;   // segment rows per pair and round
constexpr int RPATH_CHUNK_WORDS = 512;    // subtitle words per work item (at most)

struct RangePathItem {
    int64_t g0;    // first subtitle word of the chunk
    int32_t row;   // slot * RPATH_ROUND_SEGMENTS + the segment's place in the round
    int32_t nw;    // words in the chunk (1 .. RPATH_CHUNK_WORDS)
    int32_t lag0;  // the lag of the item's cell 0
    int32_t n;     // lags the item counts
    int32_t col;   // first cell of the row it adds to
    int32_t pad;
};
static_assert(sizeof(RangePathItem) == 32, "RangePathItem is uploaded as it is");

struct RangePathSegment {
    int64_t first_block, end_block;
    int64_t o_min, o_max;
};

// the segments of the B blocks of one pair
inline void range_path_segments(const int32_t* o, const uint8_t* jump, int64_t B, std::vector<RangePathSegment>& out) {
    out.clear();
    int64_t f = 0;
    for (int64_t b = 1; b <= B; ++b) {
        if (b < B && jump[b] == 0) continue;
        RangePathSegment sg{f, b, o[f], o[f]};
        for (int64_t q = f; q < b; ++q) {
            sg.o_min = std::min<int64_t>(sg.o_min, o[q]);
            sg.o_max = std::max<int64_t>(sg.o_max, o[q]);
        }
        out.push_back(sg);
        f = b;
    }
}

// words [w0, w1) in chunks of at most RPATH_CHUNK_WORDS
inline void range_path_chunks(int64_t w0, int64_t w1, int32_t row, int64_t lag0, int64_t n, int64_t col,
                              std::vector<RangePathItem>& out) {
    for (int64_t c = w0; c < w1; c += RPATH_CHUNK_WORDS) {
        RangePathItem it;
        it.g0 = c;
        it.row = row;
        it.nw = (int32_t)std::min<int64_t>(RPATH_CHUNK_WORDS, w1 - c);
        it.lag0 = (int32_t)lag0;
        it.n = (int32_t)n;
        it.col = (int32_t)col;
        it.pad = 0;
        out.push_back(it);
    }
}

// the work items of one segment into row `row` (appended): the path items of its runs, then its flat items.  K is a
// multiple of 32, so every block and run starts on a word; S is the subtitle length, [lag_lo, lag_lo + L) the lag set.
inline void range_path_items(const int32_t* o, const RangePathSegment& sg, int64_t K, int64_t S, int64_t lag_lo, int64_t L,
                             int32_t row, std::vector<RangePathItem>& out) {
    const int64_t spread = sg.o_max - sg.o_min, n_lags = L - spread;
    for (int64_t b = sg.first_block; b < sg.end_block;) {
        int64_t b1 = b + 1;
        while (b1 < sg.end_block && o[b1] == o[b]) ++b1;
        const int64_t w0 = b * K / 32, w1 = (std::min(b1 * K, S) + 31) / 32;
        range_path_chunks(w0, w1, row, lag_lo + (o[b] - sg.o_min), n_lags, 0, out);
        b = b1;
    }
    const int64_t w0 = sg.first_block * K / 32, w1 = (std::min(sg.end_block * K, S) + 31) / 32;
    range_path_chunks(w0, w1, row, sg.o_min, spread + 1, n_lags, out);
}

// an upper bound of one pair's items over all its rounds: every run and every segment ends in at most one short chunk
inline int64_t range_path_item_cap(int64_t max_samples, int64_t max_blocks) {
    return 2 * (((max_samples + 31) / 32 + RPATH_CHUNK_WORDS - 1) / RPATH_CHUNK_WORDS + max_blocks);
}

}  // namespace ffsa
