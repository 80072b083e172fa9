// Stand-alone check of csrc/ffs_drift_range_sched.h (no HIP, no GPU): builds the segment and work-item tables of the
// segment path report for hostile shapes and asserts what k_range_path_counts relies on.  tests/
// test_drift_range_report_host.py compiles it with the host compiler under -fsanitize=address,undefined and runs it.
//
// Shapes: the block lengths of the range groups (256, 288, 800, 1024, 2080, 32768: 1024-word blocks, more than one item
// per run), tails of 1 to 33 samples, one block, more than 1024 blocks with jumps at 1023 / 1024 / 1025, more than eight
// segments, a step every block (8-word items), one-lag ranges, asymmetric ranges, hand-made flags where the offset does
// not change and in adjacent blocks.
//
// Per case: segments tile the blocks; for every segment the path items tile its words exactly once, each inside one run
// of equal offsets of that segment, 1 <= nw <= 512; the flat items tile its words exactly once; for every item
// 0 <= lag0 - lag_lo and lag0 - lag_lo + n <= L, n >= 1, and its cells [col, col + n) lie inside the row of L + 1
// cells with the path cells [0, n_lags) and the flat cells [n_lags, L + 1) disjoint; the item count stays within
// range_path_item_cap.
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "../ffsubsync_amd/csrc/ffs_drift_range_sched.h"

using namespace ffsa;

static int g_cases = 0;
static long long g_items = 0;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            fprintf(stderr, "%s:%d: case %d: check failed: %s\n", __FILE__, __LINE__, g_cases, #cond); \
            exit(1);                                                                                 \
        }                                                                                            \
    } while (0)

static void check_case(int64_t K, int64_t S, int64_t lag_lo, int64_t lag_hi, const std::vector<int32_t>& o,
                       const std::vector<uint8_t>& jump) {
    ++g_cases;
    const int64_t B = (S + K - 1) / K, L = lag_hi - lag_lo + 1;
    CHECK((int64_t)o.size() == B && (int64_t)jump.size() == B && K % 32 == 0 && L >= 1);
    std::vector<RangePathSegment> segs;
    range_path_segments(o.data(), jump.data(), B, segs);
    CHECK(!segs.empty() && segs.front().first_block == 0 && segs.back().end_block == B);
    int64_t total = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const RangePathSegment& sg = segs[i];
        CHECK(sg.first_block < sg.end_block);
        CHECK(i == 0 || sg.first_block == segs[i - 1].end_block);
        CHECK(i == 0 || jump[(size_t)sg.first_block] != 0);
        for (int64_t b = sg.first_block; b < sg.end_block; ++b) {
            CHECK(b == sg.first_block || jump[(size_t)b] == 0);
            CHECK(sg.o_min <= o[(size_t)b] && o[(size_t)b] <= sg.o_max);
        }
        CHECK(lag_lo <= sg.o_min && sg.o_max <= lag_hi);
        const int64_t spread = sg.o_max - sg.o_min, n_lags = L - spread;
        CHECK(n_lags >= 1);
        const int32_t row = (int32_t)(3 * RPATH_ROUND_SEGMENTS + (int)(i % RPATH_ROUND_SEGMENTS));
        std::vector<RangePathItem> items;
        range_path_items(o.data(), sg, K, S, lag_lo, L, row, items);
        total += (int64_t)items.size();
        const int64_t w0 = sg.first_block * K / 32, w1 = (std::min(sg.end_block * K, S) + 31) / 32;
        std::vector<uint8_t> path_seen((size_t)(w1 - w0), 0), flat_seen((size_t)(w1 - w0), 0);
        for (const RangePathItem& it : items) {
            CHECK(it.row == row && it.nw >= 1 && it.nw <= RPATH_CHUNK_WORDS && it.n >= 1);
            CHECK(it.g0 >= w0 && it.g0 + it.nw <= w1);  // inside its segment
            CHECK((int64_t)it.lag0 - lag_lo >= 0 && (int64_t)it.lag0 - lag_lo + it.n <= L);
            CHECK(it.col >= 0 && (int64_t)it.col + it.n <= L + 1);
            // n_lags >= 1, so only path items start at cell 0: all their words inside blocks of ONE offset
            if (it.col == 0) {
                CHECK(it.n == n_lags);
                const int64_t b_first = it.g0 * 32 / K, b_last = ((it.g0 + it.nw) * 32 - 1) / K;
                for (int64_t b = b_first; b <= b_last; ++b) {
                    CHECK(b >= sg.first_block && b < sg.end_block && o[(size_t)b] == o[(size_t)b_first]);
                }
                CHECK(it.lag0 == lag_lo + (o[(size_t)b_first] - sg.o_min));
                for (int w = 0; w < it.nw; ++w) CHECK(path_seen[(size_t)(it.g0 - w0 + w)]++ == 0);
            } else {
                CHECK(it.col == n_lags && it.n == spread + 1 && it.lag0 == sg.o_min);
                for (int w = 0; w < it.nw; ++w) CHECK(flat_seen[(size_t)(it.g0 - w0 + w)]++ == 0);
            }
        }
        for (size_t w = 0; w < path_seen.size(); ++w) CHECK(path_seen[w] == 1 && flat_seen[w] == 1);
    }
    CHECK(total <= range_path_item_cap(S, B));
    g_items += total;
}

// a random path: a jump with probability p_jump per block, else a step of up to max_step with probability p_step
static void random_case(std::mt19937& rng, int64_t K, int64_t S, int64_t lag_lo, int64_t lag_hi, double p_jump,
                        double p_step, int max_step) {
    const int64_t B = (S + K - 1) / K;
    std::vector<int32_t> o((size_t)B);
    std::vector<uint8_t> jump((size_t)B, 0);
    std::uniform_int_distribution<int64_t> any(lag_lo, lag_hi);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::uniform_int_distribution<int> st(-max_step, max_step);
    int64_t cur = any(rng);
    for (int64_t b = 0; b < B; ++b) {
        if (b > 0 && u(rng) < p_jump) {
            jump[(size_t)b] = 1;
            cur = any(rng);
        } else if (b > 0 && max_step > 0 && u(rng) < p_step) {
            cur = std::min(lag_hi, std::max(lag_lo, cur + st(rng)));
        }
        o[(size_t)b] = (int32_t)cur;
    }
    check_case(K, S, lag_lo, lag_hi, o, jump);
}

int main() {
    std::mt19937 rng(20240);
    const int64_t ks[] = {256, 288, 800, 1024, 2080, 32768};
    for (int64_t K : ks) {
        const int64_t tails[] = {0, 1, 31, 32, 33};
        for (int64_t tail : tails) {
            for (int64_t blocks : {1, 2, 5, 24}) {
                const int64_t S = blocks * K + tail;
                if (S == 0) continue;
                const int64_t R = S + 300;
                random_case(rng, K, S, -(S - 1), R - 1, 0.3, 0.5, 7);   // the full range
                random_case(rng, K, S, -500, 1500, 0.5, 1.0, 7);        // asymmetric, a step every block
                random_case(rng, K, S, -45, 60, 0.0, 1.0, 2);           // one segment
                random_case(rng, K, S, 37, 37, 0.4, 1.0, 7);            // a one-lag range
                random_case(rng, K, S, 1, 1, 0.0, 0.0, 0);
                random_case(rng, K, S, 910, 1400, 0.2, 0.3, 1);         // a range that may not overlap anything
                random_case(rng, K, S, -3, 4, 0.0, 1.0, 7);             // the spread can reach the whole range
            }
        }
    }
    {  // more than 1024 blocks, jumps at 1023, 1024 and 1025 and every 100 blocks
        const int64_t K = 256, S = 1030 * K + 31, B = 1031;
        std::vector<int32_t> o((size_t)B);
        std::vector<uint8_t> jump((size_t)B, 0);
        for (int64_t b = 0; b < B; ++b) {
            if (b && (b % 100 == 0 || (b >= 1023 && b <= 1025))) jump[(size_t)b] = 1;
            o[(size_t)b] = (int32_t)(-45 + (b * 7) % 106);
        }
        check_case(K, S, -45, 60, o, jump);
    }
    {  // a step every block over 160 blocks: a spread of more than 1024 lags, 8-word items
        const int64_t K = 256, S = 160 * K + 1, B = 161;
        std::vector<int32_t> o((size_t)B);
        std::vector<uint8_t> jump((size_t)B, 0);
        for (int64_t b = 0; b < B; ++b) o[(size_t)b] = (int32_t)(-600 + 7 * b);
        check_case(K, S, -999, 1000, o, jump);
        check_case(K, S, -600, -600 + 7 * 160, o, jump);  // a shift set of one shift
    }
    {  // hand-made flags: set where the offset does not change, and in two adjacent blocks
        const int64_t K = 288, S = 8 * K + 17;
        check_case(K, S, -100, 100, {25, 25, 25, 26, -40, -41, -40, -40, -40}, {0, 0, 1, 0, 1, 1, 0, 0, 0});
    }
    {  // a two-hour pair over its full range at K = 1024
        const int64_t K = 1024, S = 720000, R = 720000;
        random_case(rng, K, S, -(S - 1), R - 1, 0.005, 0.2, 2);
    }
    printf("ok: %d cases, %lld items\n", g_cases, g_items);
    return 0;
}
