// ffs_stability.h -- delete-half resamples of a boundary list and the order statistics of their solved offsets (gfx950):
// the device side of ffsubsync_amd/stability.py.
//
// "How precisely is this offset known, and would the peak that won still win on another half of the cues?" without a
// tuned score threshold: solve K subtitles that each keep a hashed half of the cue blocks, positions untouched, and look
// at the spread of the K offsets.  Contract (include/ffsubsync_amd.h, ffs_subsample_lists / ffs_offset_stats), pinned
// against tests/stability_model.py:
//   - a list of n boundaries has m = n / 2 runs, cut into nb = ceil(m / B) blocks of B consecutive runs (all of them; the
//     last block may be short)
//   - subsample s keeps block b iff ((key(seed, s >> 1, b) >> 31) ^ (s & 1)) == 1, key the surrogate's hash: subsamples
//     2j and 2j + 1 are complementary
//   - the output is the valid list of the kept runs in input order: pos copied, ones_before recomputed
//
// k_subsample_lists: one 256-thread workgroup per (vector, subsample).  The runs are walked in chunks of 64, a run a
// lane; every wave owns a contiguous quarter of the chunks.  A run's keep flag is one hash of its block index.  Count
// pass: every lane adds up (kept runs, kept ones) of its runs, packed into one 64-bit word (both stay below 2^31), a
// cross-lane sum gives the wave's total and an exclusive scan over the four totals in LDS the wave's first output slot
// and first ones_before.  Write pass: the wave walks its chunks again in order; a ballot and a popcount of the lanes
// below give a kept run its slot inside the chunk, a wave scan of the kept lengths its ones_before, and consecutive
// kept lanes store to consecutive entries (8-byte stores: a list block is only 8-byte aligned).  The input is read twice
// per subsample and K times per vector from L2.  No array grows with the list: there is no unit limit.  The vectors'
// descriptors (SurrVec, shared with k_surrogate_lists) are uploaded behind the caller's stream by the host call.
//
// k_offset_stats: one 256-thread workgroup per file over its K + 1 solve records.  The K subsample offsets are staged in
// LDS as 64-bit words -- an unusable record as INT64_MAX, so the c usable ones are the first c of the sorted order
// whatever their values -- and sorted by the bitonic network of k_surrogate_lists; the three ranks are read out of the
// sorted array.  Counts, maxima and the pair minimum are reduced across lanes, then across the four waves in LDS.
#pragma once
#include "ffs_kernels.h"
#include "ffs_surrogate.h"
#include "ffs_sweep.h"

namespace ffsa {

constexpr int STAB_THREADS = 256;
constexpr int STAB_WAVES = STAB_THREADS / 64;
constexpr int STAB_MAX_K = 4096;                 // FFS_STAB_MAX_K
constexpr int STAB_MAX_BLOCK_RUNS = 1 << 24;     // FFS_STAB_MAX_BLOCK_RUNS
constexpr int32_t SUB_BAD_ODD = SURR_BAD_ODD;              // FFS_SUB_BAD_ODD
constexpr int32_t SUB_BAD_TRUNCATED = SURR_BAD_TRUNCATED;  // FFS_SUB_BAD_TRUNCATED
constexpr int32_t SUB_BAD_BOUND = SURR_BAD_BOUND;          // FFS_SUB_BAD_BOUND
constexpr int32_t STAB_EMPTY = 1;      // FFS_STAB_EMPTY
constexpr int32_t STAB_AMBIGUOUS = 2;  // FFS_STAB_AMBIGUOUS
constexpr int32_t STAB_NO_PAIRS = 4;   // FFS_STAB_NO_PAIRS

struct StabilityResult {  // = ffs_stability_result
    double real_score;
    int64_t real_offset;
    int64_t off_min, off_max, off_median, off_lo, off_hi;
    int64_t max_dev, max_pair_gap;
    double pair_score_min;
    int32_t n_sub, n_within, n_pairs, n_pairs_within;
    int64_t tol;
    int32_t flags, reserved;
};
static_assert(sizeof(StabilityResult) == 112, "StabilityResult must match ffs_stability_result");

__global__ void __launch_bounds__(STAB_THREADS) k_subsample_lists(const SurrVec* __restrict__ vecs, int n_sub, int block_runs,
                                                                  char* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ unsigned long long s_wave[STAB_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int v = (int)(blockIdx.x / (unsigned)n_sub), s = (int)(blockIdx.x % (unsigned)n_sub);
    const SurrVec d = vecs[v];
    const int2* hdr = (const int2*)d.list;
    const int2* __restrict__ e = hdr + 2;
    const int2 h0 = hdr[0], h1 = hdr[1];
    const int n = h0.x, len = h1.x, cap = h1.y;
    int2* oh = (int2*)(out + d.out_off + (long long)s * (16 + 8 * (long long)d.cap_out));
    int2* __restrict__ oe = oh + 2;

    int32_t bad = 0;
    if (n & 1) bad |= SUB_BAD_ODD;
    if (n < 0 || n >= cap) bad |= SUB_BAD_TRUNCATED;
    if (n > d.n_bound) bad |= SUB_BAD_BOUND;
    if (s == 0 && t == 0) status[v] = bad;
    if (bad) {  // (uniform) an unusable list: every subsample is the empty list of the same length
        if (t == 0) {
            oh[0] = make_int2(0, 0);
            oh[1] = make_int2(len, d.cap_out);
            oe[0] = make_int2(INT32_MAX, 0);
        }
        return;
    }
    const int m = n >> 1;
    const unsigned B = (unsigned)block_runs;
    const uint32_t hs = surr_fmix32(d.seed + 0x9E3779B9u * (uint32_t)((s >> 1) + 1));
    const uint32_t flip = (uint32_t)(s & 1);
    const int chunks = (m + 63) >> 6, per = (chunks + STAB_WAVES - 1) / STAB_WAVES;
    const int c0 = wave * per < chunks ? wave * per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;

    // count pass: (kept runs << 32 | kept ones) of this wave's chunks
    unsigned long long mine = 0;
    for (int c = c0; c < c1; ++c) {
        const int j = (c << 6) + lane;
        if (j < m && ((surr_fmix32(hs ^ ((unsigned)j / B)) >> 31) ^ flip) == 1u)
            mine += (1ull << 32) | (unsigned)(e[2 * j + 1].x - e[2 * j].x);
    }
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int w = 0; w < STAB_WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    int slot0 = (int)(before >> 32), ones0 = (int)(unsigned)before;

    // write pass: the kept runs of a chunk go to consecutive entries behind the wave's running slot
    for (int c = c0; c < c1; ++c) {
        const int j = (c << 6) + lane;
        int2 a = make_int2(0, 0), b = make_int2(0, 0);
        bool keep = false;
        if (j < m) {
            keep = ((surr_fmix32(hs ^ ((unsigned)j / B)) >> 31) ^ flip) == 1u;
            if (keep) {
                a = e[2 * j];
                b = e[2 * j + 1];
            }
        }
        const int run = b.x - a.x;  // (0 for a lane that keeps nothing)
        const unsigned long long kept = __ballot(keep);
        int inc = run;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (keep) {
            const int q = slot0 + __popcll(kept & ((1ull << lane) - 1ull));
            const int ob = ones0 + inc - run;
            oe[2 * q] = make_int2(a.x, ob);
            oe[2 * q + 1] = make_int2(b.x, ob + run);
        }
        slot0 += __popcll(kept);
        ones0 += __shfl(inc, 63, 64);
    }
    if (t == 0) {
        const int runs = (int)(total >> 32), ones = (int)(unsigned)total;
        oh[0] = make_int2(2 * runs, ones);
        oh[1] = make_int2(len, d.cap_out);
        oe[2 * runs] = make_int2(INT32_MAX, ones);
    }
}

// a double as an unsigned word of the same order (-0.0 below +0.0), and back
FFS_DEV unsigned long long stab_order_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
FFS_DEV double stab_order_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}
FFS_DEV long long stab_abs_diff(long long a, long long b) { return a > b ? a - b : b - a; }

// File f owns records rec[f * (K + 1) ..]: record 0 the real list's solve, record 1 + s subsample s.
__global__ void __launch_bounds__(STAB_THREADS) k_offset_stats(const CandResult* __restrict__ rec, int n_sub, long long tol,
                                                               StabilityResult* __restrict__ out) {
    __shared__ long long s_off[STAB_MAX_K];
    __shared__ long long s_dev[STAB_WAVES], s_gap[STAB_WAVES];
    __shared__ unsigned long long s_low[STAB_WAVES];
    __shared__ int s_cnt[STAB_WAVES], s_in[STAB_WAVES], s_pairs[STAB_WAVES], s_pin[STAB_WAVES], s_amb[STAB_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const CandResult* r = rec + (int64_t)blockIdx.x * (n_sub + 1);
    const CandResult real = r[0];
    const bool real_ok = !sweep_skipped(real);
    const long long ro = (long long)real.offset;
    const int P = surr_pow2(n_sub);

    // the subsamples: stage the offsets, count the usable ones and those within tol, the largest deviation
    int cnt = 0, in = 0, amb = (real.flags & SWEEP_REC_AMBIGUOUS) != 0;
    long long dev = 0;
    for (int i = t; i < P; i += STAB_THREADS) {
        long long o = INT64_MAX;
        if (i < n_sub) {
            const CandResult c = r[1 + i];
            amb |= (c.flags & SWEEP_REC_AMBIGUOUS) != 0;
            if (!sweep_skipped(c)) {
                o = (long long)c.offset;
                const long long dd = stab_abs_diff(o, ro);
                ++cnt;
                in += dd <= tol;
                dev = dd > dev ? dd : dev;
            }
        }
        s_off[i] = o;
    }
    // the pairs (2j, 2j + 1) with both members usable: the largest gap, the smallest score sum
    int pairs = 0, pin = 0;
    long long gap = 0;
    unsigned long long low = ~0ull;
    for (int j = t; j < (n_sub >> 1); j += STAB_THREADS) {
        const CandResult a = r[1 + 2 * j], b = r[2 + 2 * j];
        if (sweep_skipped(a) || sweep_skipped(b)) continue;
        const long long g = stab_abs_diff((long long)a.offset, (long long)b.offset);
        const unsigned long long key = stab_order_key(a.score + b.score);
        ++pairs;
        pin += g <= tol;
        gap = g > gap ? g : gap;
        low = key < low ? key : low;
    }
    for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        in += __shfl_xor(in, o, 64);
        amb |= __shfl_xor(amb, o, 64);
        pairs += __shfl_xor(pairs, o, 64);
        pin += __shfl_xor(pin, o, 64);
        const long long od = __shfl_xor(dev, o, 64), og = __shfl_xor(gap, o, 64);
        const unsigned long long ol = __shfl_xor(low, o, 64);
        dev = od > dev ? od : dev;
        gap = og > gap ? og : gap;
        low = ol < low ? ol : low;
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_in[wave] = in;
        s_amb[wave] = amb;
        s_pairs[wave] = pairs;
        s_pin[wave] = pin;
        s_dev[wave] = dev;
        s_gap[wave] = gap;
        s_low[wave] = low;
    }
    __syncthreads();  // (publishes the staged offsets and the waves' partial results)
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += STAB_THREADS) {
                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                const long long x = s_off[a], y = s_off[b];
                if ((x > y) == ((a & k) == 0)) {
                    s_off[a] = y;
                    s_off[b] = x;
                }
            }
            __syncthreads();
        }
    }
    if (t == 0) {
        cnt = in = amb = pairs = pin = 0;
        dev = gap = 0;
        low = ~0ull;
        for (int w = 0; w < STAB_WAVES; ++w) {
            cnt += s_cnt[w];
            in += s_in[w];
            amb |= s_amb[w];
            pairs += s_pairs[w];
            pin += s_pin[w];
            dev = s_dev[w] > dev ? s_dev[w] : dev;
            gap = s_gap[w] > gap ? s_gap[w] : gap;
            low = s_low[w] < low ? s_low[w] : low;
        }
        const bool has = real_ok && cnt > 0;
        const int c = cnt;
        StabilityResult* p = out + blockIdx.x;
        p->real_score = real.score;
        p->real_offset = ro;
        p->off_min = has ? s_off[0] : 0;
        p->off_max = has ? s_off[c - 1] : 0;
        p->off_median = has ? s_off[(c - 1) / 2] : 0;
        p->off_lo = has ? s_off[(c - 1) / 20] : 0;
        p->off_hi = has ? s_off[c - 1 - (c - 1) / 20] : 0;
        p->max_dev = has ? dev : 0;
        p->max_pair_gap = gap;
        p->pair_score_min = pairs ? stab_order_value(low) : 0.0;
        p->n_sub = c;
        p->n_within = has ? in : 0;
        p->n_pairs = pairs;
        p->n_pairs_within = pin;
        p->tol = tol;
        p->flags = (has ? 0 : STAB_EMPTY) | (amb ? STAB_AMBIGUOUS : 0) | (pairs ? 0 : STAB_NO_PAIRS);
        p->reserved = 0;
    }
}

}  // namespace ffsa
