// ffs_sampled.h -- sampled alignment: the quality report of a reference read in segments, updated per segment (gfx950).
// A sampled slot of the progressive plan (ffs_progressive.h) holds a reference of declared length T of which disjoint
// intervals [a, b) arrive in any order; K is their union.  Unread frames contribute nothing: the counts of candidate c at
// lag d run over I(d) = { i : 0 <= i < S_c, i + d in K },
//     ov = |I|,  n11 = sum_I s[i] r[i+d],  n1x = sum_I s[i],  nx1 = sum_I r[i+d],
// and the score is two_level_score's expression on them with ov in place of the overlap length (0.0 where ov = 0) --
// what the reference aligner computes on a vector that holds 0.5 in every unread frame, since 2 * 0.5 - 1 = 0.  All four
// counts are additive over the intervals, so an append costs one pass over its own samples whatever is already known.
// The contract is this library's own, pinned against tests/sampled_model.py.
//
// A sampled slot keeps what a prefix slot keeps (the reference words r, zero outside K; pre_r over ALL words of [0, T);
// per candidate s, pre_s, the n11 curve and the score row) plus three uint32 side curves ov, n1x, nx1 per candidate.
//
//   k_samp_zero    per (slot, candidate), behind k_prog_open: zero the side curves; candidate 0 also zeroes pre_r.
//   k_samp_ingest  per slot: bits [first_bit, first_bit + n) of the chunk into r at [a, b) -- k_prog_ingest's funnel
//                  shift, one writer per word, both ends masked (the straddling words may hold a neighbour's bits) --
//                  then pre_r recomputed from word a >> 5 to the END of the reference: every later entry moved, and
//                  pre_r[a >> 5] is final because no earlier word changed.
//   k_samp_counts  per (slot, candidate, 4096-lag tile): k_prog_counts' staging and 32-lags-per-thread funnel-shift /
//                  v_bcnt loop (prog_count_words, shared with it) on the words of [a, b), masked at BOTH ends (a known
//                  neighbour may share either word);
//                  the epilogue adds this interval's share of ov, n1x, nx1 per lag of the tile from four prefix lookups
//                  with i0 = max(a - d, 0), i1 = min(b - d, S).  The workgroup owns its tile: plain adds.
//   k_samp_peaks   per (slot, candidate): quality_curve_moments / quality_curve_peaks on a score that reads the four
//                  curves.
//   (pick)         k_prog_pick, unchanged, on ProgSlotDesc with L = |K| before the append.
#pragma once
#include "ffs_progressive.h"

namespace ffsa {

struct SampOpenDesc {  // one per (slot, candidate)
    uint32_t* side;    // ov, n1x, nx1: three rows of lpad words
    int32_t* pre_r;    // candidate 0 only (else nullptr)
    int64_t lpad, r_words;
};

struct SampSlotDesc {  // one per slot of an append
    const uint32_t* chunk;
    uint32_t* r;
    int32_t* pre_r;
    int64_t a, n_new;  // the interval [a, a + n_new)
    int64_t T, W;
    int32_t first_bit, n_cand;
    int32_t desc0;     // the slot's first SampDesc (n_cand of them, candidates in order)
    int32_t pad_;
};

struct SampDesc {  // one per (slot, candidate)
    const uint32_t* s;
    const int32_t* pre_s;
    uint32_t* n11;   // lpad words each, lag index j = d + W - 1
    uint32_t* side;  // ov at [0, lpad), n1x at [lpad, 2 lpad), nx1 at [2 lpad, 3 lpad)
    double* sc;
    int64_t S, lpad, n_lags, d_lo, out_row;
    double s0, s1, r0, r1;  // mapped levels
};

__global__ void __launch_bounds__(PROG_THREADS) k_samp_zero(const SampOpenDesc* __restrict__ desc) {
    const SampOpenDesc d = desc[blockIdx.x];
    for (int64_t j = threadIdx.x; j < 3 * d.lpad; j += PROG_THREADS) d.side[j] = 0u;
    if (d.pre_r)
        for (int64_t g = threadIdx.x; g < d.r_words; g += PROG_THREADS) d.pre_r[g] = 0;
}

__global__ void __launch_bounds__(PROG_THREADS) k_samp_ingest(const SampSlotDesc* __restrict__ desc) {
    __shared__ int32_t s_part[PROG_THREADS];
    const SampSlotDesc d = desc[blockIdx.x];
    if (d.n_new <= 0) return;  // (uniform) a re-report
    const int t = threadIdx.x;
    const int64_t a = d.a, b = d.a + d.n_new;
    const int64_t g0 = a >> 5, g1 = (b + 31) >> 5;
    const int64_t n_src = ((int64_t)d.first_bit + d.n_new + 31) >> 5;  // the chunk words that hold new samples
    for (int64_t g = g0 + t; g < g1; g += PROG_THREADS) {
        // reference bit 32 g + k is chunk bit p0 + k
        const int64_t p0 = 32 * g - a + d.first_bit;
        const int64_t q = p0 >= 0 ? (p0 >> 5) : -((31 - p0) >> 5);  // floor(p0 / 32)
        const int sh = (int)(p0 - q * 32);
        const uint32_t lo = (q >= 0 && q < n_src) ? d.chunk[q] : 0u;
        const uint32_t hi = (q + 1 >= 0 && q + 1 < n_src) ? d.chunk[q + 1] : 0u;
        uint32_t mask = 0xFFFFFFFFu;
        if (32 * g < a) mask &= 0xFFFFFFFFu << (int)(a - 32 * g);            // (a - 32 g in 1..31)
        if (32 * g + 32 > b) mask &= 0xFFFFFFFFu >> (int)(32 * g + 32 - b);  // (in 1..31)
        d.r[g] |= __builtin_amdgcn_alignbit(hi, lo, sh) & mask;  // (the bits of [a, b) were zero: disjoint from K)
    }
    const int32_t base = d.pre_r[g0];  // no word before g0 changed: final
    __syncthreads();  // the new words are read back below by other threads of this workgroup
    prog_extend_prefix(d.r, d.pre_r, g0, (d.T + 31) >> 5, base, s_part);
}

// n11, ov, n1x, nx1 of one 4096-lag tile of one candidate over the interval; grid.x = slots * max_cand * n_tiles
__global__ void __launch_bounds__(PROG_CNT_THREADS) k_samp_counts(const SampSlotDesc* __restrict__ slots,
                                                                   const SampDesc* __restrict__ qd, int n_tiles, int max_cand) {
    __shared__ uint32_t s_ref[PROG_PIECE];
    __shared__ uint32_t s_sub[PROG_PIECE + PROG_CNT_THREADS + 1];
    __shared__ uint32_t s_acc[PROG_CNT_THREADS * 33];  // [q][sh], rows padded to 33 words against bank conflicts
    const int tile = blockIdx.x % n_tiles;
    const int cand = (blockIdx.x / n_tiles) % max_cand;
    const SampSlotDesc sd = slots[blockIdx.x / (n_tiles * max_cand)];
    const int64_t e0 = (int64_t)tile * PROG_TILE;  // first e = W - d of the tile
    if (cand >= sd.n_cand || e0 >= 2 * sd.W || sd.n_new <= 0) return;  // (uniform)
    const SampDesc d = qd[sd.desc0 + cand];
    const int64_t a = sd.a, b = sd.a + sd.n_new;
    const int64_t g0 = a >> 5, g1 = (b + 31) >> 5;
    const int t = threadIdx.x;
    uint32_t acc[32];
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) acc[sh] = 0;
    prog_count_words(
        d.s, d.S, g0, g1, sd.W, e0,
        [&](int64_t g) {
            const int64_t at = 32 * g;
            uint32_t rw = sd.r[g];
            if (at < a) rw &= 0xFFFFFFFFu << (int)(a - at);            // a known neighbour in front: counted by its append
            if (at + 32 > b) rw &= 0xFFFFFFFFu >> (int)(at + 32 - b);  // ... and one behind
            return rw;
        },
        s_ref, s_sub, acc);
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) s_acc[t * 33 + sh] = acc[sh];
    __syncthreads();
    const int64_t n_here = 2 * sd.W - e0 < PROG_TILE ? 2 * sd.W - e0 : PROG_TILE;
    const int64_t jtop = 2 * sd.W - 1 - e0;  // lag index j = d + W - 1 = 2W - 1 - e
    for (int l = t; l < n_here; l += PROG_CNT_THREADS) {  // this workgroup owns the tile: plain adds
        const int64_t j = jtop - l;
        const uint32_t v = s_acc[(l >> 5) * 33 + (l & 31)];
        if (v) d.n11[j] += v;
        const int64_t lag = sd.W - e0 - l;
        const int64_t i0 = a - lag > 0 ? a - lag : 0;
        const int64_t i1 = b - lag < d.S ? b - lag : d.S;
        if (i1 > i0) {  // subtitle samples [i0, i1) meet reference samples [i0 + lag, i1 + lag) of [a, b)
            d.side[j] += (uint32_t)(i1 - i0);
            d.side[d.lpad + j] += (uint32_t)(split_prefix_at(d.pre_s, d.s, i1) - split_prefix_at(d.pre_s, d.s, i0));
            d.side[2 * d.lpad + j] +=
                (uint32_t)(split_prefix_at(sd.pre_r, sd.r, i1 + lag) - split_prefix_at(sd.pre_r, sd.r, i0 + lag));
        }
    }
}

// the score of lag index j: exactly 0.0 where nothing known is met, else two_level_score's expression on the counts
FFS_DEV double samp_score(const SampDesc& d, int64_t j) {
    const int ov = (int)d.side[j];
    if (ov == 0) return 0.0;
    const int n11 = (int)d.n11[j];
    const int n10 = (int)d.side[d.lpad + j] - n11, n01 = (int)d.side[2 * d.lpad + j] - n11;
    const int n00 = ov - n11 - n10 - n01;
    double r = (double)n00 * (d.s0 * d.r0);
    r = __builtin_fma((double)n01, d.s0 * d.r1, r);
    r = __builtin_fma((double)n10, d.s1 * d.r0, r);
    return __builtin_fma((double)n11, d.s1 * d.r1, r);
}

// one workgroup per (slot, candidate): scores, moments and greedy peaks into the candidate's ffs_quality_result
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_samp_peaks(const SampDesc* __restrict__ desc, int top_k,
                                                                  int64_t exclusion, QualResult* __restrict__ out) {
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    const SampDesc d = desc[blockIdx.x];
    const int64_t n = d.n_lags;  // 2W >= 2
    QualResult* rec = out + d.out_row;
    double mean, sd;
    bool flat;
    quality_curve_moments(
        n,
        [&](int64_t j) {
            const double v = samp_score(d, j);
            d.sc[j] = v;  // (read back below by this same thread only)
            return v;
        },
        [&](int64_t j) { return d.sc[j]; }, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(n, [&](int64_t j) { return d.sc[j]; }, top_k, exclusion, s_peak, s_pscore);
    if (threadIdx.x == 0) {
        for (int k = 0; k < QUAL_MAX_PEAKS; ++k) {
            rec->peak_score[k] = k < n_peaks ? s_pscore[k] : 0.0;
            rec->peak_offset[k] = k < n_peaks ? d.d_lo + s_peak[k] : 0;
        }
        rec->mean = mean;
        rec->std = sd;
        rec->n_lags = n;
        rec->n_peaks = n_peaks;
        rec->flags = flat ? QUAL_FLAT : 0;
    }
}

}  // namespace ffsa
