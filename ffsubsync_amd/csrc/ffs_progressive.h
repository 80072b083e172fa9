// ffs_progressive.h -- progressive alignment: the quality report of a growing reference prefix, updated per append
// (gfx950).  Score counts are additive over the reference: after n_new more reference samples, n11 of candidate c at
// lag d grows by sum_{j in [L, L + n_new)} r[j] s_c[j - d], so the exact answer so far costs one pass over the new
// samples, not a re-solve.  The contract is this library's own, pinned against tests/progressive_model.py.
//
// A slot holds one file: the plan-owned reference prefix r[0, L) (bits; the words' bits at and beyond L are kept
// zero), its exclusive word prefix popcounts pre_r, and per candidate the plan's copy of its bits (tail bits cleared),
// pre_s, the uint32 curve n11[j] and the score row sc[j] over the lag window d = -W+1 .. W (lag index j = d + W - 1).
//
//   k_prog_open    per (slot, candidate): copy the candidate's words into the plan, write pre_s, zero the curve; the
//                  workgroup of candidate 0 also zeroes the slot's reference words.
//   k_prog_ingest  per slot: bits [first_bit, first_bit + n_new) of the caller's chunk words into the reference at bit
//                  L -- a funnel shift (v_alignbit) with both ends masked; one thread per reference word, so the word
//                  that straddles L has one writer -- then pre_r extended from pre_r[L >> 5], which is final.
//   k_prog_counts  per (slot, candidate, 4096-lag tile): the bit form of k_quality_counts with the roles swapped.  The
//                  new reference words (bits below L masked off) are staged in LDS in pieces of PROG_PIECE words,
//                  with the subtitle words they can meet; thread q holds the 32 lags e = 32q .. 32q+31 of the tile
//                  (e = W - d, so that the subtitle position grows with e), whose subtitle word at reference word w
//                  is a funnel shift of the staged words q+w, q+w+1; each step is a v_bcnt accumulate against the
//                  broadcast reference word.  The workgroup owns its tile of the curve: plain adds, no atomics.
//                  Nothing of the reference before L and nothing of a subtitle outside [L - W, L + n_new + W) is read.
//   (report)       k_quality_peaks, unchanged, on one QualDesc per (slot, candidate) with R = L + n_new.
//   k_prog_pick    per slot: ffs_prog_state from its candidates' records; records of candidates >= n_cand zeroed.
#pragma once
#include "ffs_quality.h"

namespace ffsa {

constexpr int PROG_THREADS = 256;                      // k_prog_open / k_prog_ingest workgroup
constexpr int PROG_CNT_THREADS = 128;                  // k_prog_counts workgroup: one thread per 32 lags
constexpr int PROG_TILE = PROG_CNT_THREADS * 32;       // lags per workgroup
constexpr int PROG_PIECE = 512;                        // reference words staged at a time (16 384 samples)
constexpr int PROG_PICK_THREADS = 64;
constexpr int PROG_MAX_CAND = 8;

struct ProgOpenDesc {  // one per (slot, candidate)
    const uint32_t* src;  // the caller's candidate bits
    uint32_t* s;          // the plan's copy
    int32_t* pre_s;
    uint32_t* curve;      // lpad words
    uint32_t* r;          // candidate 0 only: the slot's reference words (else nullptr)
    int32_t* pre_r;       // ... and its prefix row
    int64_t S, lpad, r_words;
};

struct ProgSlotDesc {  // one per slot of an append
    const uint32_t* chunk;  // the caller's chunk words
    uint32_t* r;
    int32_t* pre_r;
    int64_t L, n_new;  // the prefix before the append, the new samples
    int64_t W;
    int32_t first_bit, n_cand;
    int32_t desc0;     // the slot's first QualDesc (n_cand of them, candidates in order)
    int32_t pad_;
};

struct ProgState {  // = ffs_prog_state
    int64_t ref_len, offset;
    double score, mean, std, runner_up, other_best;
    int32_t best_cand, flags;
};
static_assert(sizeof(ProgState) == 64, "ProgState must match ffs_prog_state");

// pre[g + 1] for g in [g0, g1) from `base` = pre[g0]: exclusive word prefix popcounts of the words v (whose bits outside
// the vector are zero).  Every thread of the PROG_THREADS workgroup calls it.
FFS_DEV void prog_extend_prefix(const uint32_t* v, int32_t* pre, int64_t g0, int64_t g1, int32_t base, int32_t* s_part) {
    const int t = threadIdx.x;
    const int64_t nw = g1 - g0;
    const int64_t per = (nw + PROG_THREADS - 1) / PROG_THREADS;
    const int64_t w0 = g0 + t * per < g1 ? g0 + t * per : g1, w1 = w0 + per < g1 ? w0 + per : g1;
    int32_t sum = 0;
    for (int64_t g = w0; g < w1; ++g) sum += __popc(v[g]);
    __syncthreads();
    s_part[t] = sum;
    __syncthreads();
    for (int off = 1; off < PROG_THREADS; off <<= 1) {  // inclusive Hillis-Steele scan of the thread sums
        const int32_t add = t >= off ? s_part[t - off] : 0;
        __syncthreads();
        s_part[t] += add;
        __syncthreads();
    }
    int32_t run = base + s_part[t] - sum;
    for (int64_t g = w0; g < w1; ++g) {
        run += __popc(v[g]);
        pre[g + 1] = run;
    }
}

__global__ void __launch_bounds__(PROG_THREADS) k_prog_open(const ProgOpenDesc* __restrict__ desc) {
    __shared__ int32_t s_part[PROG_THREADS];
    const ProgOpenDesc d = desc[blockIdx.x];
    const int t = threadIdx.x;
    const int64_t sw = (d.S + 31) >> 5;
    for (int64_t g = t; g < sw; g += PROG_THREADS) d.s[g] = split_word(d.src, d.S, g);
    for (int64_t j = t; j < d.lpad; j += PROG_THREADS) d.curve[j] = 0u;
    if (d.r) {
        for (int64_t g = t; g < d.r_words; g += PROG_THREADS) d.r[g] = 0u;
        if (t == 0) d.pre_r[0] = 0;
    }
    if (t == 0) d.pre_s[0] = 0;
    __syncthreads();  // the copy is read back below by other threads of this workgroup
    prog_extend_prefix(d.s, d.pre_s, 0, sw, 0, s_part);
}

__global__ void __launch_bounds__(PROG_THREADS) k_prog_ingest(const ProgSlotDesc* __restrict__ desc) {
    __shared__ int32_t s_part[PROG_THREADS];
    const ProgSlotDesc d = desc[blockIdx.x];
    const int t = threadIdx.x;
    const int64_t L = d.L, L1 = d.L + d.n_new;
    const int64_t g0 = L >> 5, g1 = (L1 + 31) >> 5;
    // the chunk words that hold new samples: no other is loaded (none at all for an empty append)
    const int64_t n_src = d.n_new > 0 ? ((int64_t)d.first_bit + d.n_new + 31) >> 5 : 0;
    for (int64_t g = g0 + t; g < g1; g += PROG_THREADS) {
        // reference bit 32 g + b is chunk bit p0 + b
        const int64_t p0 = 32 * g - L + d.first_bit;
        const int64_t q = p0 >= 0 ? (p0 >> 5) : -((31 - p0) >> 5);  // floor(p0 / 32)
        const int sh = (int)(p0 - q * 32);
        const uint32_t lo = (q >= 0 && q < n_src) ? d.chunk[q] : 0u;
        const uint32_t hi = (q + 1 >= 0 && q + 1 < n_src) ? d.chunk[q + 1] : 0u;
        uint32_t mask = 0xFFFFFFFFu;
        if (32 * g < L) mask &= 0xFFFFFFFFu << (int)(L - 32 * g);        // (L - 32 g in 1..31)
        if (32 * g + 32 > L1) mask &= 0xFFFFFFFFu >> (int)(32 * g + 32 - L1);  // (in 1..31)
        d.r[g] |= __builtin_amdgcn_alignbit(hi, lo, sh) & mask;  // (the word's bits at and beyond L were zero)
    }
    const int32_t base = d.pre_r[g0];  // words [0, g0) are complete: final
    __syncthreads();  // the new words are read back below by other threads of this workgroup
    prog_extend_prefix(d.r, d.pre_r, g0, g1, base, s_part);
}

// The count loop of one (slot, candidate, 4096-lag tile) workgroup over the reference words [g0, g1): acc[sh] += n11 of
// tile lag 32 t + sh (e = e0 + 32 t + sh = W - d).  The words are staged in LDS in pieces of PROG_PIECE with the subtitle
// words they can meet; word(g) hands over reference word g with every bit that is not to be counted masked off.  Every
// thread of the PROG_CNT_THREADS workgroup calls it; k_prog_counts and k_samp_counts (ffs_sampled.h) differ in the mask.
template <class WordF>
FFS_DEV void prog_count_words(const uint32_t* s, int64_t S, int64_t g0, int64_t g1, int64_t W, int64_t e0, WordF word,
                              uint32_t* s_ref, uint32_t* s_sub, uint32_t (&acc)[32]) {
    const int t = threadIdx.x;
    for (int64_t gp = g0; gp < g1; gp += PROG_PIECE) {
        const int nw = (int)(g1 - gp < PROG_PIECE ? g1 - gp : PROG_PIECE);
        // subtitle bits [base + 32 k, +32) for k <= nw + PROG_CNT_THREADS meet reference word gp + w at tile lag 32 q + sh
        const int64_t base = 32 * gp - W + e0;
        if (base + 32 * (int64_t)(nw + PROG_CNT_THREADS + 1) <= 0 || base >= S) continue;  // (uniform) no subtitle sample
        const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
        const int bsh = (int)(base - gbase * 32);
        __syncthreads();  // the previous piece has been read
        for (int k = t; k <= nw + PROG_CNT_THREADS; k += PROG_CNT_THREADS) {
            const uint32_t lo = split_word(s, S, gbase + k), hi = split_word(s, S, gbase + k + 1);
            s_sub[k] = __builtin_amdgcn_alignbit(hi, lo, bsh);
        }
        for (int w = t; w < nw; w += PROG_CNT_THREADS) s_ref[w] = word(gp + w);
        __syncthreads();
        uint32_t lo = s_sub[t];
        for (int w = 0; w < nw; ++w) {
            const uint32_t rw = s_ref[w];  // (one address per wave: broadcast)
            const uint32_t hi = s_sub[t + w + 1];
#pragma unroll
            for (int sh = 0; sh < 32; ++sh) acc[sh] += __popc(__builtin_amdgcn_alignbit(hi, lo, sh) & rw);
            lo = hi;
        }
    }
}

// n11 of one 4096-lag tile of one candidate over the new reference samples; grid.x = slots * max_cand * n_tiles
__global__ void __launch_bounds__(PROG_CNT_THREADS) k_prog_counts(const ProgSlotDesc* __restrict__ slots,
                                                                   const QualDesc* __restrict__ qd, int n_tiles, int max_cand) {
    __shared__ uint32_t s_ref[PROG_PIECE];
    __shared__ uint32_t s_sub[PROG_PIECE + PROG_CNT_THREADS + 1];
    __shared__ uint32_t s_acc[PROG_CNT_THREADS * 33];  // [q][sh], rows padded to 33 words against bank conflicts
    const int tile = blockIdx.x % n_tiles;
    const int cand = (blockIdx.x / n_tiles) % max_cand;
    const ProgSlotDesc sd = slots[blockIdx.x / (n_tiles * max_cand)];
    const int64_t e0 = (int64_t)tile * PROG_TILE;  // first e = W - d of the tile
    if (cand >= sd.n_cand || e0 >= 2 * sd.W || sd.n_new <= 0) return;  // (uniform)
    const QualDesc d = qd[sd.desc0 + cand];
    const int64_t L = sd.L, L1 = sd.L + sd.n_new;
    const int64_t g0 = L >> 5, g1 = (L1 + 31) >> 5;
    const int t = threadIdx.x;
    uint32_t acc[32];
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) acc[sh] = 0;
    prog_count_words(
        d.s, d.S, g0, g1, sd.W, e0,
        [&](int64_t g) {
            uint32_t rw = d.r[g];  // (bits at and beyond L1 are zero)
            if (32 * g < L) rw &= 0xFFFFFFFFu << (int)(L - 32 * g);  // counted by earlier appends
            return rw;
        },
        s_ref, s_sub, acc);
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) s_acc[t * 33 + sh] = acc[sh];
    __syncthreads();
    const int64_t n_here = 2 * sd.W - e0 < PROG_TILE ? 2 * sd.W - e0 : PROG_TILE;
    uint32_t* top = d.curve + (2 * sd.W - 1 - e0);  // lag index j = d + W - 1 = 2W - 1 - e
    for (int l = t; l < n_here; l += PROG_CNT_THREADS) {
        const uint32_t v = s_acc[(l >> 5) * 33 + (l & 31)];
        if (v) *(top - l) += v;  // this workgroup owns the tile
    }
}

// one workgroup per slot: the slot's state from its candidates' records; the records of candidates >= n_cand as zeros
__global__ void __launch_bounds__(PROG_PICK_THREADS) k_prog_pick(const ProgSlotDesc* __restrict__ slots, int max_cand,
                                                                 QualResult* __restrict__ cand_out,
                                                                 ProgState* __restrict__ state_out) {
    const ProgSlotDesc sd = slots[blockIdx.x];
    QualResult* rec = cand_out + (int64_t)blockIdx.x * max_cand;
    const int t = threadIdx.x;
    constexpr int REC_WORDS = (int)(sizeof(QualResult) / 8);
    for (int i = t; i < (max_cand - sd.n_cand) * REC_WORDS; i += PROG_PICK_THREADS)
        ((unsigned long long*)(rec + sd.n_cand))[i] = 0ull;
    if (t != 0) return;
    int best = 0;
    for (int c = 1; c < sd.n_cand; ++c)
        if (rec[c].peak_score[0] > rec[best].peak_score[0]) best = c;  // the smallest index on ties
    double other = NAN;
    for (int c = 0; c < sd.n_cand; ++c)
        if (c != best && !(rec[c].peak_score[0] <= other)) other = rec[c].peak_score[0];  // (NaN: nothing yet)
    ProgState st;
    st.ref_len = sd.L + sd.n_new;
    st.offset = rec[best].peak_offset[0];
    st.score = rec[best].peak_score[0];
    st.mean = rec[best].mean;
    st.std = rec[best].std;
    st.runner_up = rec[best].n_peaks > 1 ? rec[best].peak_score[1] : NAN;
    st.other_best = other;
    st.best_cand = best;
    st.flags = rec[best].flags;
    state_out[blockIdx.x] = st;
}

}  // namespace ffsa
