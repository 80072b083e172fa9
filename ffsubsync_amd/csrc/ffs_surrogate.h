// ffs_surrogate.h -- shuffled-cue surrogates of a boundary list and the empirical null of their scores (gfx950): the
// device side of ffsubsync_amd/surrogate.py.
//
// "Can this sync be trusted?" without a tuned threshold: compare the window-maximum score of the real subtitle with the
// scores of K surrogate subtitles that keep every cue, every silence, the length and the number of speech samples and
// differ only in which cue sits where.  Contract (include/ffsubsync_amd.h, ffs_surrogate_lists / ffs_null_stats), pinned
// against tests/surrogate_model.py:
//   - a list of n boundaries has m = n / 2 runs; unit j < m - 1 = run j and the silence behind it.  The silence in
//     front of run 0, the last run and the tail stay where they are
//   - the U = m - 1 units are cut into nb = ceil(U / B) blocks of B consecutive units (the last may be short); surrogate
//     s places the blocks in ascending order of (key(seed, s, b), b), key = fmix32(fmix32(seed + 0x9E3779B9 (s + 1)) ^ b)
//   - the output is a valid list with the same n, ones and len
//
// k_surrogate_lists: one 256-thread workgroup per (vector, surrogate).  fmix32 is a bijection of uint32, so the keys of
// one surrogate -- fmix32 of distinct words -- are distinct: the index half of the (key, b) order never decides, the sort
// carries the 32-bit keys alone and a place's source block is read back out of its key (b = fmix32^-1(key) ^ hash of the
// surrogate).  The keys are sorted by a bitonic network in LDS: thread t owns the compare-exchanges t, t + 256, ... of
// every step, and a workgroup barrier separates the steps (66 of them for a 2 048-key sort).  Each thread then takes a
// contiguous piece of the sorted order, reads the span and the ones of its blocks from the input list by differences
// at the block edges, and a workgroup exclusive scan of the two sums (packed into one 64-bit word: both stay below
// 2^30) gives every block its place.  All blocks but the last hold B units, so a block's first output unit follows from
// the sorted position of the short block alone.  What stays in LDS per place is its key and the shift of its positions
// and of its ones_before (12 bytes: 96 KiB at the unit limit with B = 1, 24 KiB for a 2 000-cue subtitle).  The write:
// thread t writes entries t, t + 256, ...: one 8-byte load of the source entry (global memory; the list stays in L2
// across the K workgroups of a vector), one add, one 8-byte store, consecutive threads to consecutive entries.  The
// vectors' descriptors (SurrVec) are uploaded behind the caller's stream by the host call.
//
// k_null_stats: one 256-thread workgroup per file over its K + 1 solve records, shaped like k_sweep_peaks.
#pragma once
#include "ffs_kernels.h"
#include "ffs_sweep.h"

namespace ffsa {

constexpr int SURR_THREADS = 256;
constexpr int SURR_WAVES = SURR_THREADS / 64;
constexpr int SURR_MAX_UNITS = 8192;  // FFS_SURR_MAX_UNITS
constexpr int SURR_MAX_K = 4096;      // FFS_SURR_MAX_K
constexpr int32_t SURR_BAD_ODD = 1;        // FFS_SURR_BAD_ODD
constexpr int32_t SURR_BAD_TRUNCATED = 2;  // FFS_SURR_BAD_TRUNCATED
constexpr int32_t SURR_BAD_BOUND = 4;      // FFS_SURR_BAD_BOUND
constexpr int32_t SURR_BAD_UNITS = 8;      // FFS_SURR_BAD_UNITS
constexpr int32_t NULL_FLAT = 1;       // FFS_NULL_FLAT
constexpr int32_t NULL_EMPTY = 2;      // FFS_NULL_EMPTY
constexpr int32_t NULL_AMBIGUOUS = 4;  // FFS_NULL_AMBIGUOUS

struct SurrVec {
    const char* list;   // the input block (8-byte aligned)
    long long out_off;  // byte offset of surrogate 0's block; surrogate s follows at s * (16 + 8 * cap_out)
    uint32_t seed;
    int32_t n_bound;
    int32_t cap_out;
    int32_t pad;
};
static_assert(sizeof(SurrVec) == 32, "SurrVec is 32 bytes");

struct NullResult {  // = ffs_null_result
    double real_score, null_mean, null_std, null_min, null_max;
    int32_t n_null, n_ge, n_gt, flags;
};
static_assert(sizeof(NullResult) == 56, "NullResult must match ffs_null_result");

FFS_DEV uint32_t surr_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// its inverse: the multipliers' inverses mod 2^32, the xor-shifts undone
FFS_DEV uint32_t surr_unmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7ED1B41Du;
    h ^= (h >> 13) ^ (h >> 26);
    h *= 0xA5CB9243u;
    h ^= h >> 16;
    return h;
}
static_assert((uint32_t)(0x85EBCA6Bu * 0xA5CB9243u) == 1u && (uint32_t)(0xC2B2AE35u * 0x7ED1B41Du) == 1u,
              "surr_unmix32 must invert surr_fmix32");

// smallest power of two >= max(x, 1)
inline __host__ __device__ int surr_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}
// dynamic LDS of k_surrogate_lists for lists of up to `blocks` blocks
inline size_t surr_lds_bytes(int blocks) { return (size_t)surr_pow2(blocks) * 12; }

__global__ void __launch_bounds__(SURR_THREADS) k_surrogate_lists(const SurrVec* __restrict__ vecs, int n_surr, int block_units,
                                                                  char* __restrict__ out, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long s_wave[SURR_WAVES];
    __shared__ int s_short;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int v = (int)(blockIdx.x / (unsigned)n_surr), s = (int)(blockIdx.x % (unsigned)n_surr);
    const SurrVec d = vecs[v];
    const int2* hdr = (const int2*)d.list;
    const int2* __restrict__ e = hdr + 2;
    const int2 h0 = hdr[0], h1 = hdr[1];
    const int n = h0.x, ones = h0.y, len = h1.x, cap = h1.y;
    int2* oh = (int2*)(out + d.out_off + (long long)s * (16 + 8 * (long long)d.cap_out));
    int2* __restrict__ oe = oh + 2;

    int32_t bad = 0;
    if (n & 1) bad |= SURR_BAD_ODD;
    if (n < 0 || n >= cap) bad |= SURR_BAD_TRUNCATED;
    if (n > d.n_bound) bad |= SURR_BAD_BOUND;
    if (n / 2 - 1 > SURR_MAX_UNITS) bad |= SURR_BAD_UNITS;
    if (s == 0 && t == 0) status[v] = bad;
    if (bad) {  // (uniform) an unusable list: every surrogate is the empty list of the same length
        if (t == 0) {
            oh[0] = make_int2(0, 0);
            oh[1] = make_int2(len, d.cap_out);
            oe[0] = make_int2(INT32_MAX, 0);
        }
        return;
    }
    const int B = block_units;
    const int U = n >= 4 ? n / 2 - 1 : 0;
    const int nb = (U + B - 1) / B;
    const int P = surr_pow2(nb);
    uint32_t* skey = (uint32_t*)smem;  // the keys, sorted; a place's source block is surr_unmix32(key) ^ hs
    int* spos = (int*)smem + P;        // shift of pos per place
    int* sones = (int*)smem + 2 * P;   // shift of ones_before per place
    const uint32_t hs = surr_fmix32(d.seed + 0x9E3779B9u * (uint32_t)(s + 1));
    if (t == 0) s_short = 0;

    if (nb > 0) {
        // (a key equal to the padding value 0xFFFFFFFF sorts among the padding, and any of those equal words serves)
        for (int i = t; i < P; i += SURR_THREADS) skey[i] = i < nb ? surr_fmix32(hs ^ (uint32_t)i) : 0xFFFFFFFFu;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < (P >> 1); i += SURR_THREADS) {
                    const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                    const uint32_t x = skey[a], y = skey[b];
                    if ((x > y) == ((a & k) == 0)) {
                        skey[a] = y;
                        skey[b] = x;
                    }
                }
                __syncthreads();
            }
        }
        // spans and ones of this thread's places, by differences at the block edges
        const int per = P > SURR_THREADS ? P / SURR_THREADS : 1;
        const int i0 = t * per < nb ? t * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
        const int2 e0 = e[0];
        int span = 0, on = 0;
        for (int i = i0; i < i1; ++i) {
            const int b = (int)(surr_unmix32(skey[i]) ^ hs);
            const int u0 = b * B, u1 = u0 + B < U ? u0 + B : U;
            const int2 a0 = e[2 * u0], a1 = e[2 * u1];
            spos[i] = span - (a0.x - e0.x);
            sones[i] = on - (a0.y - e0.y);
            span += a1.x - a0.x;
            on += a1.y - a0.y;
            if (b == nb - 1) s_short = i;
        }
        // workgroup exclusive scan of (span, ones)
        const unsigned long long mine = ((unsigned long long)(unsigned)span << 32) | (unsigned)on;
        unsigned long long inc = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned long long before = inc - mine;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        const int dspan = (int)(before >> 32), dones = (int)(unsigned)before;
        for (int i = i0; i < i1; ++i) {
            spos[i] += dspan;
            sones[i] += dones;
        }
    }
    __syncthreads();
    const int sp = s_short, tail = U - (nb - 1) * B;  // the short block's place and its units
    for (int k = t; k <= n; k += SURR_THREADS) {
        int2 val;
        if (k == n) {
            val = make_int2(INT32_MAX, ones);
        } else if (k >= 2 * U) {
            val = e[k];
        } else {
            const int q = k >> 1;
            int i, r;
            if (q < sp * B) {
                i = q / B;
                r = q - i * B;
            } else if (q < sp * B + tail) {
                i = sp;
                r = q - sp * B;
            } else {
                const int qq = q - sp * B - tail;
                i = sp + 1 + qq / B;
                r = qq - (qq / B) * B;
            }
            const int b = (int)(surr_unmix32(skey[i]) ^ hs);
            val = e[2 * (b * B + r) + (k & 1)];
            val.x += spos[i];
            val.y += sones[i];
        }
        oe[k] = val;
    }
    if (t == 0) {
        oh[0] = make_int2(n, ones);
        oh[1] = make_int2(len, d.cap_out);
    }
}

// File f owns records rec[f * (K + 1) ..]: record 0 the real list's solve, records 1..K the surrogates'.
__global__ void __launch_bounds__(SWEEP_THREADS) k_null_stats(const CandResult* __restrict__ rec, int n_surr,
                                                              NullResult* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_part[SWEEP_WAVES];
    __shared__ double s_mn[SWEEP_WAVES], s_mx[SWEEP_WAVES];
    __shared__ int s_cnt[SWEEP_WAVES], s_ge[SWEEP_WAVES], s_gt[SWEEP_WAVES], s_amb[SWEEP_WAVES];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const CandResult* r = rec + (int64_t)blockIdx.x * (n_surr + 1);
    const CandResult real = r[0];
    const bool real_ok = !sweep_skipped(real);

    // pass 1: count, sum, min and max of the usable null records, how many reach the real score; any AMBIGUOUS record
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    int cnt = 0, ge = 0, gt = 0, amb = (real.flags & SWEEP_REC_AMBIGUOUS) != 0;
    for (int j = 1 + t; j <= n_surr; j += SWEEP_THREADS) {
        const CandResult c = r[j];
        amb |= (c.flags & SWEEP_REC_AMBIGUOUS) != 0;
        if (sweep_skipped(c)) continue;
        sum += c.score;
        mn = fmin(mn, c.score);
        mx = fmax(mx, c.score);
        ++cnt;
        ge += real_ok && c.score >= real.score;
        gt += real_ok && c.score > real.score;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, s, 64));
        mx = fmax(mx, __shfl_xor(mx, s, 64));
        cnt += __shfl_xor(cnt, s, 64);
        ge += __shfl_xor(ge, s, 64);
        gt += __shfl_xor(gt, s, 64);
        amb |= __shfl_xor(amb, s, 64);
    }
    if (lane == 0) {
        s_mn[wave] = mn;
        s_mx[wave] = mx;
        s_cnt[wave] = cnt;
        s_ge[wave] = ge;
        s_gt[wave] = gt;
        s_amb[wave] = amb;
    }
    const double total = sweep_block_sum(sum, s_part);  // (its barriers publish the arrays above)
    cnt = ge = gt = amb = 0;
    for (int w = 0; w < SWEEP_WAVES; ++w) {
        mn = fmin(mn, s_mn[w]);
        mx = fmax(mx, s_mx[w]);
        cnt += s_cnt[w];
        ge += s_ge[w];
        gt += s_gt[w];
        amb |= s_amb[w];
    }
    const bool flat = cnt == 0 || mn == mx;
    const double mean = cnt == 0 ? 0.0 : (flat ? mx : total / (double)cnt);

    // pass 2: the centred sum of squares
    double ss = 0.0;
    if (!flat) {
        for (int j = 1 + t; j <= n_surr; j += SWEEP_THREADS) {
            const CandResult c = r[j];
            if (sweep_skipped(c)) continue;
            const double dlt = c.score - mean;
            ss += dlt * dlt;
        }
    }
    const double css = sweep_block_sum(ss, s_part);
    if (t == 0) {
        NullResult* p = out + blockIdx.x;
        p->real_score = real.score;
        p->null_mean = mean;
        p->null_std = flat ? 0.0 : sqrt(css / (double)cnt);
        p->null_min = cnt ? mn : 0.0;
        p->null_max = cnt ? mx : 0.0;
        p->n_null = cnt;
        p->n_ge = ge;
        p->n_gt = gt;
        p->flags = (flat ? NULL_FLAT : 0) | (cnt == 0 || !real_ok ? NULL_EMPTY : 0) | (amb ? NULL_AMBIGUOUS : 0);
    }
}

}  // namespace ffsa
