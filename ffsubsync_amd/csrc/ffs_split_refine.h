// ffs_split_refine.h -- sample-exact break refinement after a split solve (gfx950).  The split DP places every break on a
// block boundary; here each break gets two sample-exact cut points t1 <= t2 from exact integer counts.  The contract is
// this library's own, pinned against the numpy model tests/split_refine_model.py, bit for bit.
//
// Per pair: two-level reference r (R samples), subtitle s (S samples), block offsets o_b (b < B = ceil(S/K)), block
// length K, radius Rr (1 <= Rr <= REFINE_MAX_RADIUS) and unmatched margin beta (>= 0, or NaN for a single cut).
// Breaks are the blocks f_j (j = 1..n) with o_{f_j} != o_{f_j - 1}; break j sits at c_j = f_j K between the offsets
// o_a = o_{f_j - 1} and o_b = o_{f_j}; c_0 = 0, c_{n+1} = S.  Window:
//     L_j = max(c_j - Rr, j == 1 ? 0 : floor((c_{j-1} + c_j) / 2)),  U_j = min(c_j + Rr, j == n ? S : floor((c_j + c_{j+1}) / 2))
// A(t): split_mix of the counts (ov, n11, n1x, nx1) of subtitle samples [L, t) at lag o_a; B(t): of [t, U) at lag o_b;
// samples whose partner lies outside the reference are absent, as in the split.  Null score of a sample
// z_x = s~_x * rbar + beta * |s~_x| (s~_x = 2 lvl_s[x] - 1; rbar = ((R - P1) * r~_0 + P1 * r~_1) / R, P1 = popcount of r);
// N(t) = n0 * z0 + n1 * z1 over [L, t).  F(t) = A(t) - N(t), G(t) = N(t) + B(t).  t2 = the smallest maximiser over
// t in [L, U] of G(t) + max_{L <= t' <= t} F(t'); t1 = the smallest maximiser of F on [L, t2].  beta = NaN: t1 = t2 = the
// smallest maximiser of A(t) + B(t).  Every value is a fixed fp64 expression of integer counts, each operation rounded on
// its own (no FMA).
//
// Two kernels per sub-batch of pairs (the split plan's pairs_in_flight):
//   k_refine_breaks  one workgroup per pair: numbers the breaks with a workgroup scan (wave ballots), writes each break's
//                    block, cut, offsets and window into its record, zeroes the records past the count, stores the count,
//                    and reduces the reference's popcount into rbar, z0, z1 (the pair's slot of the plan's refine scratch).
//   k_refine_cut     one workgroup per (pair, break slot; slots past the count return at once).  Each thread owns a
//                    contiguous run of the window's words.  Pass 1: per word the nine masks (presence, n11, n1x, nx1 at
//                    o_a and at o_b, subtitle bits; the reference word at an arbitrary shift is a v_alignbit of two
//                    words) and their popcounts, then an exclusive workgroup scan of the nine sums (wave shuffles, LDS
//                    across the waves).  Pass 2 (beta given): every sample's F from the scanned counts plus masked
//                    popcounts inside the word, the thread's (max, first index), and an exclusive workgroup scan of
//                    those.  Pass 3: the running prefix max M, G(t) + M(t), the thread's first maximiser, and a
//                    workgroup argmax (smallest t on ties).
#pragma once
#include "ffs_kernels.h"
#include "ffs_split.h"

namespace ffsa {

constexpr int REFINE_TABLE_THREADS = 1024;  // k_refine_breaks workgroup (one per pair)
constexpr int REFINE_THREADS = 256;         // k_refine_cut workgroup (one per break)
constexpr int64_t REFINE_MAX_RADIUS = 131072;  // FFS_REFINE_MAX_RADIUS: a window of <= 8194 words, <= 33 per thread
constexpr int32_t REFINE_CLIPPED = 1;       // FFS_REFINE_CLIPPED
constexpr int32_t REFINE_AT_EDGE = 2;       // FFS_REFINE_AT_EDGE
constexpr int32_t REFINE_UNMATCHED = 4;     // FFS_REFINE_UNMATCHED
constexpr int REFINE_NC = 9;                // counts per word: ov, n11, n1x, nx1 at o_a; the same at o_b; subtitle ones

struct RefineDesc {
    const uint32_t* r;  // reference bits (FFS_DTYPE_U1)
    const uint32_t* s;  // subtitle bits
    int64_t R, S;
    double r0, r1, s0, s1;      // 2 * level - 1
    double c00, c01, c10, c11;  // s~_x * r~_y, as SplitDesc
    double* pair_ws;    // scratch: [0] = z0, [1] = z1, [2] = rbar
    int64_t out_row;    // pair index in the caller's outputs
};

struct BreakRefine {  // = ffs_break_refine
    int64_t block, cut;       // f_j, c_j = f_j K
    int64_t lo, hi;           // window [L, U]
    int64_t t1, t2;
    int64_t offset_prev, offset_next;  // o_a, o_b
    double coarse_score;      // A(c) + B(c)
    double refined_score;     // F(t1) + G(t2); A(t1) + B(t1) for a single cut
    int32_t flags, reserved;
};
static_assert(sizeof(BreakRefine) == 88, "BreakRefine must match ffs_break_refine");

// split_mix of RefineDesc's weights: ((n00*c00 + n01*c01) + n10*c10) + n11*c11, every operation rounded on its own
FFS_DEV double refine_mix(const RefineDesc& d, int32_t ov, int32_t n11, int32_t n1x, int32_t nx1) {
#pragma clang fp contract(off)
    const int32_t n10 = n1x - n11, n01 = nx1 - n11, n00 = ov - n11 - n10 - n01;
    return (((double)n00 * d.c00 + (double)n01 * d.c01) + (double)n10 * d.c10) + (double)n11 * d.c11;
}

// bits k of word g with lo <= 32 g + k < hi
FFS_DEV uint32_t refine_range_mask(int64_t g, int64_t lo, int64_t hi) {
    const int64_t base = g * 32;
    const int64_t a = lo - base < 0 ? 0 : (lo - base > 32 ? 32 : lo - base);
    const int64_t e = hi - base < 0 ? 0 : (hi - base > 32 ? 32 : hi - base);
    if (e <= a) return 0u;
    const uint32_t upto = e == 32 ? 0xffffffffu : (1u << e) - 1u;
    return upto & ~((1u << a) - 1u);
}

// reference bits at samples 32 g + k + lag (zero outside [0, R)): a funnel shift of two words, as k_split_counts
FFS_DEV uint32_t refine_ref_word(const RefineDesc& d, int64_t g, int64_t lag) {
    const int64_t base = g * 32 + lag;
    const int64_t gb = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
    const int sh = (int)(base - gb * 32);
    return __builtin_amdgcn_alignbit(split_word(d.r, d.R, gb + 1), split_word(d.r, d.R, gb), sh);
}

// the nine masks of word g of the window [lo, hi) at the lags oa, ob
FFS_DEV void refine_masks(const RefineDesc& d, int64_t g, int64_t lo, int64_t hi, int64_t oa, int64_t ob,
                          uint32_t (&m)[REFINE_NC]) {
    const uint32_t win = refine_range_mask(g, lo, hi);
    const uint32_t sw = split_word(d.s, d.S, g) & win;
    const int64_t lag[2] = {oa, ob};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int64_t plo = lo > -lag[q] ? lo : -lag[q], phi = hi < d.R - lag[q] ? hi : d.R - lag[q];
        const uint32_t pres = refine_range_mask(g, plo, phi);
        const uint32_t rw = refine_ref_word(d, g, lag[q]) & win;  // zero where the partner is outside the reference
        m[4 * q + 0] = pres;
        m[4 * q + 1] = sw & rw;
        m[4 * q + 2] = sw & pres;
        m[4 * q + 3] = rw;
    }
    m[8] = sw;
}

// one workgroup per pair: break table, windows, zeroed tail, break count, null-score constants
__global__ void __launch_bounds__(REFINE_TABLE_THREADS) k_refine_breaks(const RefineDesc* __restrict__ desc, int K,
                                                                        int64_t out_stride, int64_t radius, double beta,
                                                                        const int32_t* __restrict__ block_offset,
                                                                        BreakRefine* __restrict__ out,
                                                                        int32_t* __restrict__ n_breaks_out) {
#pragma clang fp contract(off)
    constexpr int NW = REFINE_TABLE_THREADS / 64;
    __shared__ int s_cnt[NW];
    __shared__ unsigned long long s_pop[NW];
    const RefineDesc d = desc[blockIdx.x];
    const int64_t B = (d.S + K - 1) / K;
    const int32_t* o = block_offset + d.out_row * out_stride;
    BreakRefine* rec = out + d.out_row * out_stride;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;  // breaks before this chunk of blocks
    for (int64_t b0 = 0; b0 < B; b0 += REFINE_TABLE_THREADS) {
        const int64_t b = b0 + t;
        const bool brk = b >= 1 && b < B && o[b] != o[b - 1];
        const unsigned long long m = __ballot(brk);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = carry, chunk = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_cnt[w] : 0;
            chunk += s_cnt[w];
        }
        if (brk) {
            const int idx = before + __popcll(m & ((1ull << lane) - 1ull));
            rec[idx].block = b;
            rec[idx].cut = b * K;
            rec[idx].offset_prev = o[b - 1];
            rec[idx].offset_next = o[b];
        }
        carry += chunk;
        __syncthreads();  // before the next chunk rewrites s_cnt
    }
    __threadfence_block();
    __syncthreads();  // the cuts of every break are written
    const int n = carry;
    for (int j = t; j < n; j += REFINE_TABLE_THREADS) {
        const int64_t c = rec[j].cut;
        int32_t flags = 0;
        int64_t lo = c - radius, hi = c + radius;
        if (j == 0) {
            lo = lo > 0 ? lo : 0;
        } else {
            const int64_t mid = (rec[j - 1].cut + c) / 2;  // non-negative: floor
            if (mid > lo) {
                lo = mid;
                flags |= REFINE_CLIPPED;
            }
        }
        if (j + 1 == n) {
            hi = hi < d.S ? hi : d.S;
        } else {
            const int64_t mid = (c + rec[j + 1].cut) / 2;
            if (mid < hi) {
                hi = mid;
                flags |= REFINE_CLIPPED;
            }
        }
        rec[j].lo = lo;
        rec[j].hi = hi;
        rec[j].t1 = rec[j].t2 = 0;
        rec[j].coarse_score = rec[j].refined_score = 0.0;
        rec[j].flags = flags;
        rec[j].reserved = 0;
    }
    unsigned long long* words = (unsigned long long*)rec;
    constexpr int RW = (int)(sizeof(BreakRefine) / 8);
    for (int64_t q = (int64_t)n * RW + t; q < out_stride * RW; q += REFINE_TABLE_THREADS) words[q] = 0ull;
    // popcount of the whole reference
    unsigned long long pop = 0;
    const int64_t nw = (d.R + 31) >> 5;
    for (int64_t g = t; g < nw; g += REFINE_TABLE_THREADS) pop += __popc(split_word(d.r, d.R, g));
    for (int s = 32; s >= 1; s >>= 1) pop += __shfl_xor(pop, s, 64);
    if (lane == 0) s_pop[wave] = pop;
    __syncthreads();
    if (t == 0) {
        unsigned long long p1 = 0;
        for (int w = 0; w < NW; ++w) p1 += s_pop[w];
        const double rbar = ((double)(d.R - (int64_t)p1) * d.r0 + (double)(int64_t)p1 * d.r1) / (double)d.R;
        const double bz = beta == beta ? beta : 0.0;  // NaN (single cut): the null score is never read
        d.pair_ws[0] = d.s0 * rbar + bz * fabs(d.s0);
        d.pair_ws[1] = d.s1 * rbar + bz * fabs(d.s1);
        d.pair_ws[2] = rbar;
        n_breaks_out[d.out_row] = n;
    }
}

// (value, first index) prefix maximum: the right operand wins only when strictly larger
FFS_DEV void refine_pmax(double& v, int& i, double rv, int ri) {
    if (rv > v) {
        v = rv;
        i = ri;
    }
}

// one workgroup per (pair, break slot): t1, t2, the coarse and refined scores, the edge / unmatched flags
__global__ void __launch_bounds__(REFINE_THREADS) k_refine_cut(const RefineDesc* __restrict__ desc, int n_slots,
                                                               int64_t out_stride, bool single,
                                                               const int32_t* __restrict__ n_breaks,
                                                               BreakRefine* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int NW = REFINE_THREADS / 64;
    __shared__ int32_t s_wsum[NW][REFINE_NC];
    __shared__ double s_wv[NW];
    __shared__ int s_wi[NW], s_wj[NW];
    __shared__ double s_coarse;
    const int jb = blockIdx.x % n_slots;
    const int slot = blockIdx.x / n_slots;
    const RefineDesc d = desc[slot];
    if (jb >= n_breaks[d.out_row]) return;  // (uniform)
    BreakRefine* rec = out + d.out_row * out_stride + jb;
    const int64_t L = rec->lo, U = rec->hi, c = rec->cut, oa = rec->offset_prev, ob = rec->offset_next;
    const double z0 = d.pair_ws[0], z1 = d.pair_ws[1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // words [gL, gU] hold the samples t in [L, U]; thread t owns [w0, w1)
    const int64_t gL = L >> 5, gU = U >> 5;
    const int64_t per = (gU - gL + 1 + REFINE_THREADS - 1) / REFINE_THREADS;
    const int64_t w0 = gL + t * per, w1 = (w0 + per < gU + 1) ? w0 + per : gU + 1;
    uint32_t m[REFINE_NC];
    // pass 1: the thread's sums, exclusive workgroup scan
    int32_t run[REFINE_NC], tot[REFINE_NC];
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) run[x] = 0;
    for (int64_t g = w0; g < w1; ++g) {
        refine_masks(d, g, L, U, oa, ob, m);
#pragma unroll
        for (int x = 0; x < REFINE_NC; ++x) run[x] += __popc(m[x]);
    }
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) {
        const int32_t own = run[x];
        int32_t inc = own;
        for (int s = 1; s < 64; s <<= 1) {
            const int32_t up = __shfl_up(inc, s, 64);
            if (lane >= s) inc += up;
        }
        if (lane == 63) s_wsum[wave][x] = inc;
        run[x] = inc - own;
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < REFINE_NC; ++x) {
        int32_t before = 0, all = 0;
        for (int w = 0; w < NW; ++w) {
            before += w < wave ? s_wsum[w][x] : 0;
            all += s_wsum[w][x];
        }
        run[x] += before;
        tot[x] = all;
    }
    // every sample t in [L, U] of the thread's words, in order, with its counts over [L, t)
    auto walk = [&](auto&& visit) {
        int32_t cur[REFINE_NC];
#pragma unroll
        for (int x = 0; x < REFINE_NC; ++x) cur[x] = run[x];
        for (int64_t g = w0; g < w1; ++g) {
            refine_masks(d, g, L, U, oa, ob, m);
            for (int k = 0; k < 32; ++k) {
                const int64_t ts = g * 32 + k;
                if (ts < L || ts > U) continue;
                const uint32_t low = (1u << k) - 1u;
                int32_t p[REFINE_NC];
#pragma unroll
                for (int x = 0; x < REFINE_NC; ++x) p[x] = cur[x] + __popc(m[x] & low);
                const double A = refine_mix(d, p[0], p[1], p[2], p[3]);
                const double Bv = refine_mix(d, tot[4] - p[4], tot[5] - p[5], tot[6] - p[6], tot[7] - p[7]);
                const int32_t n1 = p[8], n0 = (int32_t)(ts - L) - n1;
                const double N = (double)n0 * z0 + (double)n1 * z1;
                visit((int)ts, A, Bv, N);
            }
#pragma unroll
            for (int x = 0; x < REFINE_NC; ++x) cur[x] += __popc(m[x]);
        }
    };
    // pass 2 (two cuts): the prefix maximum of F entering the thread's samples
    double mv = -INFINITY;
    int mi = INT_MAX;
    if (!single) {
        walk([&](int ts, double A, double Bv, double N) { refine_pmax(mv, mi, A - N, ts); });
        for (int s = 1; s < 64; s <<= 1) {  // inclusive scan, earlier lanes on the left
            const double uv = __shfl_up(mv, s, 64);
            const int ui = __shfl_up(mi, s, 64);
            if (lane >= s) {
                double lv = uv;
                int li = ui;
                refine_pmax(lv, li, mv, mi);
                mv = lv;
                mi = li;
            }
        }
        if (lane == 63) {
            s_wv[wave] = mv;
            s_wi[wave] = mi;
        }
        double ev = __shfl_up(mv, 1, 64);  // exclusive within the wave
        int ei = __shfl_up(mi, 1, 64);
        if (lane == 0) {
            ev = -INFINITY;
            ei = INT_MAX;
        }
        __syncthreads();
        double pv = -INFINITY;
        int pi = INT_MAX;
        for (int w = 0; w < wave; ++w) refine_pmax(pv, pi, s_wv[w], s_wi[w]);
        refine_pmax(pv, pi, ev, ei);
        mv = pv;
        mi = pi;
        __syncthreads();  // s_wv / s_wi are reused below
    }
    // pass 3: the objective at every t, the thread's first maximiser
    double hv = -INFINITY;
    int h2 = INT_MAX, h1 = INT_MAX;
    walk([&](int ts, double A, double Bv, double N) {
        double h;
        int i1;
        if (single) {
            h = A + Bv;
            i1 = ts;
        } else {
            refine_pmax(mv, mi, A - N, ts);
            h = (N + Bv) + mv;
            i1 = mi;
        }
        if (h > hv) {
            hv = h;
            h2 = ts;
            h1 = i1;
        }
        if (ts == c) s_coarse = A + Bv;
    });
    // workgroup argmax, smallest t2 on ties
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(hv, s, 64);
        const int o2 = __shfl_xor(h2, s, 64), o1 = __shfl_xor(h1, s, 64);
        if (ov > hv || (ov == hv && o2 < h2)) {
            hv = ov;
            h2 = o2;
            h1 = o1;
        }
    }
    if (lane == 0) {
        s_wv[wave] = hv;
        s_wi[wave] = h2;
        s_wj[wave] = h1;
    }
    __syncthreads();
    if (t == 0) {
        double v = s_wv[0];
        int i2 = s_wi[0], i1 = s_wj[0];
        for (int w = 1; w < NW; ++w) {
            if (s_wv[w] > v || (s_wv[w] == v && s_wi[w] < i2)) {
                v = s_wv[w];
                i2 = s_wi[w];
                i1 = s_wj[w];
            }
        }
        int32_t flags = rec->flags;
        if ((i1 == L && L > 0) || (i2 == U && U < d.S)) flags |= REFINE_AT_EDGE;
        if (i1 < i2) flags |= REFINE_UNMATCHED;
        rec->t1 = i1;
        rec->t2 = i2;
        rec->coarse_score = s_coarse;
        rec->refined_score = v;
        rec->flags = flags;
    }
}

}  // namespace ffsa
