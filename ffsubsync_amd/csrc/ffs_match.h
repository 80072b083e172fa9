// ffs_match.h -- all-pairs quality report from boundary lists: the n11 curve of a pair over its whole lag window from the
// two run-boundary lists, no pass over the samples (gfx950).  The report itself (scores, moments, greedy peaks) is
// k_quality_peaks of ffs_quality.h, fed the same QualDesc it takes from ffs_align_quality_batch: only the producer of the
// uint32 n11 curve differs, so the records are byte-identical to that call's.
//
// Per vector, once per call (amortised over every partner of the vector in an N x M call): its bits in the plan's
// workspace (k_runs_expand over a table of vectors, one launch) and their word prefix popcounts (k_split_prefix, two
// vectors per descriptor) -- what quality_score() derives n1x / nx1 from, and what the `bits` fallback counts on.
//
// Per pair: k_runs_curve, one workgroup per (pair, tile of MATCH_TILE lags).  With P the subtitle's boundary list, Q the
// reference's, D0 the tile's first lag (the arithmetic of oracle/runs_model.py::window_counts):
//   n11(D0) = -sum_p db[p] * ones of rho in front of p + D0      one lower-bound search per subtitle boundary into the
//   g(D0)   = -sum_p db[p] * rho[p + D0 - 1]                     staged reference positions (parity of the lower bound)
//   h(d)    = sum over (p, q) with q - p = d of db[p] * drho[q]  LDS integer adds, 32-bit cells (see below)
//   g(d+1) = g(d) - h(d),  n11(d+1) = n11(d) + g(d+1)            two block-wide running sums
// Every tile searches its own n11(D0) and g(D0): nothing is carried over from a neighbouring workgroup, a workgroup owns
// its tile's cells and its slice of the curve, so there is no device-scope atomic and no zeroing of the curve.  Outside
// the overlap range the same sums give 0 (the signs of an even-length list cancel), which is what the curve must hold
// there; a tile that no overlapping lag falls into writes zeros without reading a list.
//
// Cell width: 32 bits.  A cell holds h(d) of one lag, |h| <= min(|P|, |Q|): two identical alternating vectors of n
// boundaries reach +n at lag 0 and -(n - 1) at lags +-1.  Plan-owned lists stop at 32 766 boundaries, where +32 766 fits
// a signed 16-bit cell by ONE count, but a caller-owned list may be longer (any n < cap), and two 16-bit cells packed
// into a word (k_runs_corr's layout) borrow from each other on a negative sum and must be unpacked with the carry undone.
// 4096 lags x 4 B = 16 KiB per workgroup leaves three workgroups per CU beside the 32 KiB of staged positions, so the
// width that is exact for every list costs no occupancy that the staging does not already.
//
// Staging: MATCH_QCAP reference positions at a time (lists of subtitle-like 2 h vectors, ~2000 entries, fit whole;
// longer ones go slice by slice).  A slice holds entries [k0, k0 + cnt] -- one entry of the next slice, or the sentinel
// -- and a subtitle boundary is OWNED by the slice its global lower bound falls into (local lower bound in [1, cnt], or
// 0 in the first slice): that slice adds its n11(D0) / g(D0) terms; every slice adds the coincidences with its own
// entries.  The search is a fixed-step branchless lower bound (the same trip count on every lane).
#pragma once
#include "ffs_quality.h"
#include "ffs_runs.h"

// FFS_MATCH_AUTO: a pair goes through its lists while |P| * |Q| * FFS_MATCH_AUTO_COST <= R * S / 32, i.e. while its
// coincidences per lag, each weighed as FFS_MATCH_AUTO_COST word-lag steps of k_quality_counts, stay below the bit path's
// S / 32 steps per lag (the break-even measured over the boundary densities 1x .. 16x)
#ifndef FFS_MATCH_AUTO_COST
#define FFS_MATCH_AUTO_COST 64.0
#endif

namespace ffsa {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_LPT = 16;                           // consecutive lags per thread in the scans
constexpr int MATCH_TILE = MATCH_THREADS * MATCH_LPT;   // lags per workgroup
constexpr int MATCH_QCAP = 8192;                        // reference positions staged at a time (even: parity = global parity)
constexpr int MATCH_QSENT = 0x3fffffff;                 // beyond every position and every p + D0 (vectors are shorter than 2^29)
static_assert(MATCH_QCAP % 2 == 0 && MATCH_LPT % 4 == 0, "slice parity, 16-byte cell reads");

struct MatchLists {  // pair slot's boundary lists, beside its QualDesc
    const int2* eq;  // reference entries (position, ones in front)
    const int2* ep;  // subtitle entries
    int32_t nq, np;  // boundaries (even, < capacity: checked by the entry point)
    int32_t ones_q;  // ones of the reference
    int32_t pad;
};

struct MatchHdr {  // the 16-byte header of an ffs_runs_list block
    int32_t n, ones, len, cap;
};

// the headers of a table of list blocks, gathered for the host's checks (the only device work in front of them)
__global__ void k_match_headers(const int2* const* __restrict__ blocks, int n, MatchHdr* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int2 a = blocks[i][0], b = blocks[i][1];
    out[i] = MatchHdr{a.x, a.y, b.x, b.y};
}

// exclusive block scan of one value per thread (wrapping 32-bit sums); s_w: MATCH_THREADS / 64 words
FFS_DEV uint32_t match_block_excl_scan(uint32_t v, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(inc, s, 64);
        if (lane >= s) inc += o;
    }
    __syncthreads();  // (s_w may still be read from the previous scan)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += s_w[w];
    return base + inc - v;
}

// n11 of every lag of one MATCH_TILE tile of the window from the two boundary lists; grid.x = pairs * n_tiles
__global__ void __launch_bounds__(MATCH_THREADS) k_runs_curve(const QualDesc* __restrict__ desc,
                                                              const MatchLists* __restrict__ lists, int n_tiles) {
    __shared__ int s_h[MATCH_TILE];
    __shared__ int s_q[MATCH_QCAP + 1];
    __shared__ uint32_t s_w[MATCH_THREADS / 64];
    __shared__ uint32_t s_red[2 * (MATCH_THREADS / 64)];
    const int slot = blockIdx.x / n_tiles, tile = blockIdx.x - slot * n_tiles;
    const QualDesc d = desc[slot];
    const int64_t j0 = (int64_t)tile * MATCH_TILE;
    if (j0 >= d.n_lags) return;  // (uniform)
    const int nt = (int)(d.n_lags - j0 < MATCH_TILE ? d.n_lags - j0 : MATCH_TILE);
    uint32_t* out = d.curve + j0;
    const int64_t D0w = d.d_lo + j0;  // the tile's first lag
    const int t = threadIdx.x;
    if (d.n_count <= 0 || D0w + nt - 1 < d.c_lo || D0w >= d.c_lo + d.n_count) {  // (uniform) no lag with an overlap
        for (int l = t; l < nt; l += MATCH_THREADS) out[l] = 0u;
        return;
    }
    const int D0 = (int)D0w;  // in (-S - MATCH_TILE, R): p + D0 fits 32 bits with room
    const MatchLists ls = lists[slot];
    const GEntries Q = (GEntries)ls.eq, P = (GEntries)ls.ep;
    const int nq = ls.nq, np = ls.np;
    for (int l = t; l < MATCH_TILE; l += MATCH_THREADS) s_h[l] = 0;
    uint32_t a_n11 = 0, a_g = 0;
    for (int k0 = 0; k0 == 0 || k0 < nq; k0 += MATCH_QCAP) {
        const int cnt = nq - k0 < MATCH_QCAP ? nq - k0 : MATCH_QCAP;
        __syncthreads();  // the cells are zeroed / the previous slice has been read
        for (int i = t; i <= cnt; i += MATCH_THREADS) s_q[i] = k0 + i < nq ? Q[k0 + i].pos : MATCH_QSENT;
        __syncthreads();
        for (int k = t; k < np; k += MATCH_THREADS) {
            const int x = P[k].pos + D0;
            const int sp = (k & 1) ? -1 : 1;
            int lo = 0, len = cnt + 1;  // first i in [0, cnt + 1] with s_q[i] >= x
            while (len > 1) {           // (uniform trip count)
                const int half = len >> 1;
                lo += s_q[lo + half - 1] < x ? half : 0;
                len -= half;
            }
            lo += s_q[lo] < x ? 1 : 0;
            if (lo <= cnt && (lo > 0 || k0 == 0)) {  // this slice owns p: lb is the global lower bound
                const int lb = k0 + lo;
                int ones = lb < nq ? Q[lb].ones : ls.ones_q;
                if (lb & 1) ones -= s_q[lo] - x;  // inside a run
                a_n11 -= (uint32_t)(sp * ones);
                a_g -= (uint32_t)(sp * (lb & 1));
            }
            for (int j = lo; j < cnt; ++j) {
                const int dd = s_q[j] - x;  // >= 0 in a sorted list (compared unsigned: a broken one cannot leave the cells)
                if ((unsigned)dd >= (unsigned)nt) break;
                atomicAdd(&s_h[dd], (j & 1) ? -sp : sp);
            }
        }
    }
    // block sums of the two start values
    const int lane = t & 63, wave = t >> 6;
    for (int s = 32; s >= 1; s >>= 1) {
        a_n11 += __shfl_xor(a_n11, s, 64);
        a_g += __shfl_xor(a_g, s, 64);
    }
    if (lane == 0) {
        s_red[wave] = a_n11;
        s_red[MATCH_THREADS / 64 + wave] = a_g;
    }
    __syncthreads();  // (also: every cell add has landed)
    uint32_t n11_0 = 0, g_0 = 0;
    for (int w = 0; w < MATCH_THREADS / 64; ++w) {
        n11_0 += s_red[w];
        g_0 += s_red[MATCH_THREADS / 64 + w];
    }
    // thread t: lags t * LPT .. + LPT - 1 of the tile.  g[l] = g_0 - sum_{m < l} h[m];  n11[l] = n11_0 - g_0 + sum_{m <= l} g[m]
    uint32_t g[MATCH_LPT];
    uint32_t hs = 0;
#pragma unroll
    for (int i = 0; i < MATCH_LPT; i += 4) {
        const int4 v = *reinterpret_cast<const int4*>(&s_h[t * MATCH_LPT + i]);
        g[i] = (uint32_t)v.x;
        g[i + 1] = (uint32_t)v.y;
        g[i + 2] = (uint32_t)v.z;
        g[i + 3] = (uint32_t)v.w;
        hs += g[i] + g[i + 1] + g[i + 2] + g[i + 3];
    }
    uint32_t run = g_0 - match_block_excl_scan(hs, s_w);
    uint32_t gs = 0;
#pragma unroll
    for (int i = 0; i < MATCH_LPT; ++i) {
        const uint32_t h = g[i];
        g[i] = run;
        gs += run;
        run -= h;
    }
    uint32_t acc = n11_0 - g_0 + match_block_excl_scan(gs, s_w);
#pragma unroll
    for (int i = 0; i < MATCH_LPT; ++i) {
        acc += g[i];
        g[i] = acc;
    }
    const int l0 = t * MATCH_LPT;
    if (l0 + MATCH_LPT <= nt && ((uintptr_t)(out + l0) & 15) == 0) {
#pragma unroll
        for (int i = 0; i < MATCH_LPT; i += 4)
            *reinterpret_cast<uint4*>(out + l0 + i) = make_uint4(g[i], g[i + 1], g[i + 2], g[i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < MATCH_LPT; ++i)
            if (l0 + i < nt) out[l0 + i] = g[i];
    }
}

}  // namespace ffsa
