// ffs_cue_report.h -- per-cue evidence report after any sync (gfx950).  Every sync ends in cue times; this says, cue
// by cue, how well the lag the sync applied fits the cue's own neighbourhood, which lag within a radius fits best, and
// whether the reference has any speech under the cue at all.  The contract is this library's own,
// pinned against the numpy model tests/cue_model.py, bit for bit.
//
// Per pair: two-level reference r (R samples), subtitle s (S samples).  Per cue (start, end, lag; any int64):
// a = clamp(start, 0, S), e = clamp(end, 0, S); e <= a: CUE_EMPTY; |lag| > 2^31: CUE_INVALID (the record holds start,
// end, lag and the flag, everything else zero).  Otherwise the window is L = max(0, a - m), U = min(S, e + m)
// (m = context) and for every delta in [-rho, rho] (rho = radius), d = lag + delta:
//     window counts (ov, n11, n1x, nx1) over subtitle samples i in [L, U) whose partner i + d lies in [0, R)
//     c(delta) = refine_mix of them (fp64, every operation rounded on its own)
//     cue counts cov(delta), c11(delta) = the partners inside the reference and the reference ones over i in [a, e)
// best_delta maximises c, cue_max_delta maximises c11; ties go to the smallest |delta|, then to +delta over -delta;
// n_best = the number of delta with c(delta) equal to the maximum.
//
// One kernel, one wave per cue (a 64-thread workgroup per cue, so the workgroup barrier orders the wave's own LDS
// traffic and nothing else); the grid is flat over all cues of the sub-batch.  The lanes hold the lags: round q gives
// lane l delta = -rho + 64 q + l, ceil((2 rho + 1) / 64) rounds.  Per round the wave walks the window's subtitle words
// slice by slice (CUE_SLICE words): the reference words the slice can meet at the round's 64 lags (CUE_SLICE + 3 of
// them) are staged in LDS, the subtitle word is uniform across the wave, and per (lane lag, word) the reference word
// at that bit shift is one v_alignbit of two staged words; presence comes from range masks; six v_bcnt accumulate the
// four window counts and the two cue counts.  Each lane keeps its own best under the tie rule as its lags ascend; the
// two argmaxes and n_best are xor-butterfly wave reductions; lane 0 stores the record.
#pragma once
#include "ffs_kernels.h"
#include "ffs_split.h"
#include "ffs_split_refine.h"

namespace ffsa {

constexpr int CUE_THREADS = 64;             // one wave per cue
constexpr int CUE_SLICE = 256;              // window words per staged slice
constexpr int CUE_STAGE = CUE_SLICE + 4;    // reference words staged per slice (CUE_SLICE + 3 are read)
constexpr int64_t CUE_MAX_RADIUS = 4096;    // FFS_CUE_MAX_RADIUS
constexpr int64_t CUE_MAX_CONTEXT = 65536;  // FFS_CUE_MAX_CONTEXT
constexpr int64_t CUE_MAX_LAG = (int64_t)1 << 31;
constexpr int32_t CUE_EMPTY = 1;            // FFS_CUE_EMPTY
constexpr int32_t CUE_INVALID = 2;          // FFS_CUE_INVALID
constexpr int32_t CUE_NO_OVERLAP = 4;       // FFS_CUE_NO_OVERLAP
constexpr int32_t CUE_BEST_AT_EDGE = 8;     // FFS_CUE_BEST_AT_EDGE
constexpr int32_t CUE_FLAT = 16;            // FFS_CUE_FLAT
constexpr int32_t CUE_SILENT = 32;          // FFS_CUE_SILENT

struct CueDesc {
    RefineDesc v;         // the vectors and weights (pair_ws unused, out_row = the pair)
    int64_t cue_first;    // the pair's first entry of the cue table
    int64_t grid_first;   // the pair's first workgroup of the sub-batch's grid
    int64_t cue_count;
};

struct Cue {  // = ffs_cue
    int64_t start, end, lag;
};
static_assert(sizeof(Cue) == 24, "Cue must match ffs_cue");

struct CueReport {  // = ffs_cue_report
    int64_t start, end, lo, hi, lag;
    int32_t own[4];   // ov, n11, n1x, nx1 at delta = 0
    int32_t best[4];  // the same at best_delta
    double own_score, best_score;
    int32_t best_delta, n_best;
    int32_t cue_own_n11, cue_own_ov, cue_max_n11, cue_max_delta;
    int32_t flags, reserved;
};
static_assert(sizeof(CueReport) == 120, "CueReport must match ffs_cue_report");

// 3.10's option order: the smaller |delta| first, then +delta over -delta
FFS_DEV bool cue_delta_before(int32_t x, int32_t y) {
    const int32_t ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
    return ax < ay || (ax == ay && x > y);
}

__global__ void __launch_bounds__(CUE_THREADS) k_cue_report(const CueDesc* __restrict__ desc, int n_desc,
                                                            const Cue* __restrict__ cues, int radius, int context,
                                                            CueReport* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ uint32_t s_ref[CUE_STAGE];
    // the pair of this workgroup: the last descriptor with grid_first <= blockIdx.x (uniform)
    int lo_d = 0, hi_d = n_desc - 1;
    while (lo_d < hi_d) {
        const int mid = (lo_d + hi_d + 1) >> 1;
        if (desc[mid].grid_first <= (int64_t)blockIdx.x)
            lo_d = mid;
        else
            hi_d = mid - 1;
    }
    const CueDesc cd = desc[lo_d];
    const RefineDesc& d = cd.v;
    const int64_t entry = cd.cue_first + ((int64_t)blockIdx.x - cd.grid_first);
    const Cue cue = cues[entry];
    CueReport* rec = out + entry;
    const int lane = threadIdx.x;

    const int64_t a = cue.start < 0 ? 0 : (cue.start > d.S ? d.S : cue.start);
    const int64_t e = cue.end < 0 ? 0 : (cue.end > d.S ? d.S : cue.end);
    int32_t flags = 0;
    if (e <= a) flags |= CUE_EMPTY;
    if (cue.lag > CUE_MAX_LAG || cue.lag < -CUE_MAX_LAG) flags |= CUE_INVALID;
    if (flags) {  // (uniform)
        if (lane == 0) {
            CueReport z = {};
            z.start = cue.start;
            z.end = cue.end;
            z.lag = cue.lag;
            z.flags = flags;
            *rec = z;
        }
        return;
    }
    const int64_t L = a - context > 0 ? a - context : 0;
    const int64_t U = e + context < d.S ? e + context : d.S;
    const int64_t gL = L >> 5, gU = (U + 31) >> 5;  // the window's words [gL, gU)
    const int n_delta = 2 * radius + 1;
    const int n_rounds = (n_delta + 63) >> 6;

    // the lane's best under the tie rule, its count of maxima, and the counts at delta = 0
    double bs = -INFINITY;
    int32_t bd = 0, nb = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    int32_t ms = -1, md = 0;  // cue_max_n11, cue_max_delta
    double own_s = 0.0;
    int32_t o0 = 0, o1 = 0, o2 = 0, o3 = 0, oc11 = 0, ocov = 0;

    for (int q = 0; q < n_rounds; ++q) {
        const int idx = q * 64 + lane;
        const bool live = idx < n_delta;
        const int32_t delta = -radius + (live ? idx : n_delta - 1);  // idle lanes repeat the last lag, unrecorded
        const int64_t dl = cue.lag + delta;                       // this lane's lag
        const int64_t d0 = cue.lag - radius + (int64_t)q * 64;    // lane 0's lag (uniform)
        // presence in the window and under the cue: partner i + dl in [0, R)
        const int64_t plo = -dl, phi = d.R - dl;
        const int64_t wlo = L > plo ? L : plo, whi = U < phi ? U : phi;
        const int64_t clo = a > plo ? a : plo, chi = e < phi ? e : phi;
        int32_t ov = 0, n11 = 0, n1x = 0, nx1 = 0, cov = 0, c11 = 0;
        for (int64_t g0 = gL; g0 < gU; g0 += CUE_SLICE) {
            const int64_t g1 = g0 + CUE_SLICE < gU ? g0 + CUE_SLICE : gU;
            // reference words [wb, wb + (g1 - g0) + 3) cover samples 32 g + dl + k of every lane
            const int64_t base0 = g0 * 32 + d0;
            const int64_t wb = base0 >= 0 ? (base0 >> 5) : -((31 - base0) >> 5);  // floor(base0 / 32)
            const int n_stage = (int)(g1 - g0) + 3;
            __syncthreads();  // the previous slice's reads are done
            for (int j = lane; j < n_stage; j += CUE_THREADS) s_ref[j] = split_word(d.r, d.R, wb + j);
            __syncthreads();
            for (int64_t g = g0; g < g1; ++g) {
                const uint32_t win = refine_range_mask(g, L, U);
                const uint32_t sw = split_word(d.s, d.S, g) & win;  // (uniform)
                const int64_t base = g * 32 + dl;
                const int64_t gb = base >= 0 ? (base >> 5) : -((31 - base) >> 5);
                const int sh = (int)(base - gb * 32);
                const int j = (int)(gb - wb);  // in [0, n_stage - 2]
                const uint32_t rw = __builtin_amdgcn_alignbit(s_ref[j + 1], s_ref[j], sh) & win;
                const uint32_t pres = refine_range_mask(g, wlo, whi);
                const uint32_t cmask = refine_range_mask(g, a, e);
                ov += __popc(pres);
                n11 += __popc(sw & rw);
                n1x += __popc(sw & pres);
                nx1 += __popc(rw);
                cov += __popc(refine_range_mask(g, clo, chi));
                c11 += __popc(rw & cmask);
            }
        }
        const double c = refine_mix(d, ov, n11, n1x, nx1);
        if (live) {
            if (c > bs || (c == bs && cue_delta_before(delta, bd))) {
                nb = c > bs ? 1 : nb + 1;
                bs = c;
                bd = delta;
                b0 = ov;
                b1 = n11;
                b2 = n1x;
                b3 = nx1;
            } else if (c == bs) {
                ++nb;
            }
            if (c11 > ms || (c11 == ms && cue_delta_before(delta, md))) {
                ms = c11;
                md = delta;
            }
            if (delta == 0) {
                own_s = c;
                o0 = ov;
                o1 = n11;
                o2 = n1x;
                o3 = nx1;
                oc11 = c11;
                ocov = cov;
            }
        }
    }
    // wave reductions: (score, delta, count, counts) and (cue n11, delta)
    for (int s = 32; s >= 1; s >>= 1) {
        const double xs = __shfl_xor(bs, s, 64);
        const int32_t xd = __shfl_xor(bd, s, 64), xn = __shfl_xor(nb, s, 64);
        const int32_t x0 = __shfl_xor(b0, s, 64), x1 = __shfl_xor(b1, s, 64), x2 = __shfl_xor(b2, s, 64),
                      x3 = __shfl_xor(b3, s, 64);
        if (xn > 0 && (nb == 0 || xs > bs || (xs == bs && cue_delta_before(xd, bd)))) {
            nb = (nb > 0 && xs == bs) ? nb + xn : xn;
            bs = xs;
            bd = xd;
            b0 = x0;
            b1 = x1;
            b2 = x2;
            b3 = x3;
        } else if (xn > 0 && xs == bs) {
            nb += xn;
        }
        const int32_t ys = __shfl_xor(ms, s, 64), yd = __shfl_xor(md, s, 64);
        if (ys > ms || (ys == ms && ys >= 0 && cue_delta_before(yd, md))) {
            ms = ys;
            md = yd;
        }
    }
    // delta = 0 sits at index rho: lane rho & 63 (of round rho >> 6)
    const int src = radius & 63;
    own_s = __shfl(own_s, src, 64);
    o0 = __shfl(o0, src, 64);
    o1 = __shfl(o1, src, 64);
    o2 = __shfl(o2, src, 64);
    o3 = __shfl(o3, src, 64);
    oc11 = __shfl(oc11, src, 64);
    ocov = __shfl(ocov, src, 64);
    if (lane == 0) {
        if (o0 == 0) flags |= CUE_NO_OVERLAP;
        if (radius > 0 && (bd == radius || bd == -radius)) flags |= CUE_BEST_AT_EDGE;
        if (radius > 0 && nb == n_delta) flags |= CUE_FLAT;
        if (ms == 0) flags |= CUE_SILENT;
        CueReport z;
        z.start = cue.start;
        z.end = cue.end;
        z.lo = L;
        z.hi = U;
        z.lag = cue.lag;
        z.own[0] = o0;
        z.own[1] = o1;
        z.own[2] = o2;
        z.own[3] = o3;
        z.best[0] = b0;
        z.best[1] = b1;
        z.best[2] = b2;
        z.best[3] = b3;
        z.own_score = own_s;
        z.best_score = bs;
        z.best_delta = bd;
        z.n_best = nb;
        z.cue_own_n11 = oc11;
        z.cue_own_ov = ocov;
        z.cue_max_n11 = ms;
        z.cue_max_delta = md;
        z.flags = flags;
        z.reserved = 0;
        *rec = z;
    }
}

}  // namespace ffsa
