// ffs_cue_retime.h -- joint cue retiming after any sync (gfx950): one residual shift per cue, chosen jointly by a
// Viterbi pass over (cue x residual lag), so that the cues' own neighbourhoods fit, consecutive cues do not move apart
// without evidence, and the cues stay in order.  The contract is this library's own, pinned against the
// numpy model tests/retime_model.py bit for bit, and against the enumeration of every path (tests/retime_reference.py).
//
// Everything is exact integer arithmetic.  Per pair: two-level reference r (R samples), subtitle s (S samples) and the
// pair's cues (start, end, lag; any int64) in table order = chain order.  Live and skipped cues, the window [L, U) and
// the counts at d = lag + delta are ffs_cue_report.h's.  The node score is the INTEGER agreement
//     A_k(delta) = ov - 2 n1x - 2 nx1 + 4 n11 = n00 - n01 - n10 + n11
// -- 3.18's c(delta) at levels (0,1)/(0,1).  THE PAIR'S LEVELS DO NOT ENTER THE RETIME: a max-plus recurrence over a
// thousand fp64 sums cannot be pinned against an independent optimum, integers can.  In 64ths: u_k = 64 A_k.
// Link from live cue k-1 (shift d') to live cue k (shift d): w = penalty_q |d - d'|, capped at jump_q when jump_q >= 0;
// g_k = (a_k + lag_k) - (a_{k-1} + lag_{k-1}); with KEEP_ORDER and g_k >= 0 only d' <= d + g_k is admissible.
//     V_1(d) = u_1(d),   V_k(d) = u_k(d) + max over admissible d' of (V_{k-1}(d') - w(d', d))      (int64)
// Every tie (backpointer, final argmax) goes to 3.10's option order on the candidate: smallest |.|, then + over -.
//
// Two kernels.  k_retime_profile: k_cue_report's word-lag loop, storing A_k(delta) for every delta instead of reducing
// (lanes = lags, staged reference words in LDS, one v_alignbit per (lane lag, word)); one wave per (cue, round of 64
// lags), the grid flat over both.  The bit shift and the word offset of a lane do not depend on the word, the presence
// mask is two 32-bit clamps, and A = ov - 2 popc((s ^ r) & present): two v_bcnt per (lane lag, word).
// k_retime_dp: one workgroup per pair, forward over the live cues; V stays in registers (RETIME_EPT lags per thread),
// three (value, shift) arrays in LDS carry the step's maxima: the prefix max of V + q d' (left of d), the prefix max of
// V (the jump), and a doubling table of V - q d' whose level floor(log2 g) answers the window (d, d + g] with two
// overlapping reads (g = 2 rho when order is off or the gap is wide: a suffix).  Backpointers go out as int16; then one
// lane backtracks and the waves fill the records.  No atomics, no cross-workgroup traffic.
#pragma once
#include "ffs_cue_report.h"

namespace ffsa {

constexpr int RETIME_PROFILE_THREADS = 64;   // one wave per (cue, round of 64 lags)
constexpr int RETIME_DP_THREADS = 1024;      // one workgroup per pair
constexpr int RETIME_DP_WAVES = RETIME_DP_THREADS / 64;
constexpr int64_t RETIME_MAX_RADIUS = 1024;  // FFS_RETIME_MAX_RADIUS
constexpr int RETIME_MAX_D = 2 * (int)RETIME_MAX_RADIUS + 1;
constexpr int RETIME_EPT = (RETIME_MAX_D + RETIME_DP_THREADS - 1) / RETIME_DP_THREADS;  // lags per thread: 3
constexpr int64_t RETIME_Q = 64;             // FFS_RETIME_Q: costs are in 64ths of a score sample
constexpr int64_t RETIME_MAX_PENALTY_Q = (int64_t)1 << 20;
constexpr int64_t RETIME_MAX_JUMP_Q = (int64_t)1 << 40;
constexpr int64_t RETIME_NO_JUMP = -1;       // FFS_RETIME_NO_JUMP
constexpr int64_t RETIME_WORK_CAP = (int64_t)256 << 20;  // FFS_RETIME_WORK_CAP: workspace of one sub-batch
constexpr int64_t RETIME_CELL_BYTES = 6;     // int32 profile + int16 backpointer per (cue, delta)
constexpr int32_t RETIME_KEEP_ORDER = 1;     // FFS_RETIME_KEEP_ORDER (call flag)
constexpr int32_t RETIME_EMPTY = 1;          // FFS_RETIME_EMPTY
constexpr int32_t RETIME_INVALID = 2;        // FFS_RETIME_INVALID
constexpr int32_t RETIME_MOVED = 4;          // FFS_RETIME_MOVED
constexpr int32_t RETIME_JUMP = 8;           // FFS_RETIME_JUMP
constexpr int32_t RETIME_UNORDERED = 16;     // FFS_RETIME_UNORDERED
constexpr int32_t RETIME_ORDER_TIGHT = 32;   // FFS_RETIME_ORDER_TIGHT
constexpr int32_t RETIME_AT_EDGE = 64;       // FFS_RETIME_AT_EDGE

struct RetimeDesc {
    const uint32_t* r;    // reference bits (FFS_DTYPE_U1)
    const uint32_t* s;    // subtitle bits
    int64_t R, S;
    int64_t cue_first;    // the pair's first entry of the cue table
    int64_t cue_count;
    int64_t grid_first;   // the pair's first workgroup of the sub-batch's profile grid
    int64_t ws_first;     // the pair's first row of the sub-batch's workspace (one row of D cells per cue)
    int64_t out_row;      // pair index in the caller's summaries
};

struct RetimeRec {  // = ffs_cue_retime
    int64_t start, end, lag;
    int32_t delta, flags;
    int32_t own, at, best, best_delta;
    int64_t link;
    int32_t reserved[2];
};
static_assert(sizeof(RetimeRec) == 64, "RetimeRec must match ffs_cue_retime");

struct RetimeSummary {  // = ffs_retime_summary
    int64_t total, own_total, best_total;
    int32_t n_live, n_moved, n_jumps, reserved;
};
static_assert(sizeof(RetimeSummary) == 40, "RetimeSummary must match ffs_retime_summary");

// the clamped cue [a, e) and its skip flags (RETIME_EMPTY / RETIME_INVALID = CUE_EMPTY / CUE_INVALID)
FFS_DEV int32_t retime_cue_span(const Cue& cue, int64_t S, int64_t& a, int64_t& e) {
    a = cue.start < 0 ? 0 : (cue.start > S ? S : cue.start);
    e = cue.end < 0 ? 0 : (cue.end > S ? S : cue.end);
    int32_t flags = 0;
    if (e <= a) flags |= RETIME_EMPTY;
    if (cue.lag > CUE_MAX_LAG || cue.lag < -CUE_MAX_LAG) flags |= RETIME_INVALID;
    return flags;
}

FFS_DEV uint32_t retime_low_mask(int32_t n) { return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }  // bits [0, n), n >= 0

FFS_DEV int32_t retime_clamp32(int32_t x) { return x < 0 ? 0 : (x > 32 ? 32 : x); }

// (value, shift) under the lexicographic maximum: the larger value, then 3.10's option order on the shift
FFS_DEV bool retime_better(int64_t av, int32_t ad, int64_t bv, int32_t bd) {
    return av > bv || (av == bv && cue_delta_before(ad, bd));
}

__global__ void __launch_bounds__(RETIME_PROFILE_THREADS)
k_retime_profile(const RetimeDesc* __restrict__ desc, int n_desc, const Cue* __restrict__ cues, int radius, int context,
                 int n_rounds, int32_t* __restrict__ prof) {
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
    const RetimeDesc d = desc[lo_d];
    const int64_t b = (int64_t)blockIdx.x - d.grid_first;
    const int64_t k = b / n_rounds;
    const int q = (int)(b - k * n_rounds);
    if (k >= d.cue_count) return;  // (uniform; the host's grid holds no such workgroup)
    const Cue cue = cues[d.cue_first + k];
    const int lane = threadIdx.x;
    int64_t a, e;
    if (retime_cue_span(cue, d.S, a, e)) return;  // skipped cues write nothing (uniform)
    const int64_t L = a - context > 0 ? a - context : 0;
    const int64_t U = e + context < d.S ? e + context : d.S;
    const int64_t gL = L >> 5, gU = (U + 31) >> 5;  // the window's words [gL, gU)
    const int n_delta = 2 * radius + 1;
    const int idx = q * 64 + lane;
    const bool live = idx < n_delta;
    const int32_t delta = -radius + (live ? idx : n_delta - 1);  // idle lanes repeat the last lag, unrecorded
    const int64_t dl = cue.lag + delta;                          // this lane's lag
    const int64_t d0 = cue.lag - radius + (int64_t)q * 64;       // lane 0's lag (uniform)
    // present samples [wlo, whi) inside [L, U]: in the window with the partner i + dl in [0, R); relative to word gL
    int64_t wlo = L > -dl ? L : -dl, whi = U < d.R - dl ? U : d.R - dl;
    if (wlo > U) wlo = U;
    if (whi < wlo) whi = wlo;
    const int32_t rl = (int32_t)(wlo - gL * 32), rh = (int32_t)(whi - gL * 32);  // in [0, 2^30 + 32)
    // 32 g + dl = 32 (g + floor(dl / 32)) + sh: neither the bit shift nor the word offset depends on the word
    const int64_t fdl = dl >> 5, fd0 = d0 >> 5;
    const int sh = (int)(dl - fdl * 32);
    const int joff = (int)(fdl - fd0);  // 0, 1 or 2
    int32_t ov = 0, nx = 0;
    for (int64_t g0 = gL; g0 < gU; g0 += CUE_SLICE) {
        const int64_t g1 = g0 + CUE_SLICE < gU ? g0 + CUE_SLICE : gU;
        const int64_t wb = g0 + fd0;  // reference words [wb, wb + (g1 - g0) + 3) cover every lane's samples
        const int n_stage = (int)(g1 - g0) + 3;
        __syncthreads();  // the previous slice's reads are done
        for (int j = lane; j < n_stage; j += RETIME_PROFILE_THREADS) s_ref[j] = split_word(d.r, d.R, wb + j);
        __syncthreads();
        const int n_words = (int)(g1 - g0);
        int32_t t = (int32_t)(g0 - gL) * 32;
        for (int w = 0; w < n_words; ++w, t += 32) {
            const uint32_t sw = split_word(d.s, d.S, g0 + w);  // (uniform)
            const int j = w + joff;                            // in [0, n_stage - 2]
            const uint32_t rw = __builtin_amdgcn_alignbit(s_ref[j + 1], s_ref[j], sh);
            const uint32_t pres = retime_low_mask(retime_clamp32(rh - t)) & ~retime_low_mask(retime_clamp32(rl - t));
            ov += __popc(pres);
            nx += __popc((sw ^ rw) & pres);
        }
    }
    if (live) prof[(d.ws_first + k) * n_delta + idx] = ov - 2 * nx;
}

__global__ void __launch_bounds__(RETIME_DP_THREADS)
k_retime_dp(const RetimeDesc* __restrict__ desc, const Cue* __restrict__ cues, int radius, int64_t penalty_q,
            int64_t jump_q, int call_flags, const int32_t* __restrict__ prof, int16_t* __restrict__ bp,
            RetimeRec* __restrict__ out, RetimeSummary* __restrict__ summary) {
    __shared__ int64_t s_val[3][RETIME_MAX_D + 3];  // 0: prefix max of V + q d'; 1: prefix max of V; 2: windows of V - q d'
    __shared__ int16_t s_arg[3][RETIME_MAX_D + 3];
    __shared__ int64_t s_red_v[RETIME_DP_WAVES], s_red_own[RETIME_DP_WAVES], s_red_best[RETIME_DP_WAVES];
    __shared__ int32_t s_red_d[RETIME_DP_WAVES], s_red_n[RETIME_DP_WAVES];
    const RetimeDesc d = desc[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int D = 2 * radius + 1;
    const bool keep = (call_flags & RETIME_KEEP_ORDER) != 0, jumps = jump_q >= 0;
    int64_t V[RETIME_EPT];
    for (int x = 0; x < RETIME_EPT; ++x) V[x] = 0;
    int64_t prev_pos = 0, first_live = -1, last_live = -1;

    for (int64_t k = 0; k < d.cue_count; ++k) {  // everything about the cue is uniform
        const int64_t entry = d.cue_first + k;
        const Cue cue = cues[entry];
        int64_t a, e;
        const int32_t skip = retime_cue_span(cue, d.S, a, e);
        if (skip) {
            if (t == 0) {
                RetimeRec z = {};
                z.start = cue.start;
                z.end = cue.end;
                z.lag = cue.lag;
                z.flags = skip;
                out[entry] = z;
            }
            continue;
        }
        const int64_t cell0 = (d.ws_first + k) * D;
        const int64_t pos = a + cue.lag;
        const int64_t g = pos - prev_pos;
        prev_pos = pos;
        last_live = k;
        if (first_live < 0) {
            first_live = k;
            for (int x = 0; x < RETIME_EPT; ++x) {
                const int i = t + x * RETIME_DP_THREADS;
                if (i < D) V[x] = RETIME_Q * (int64_t)prof[cell0 + i];
            }
            if (t == 0) {
                out[entry].start = cue.start;
                out[entry].end = cue.end;
                out[entry].lag = cue.lag;
                out[entry].flags = 0;
                out[entry].link = 0;
            }
            continue;
        }
        const bool order = keep && g >= 0;
        const int geff = order && g < 2 * radius ? (int)g : 2 * radius;  // admissible shifts right of d: (d, d + geff]
        const int jw = geff >= 1 ? 31 - __clz(geff) : 0;                 // the window's level: 2^jw <= geff < 2^(jw+1)
        int64_t v0[RETIME_EPT], v1[RETIME_EPT], v2[RETIME_EPT];
        int32_t a0[RETIME_EPT], a1[RETIME_EPT], a2[RETIME_EPT];
        __syncthreads();  // the previous step's reads of the arrays are done
        for (int x = 0; x < RETIME_EPT; ++x) {
            const int i = t + x * RETIME_DP_THREADS;
            v0[x] = v1[x] = v2[x] = 0;
            a0[x] = a1[x] = a2[x] = 0;
            if (i < D) {
                const int32_t dd = i - radius;
                v0[x] = V[x] + penalty_q * dd;
                v1[x] = V[x];
                v2[x] = V[x] - penalty_q * dd;
                a0[x] = a1[x] = a2[x] = dd;
                s_val[0][i] = v0[x];
                s_val[1][i] = v1[x];
                s_val[2][i] = v2[x];
                s_arg[0][i] = s_arg[1][i] = s_arg[2][i] = (int16_t)dd;
            }
        }
        __syncthreads();
        for (int j = 0; (1 << j) < D; ++j) {  // (jw < ceil(log2 D): the prefix passes cover the window's levels)
            const int off = 1 << j;
            const bool win = geff >= 1 && j < jw;
            int64_t n0[RETIME_EPT], n1[RETIME_EPT], n2[RETIME_EPT];
            int32_t m0[RETIME_EPT], m1[RETIME_EPT], m2[RETIME_EPT];
            bool hl[RETIME_EPT], hr[RETIME_EPT];
            for (int x = 0; x < RETIME_EPT; ++x) {
                const int i = t + x * RETIME_DP_THREADS;
                hl[x] = i < D && i - off >= 0;
                hr[x] = win && i + off < D;
                n0[x] = n1[x] = n2[x] = 0;
                m0[x] = m1[x] = m2[x] = 0;
                if (hl[x]) {
                    n0[x] = s_val[0][i - off];
                    m0[x] = s_arg[0][i - off];
                    if (jumps) {
                        n1[x] = s_val[1][i - off];
                        m1[x] = s_arg[1][i - off];
                    }
                }
                if (hr[x]) {
                    n2[x] = s_val[2][i + off];
                    m2[x] = s_arg[2][i + off];
                }
            }
            __syncthreads();
            for (int x = 0; x < RETIME_EPT; ++x) {
                const int i = t + x * RETIME_DP_THREADS;
                if (hl[x]) {
                    if (retime_better(n0[x], m0[x], v0[x], a0[x])) {
                        v0[x] = n0[x];
                        a0[x] = m0[x];
                        s_val[0][i] = v0[x];
                        s_arg[0][i] = (int16_t)a0[x];
                    }
                    if (jumps && retime_better(n1[x], m1[x], v1[x], a1[x])) {
                        v1[x] = n1[x];
                        a1[x] = m1[x];
                        s_val[1][i] = v1[x];
                        s_arg[1][i] = (int16_t)a1[x];
                    }
                }
                if (hr[x] && retime_better(n2[x], m2[x], v2[x], a2[x])) {
                    v2[x] = n2[x];
                    a2[x] = m2[x];
                    s_val[2][i] = v2[x];
                    s_arg[2][i] = (int16_t)a2[x];
                }
            }
            __syncthreads();
        }
        for (int x = 0; x < RETIME_EPT; ++x) {
            const int i = t + x * RETIME_DP_THREADS;
            if (i >= D) continue;
            const int32_t dd = i - radius;
            int64_t bv = v0[x] - penalty_q * dd;  // left: d' <= d
            int32_t ba = a0[x];
            if (geff >= 1 && i + 1 < D) {  // right: d < d' <= min(rho, d + geff), two overlapping windows of 2^jw
                const int64_t cv = s_val[2][i + 1] + penalty_q * dd;
                const int32_t ca = s_arg[2][i + 1];
                if (retime_better(cv, ca, bv, ba)) {
                    bv = cv;
                    ba = ca;
                }
                const int i2 = i + geff - (1 << jw) + 1;
                if (i2 < D) {
                    const int64_t ev = s_val[2][i2] + penalty_q * dd;
                    const int32_t ea = s_arg[2][i2];
                    if (retime_better(ev, ea, bv, ba)) {
                        bv = ev;
                        ba = ea;
                    }
                }
            }
            if (jumps) {  // any admissible d' at the capped cost
                const int ip = i + geff < D - 1 ? i + geff : D - 1;
                const int64_t cv = s_val[1][ip] - jump_q;
                const int32_t ca = s_arg[1][ip];
                if (retime_better(cv, ca, bv, ba)) {
                    bv = cv;
                    ba = ca;
                }
            }
            V[x] = RETIME_Q * (int64_t)prof[cell0 + i] + bv;
            bp[cell0 + i] = (int16_t)ba;
        }
        if (t == 0) {
            out[entry].start = cue.start;
            out[entry].end = cue.end;
            out[entry].lag = cue.lag;
            out[entry].flags = keep && g < 0 ? RETIME_UNORDERED : 0;
            out[entry].link = g;  // kept here for the backtrack, which replaces it
        }
    }

    if (first_live < 0) {  // no live cue (uniform)
        if (t == 0) summary[d.out_row] = RetimeSummary{};
        return;
    }
    // delta_K = argmax V_K under the option order
    int64_t bv = 0;
    int32_t bd = 0;
    bool have = false;
    for (int x = 0; x < RETIME_EPT; ++x) {
        const int i = t + x * RETIME_DP_THREADS;
        if (i < D && (!have || retime_better(V[x], i - radius, bv, bd))) {
            bv = V[x];
            bd = i - radius;
            have = true;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const int64_t xv = __shfl_xor(bv, s, 64);
        const int32_t xd = __shfl_xor(bd, s, 64);
        const bool xh = __shfl_xor((int)have, s, 64) != 0;
        if (xh && (!have || retime_better(xv, xd, bv, bd))) {
            bv = xv;
            bd = xd;
            have = true;
        }
    }
    if (lane == 0) {
        s_red_v[wave] = bv;
        s_red_d[wave] = bd;
        s_red_n[wave] = have ? 1 : 0;
    }
    __syncthreads();  // and every backpointer and record field stored above is visible to the workgroup

    int64_t total = 0;
    int32_t n_moved = 0, n_jumps = 0;
    if (t == 0) {  // the backtrack: delta, link and the flags of every live cue
        int32_t dcur = 0;
        have = false;
        for (int w = 0; w < RETIME_DP_WAVES; ++w)
            if (s_red_n[w] && (!have || retime_better(s_red_v[w], s_red_d[w], total, dcur))) {
                total = s_red_v[w];
                dcur = s_red_d[w];
                have = true;
            }
        for (int64_t k = last_live; k >= first_live; --k) {
            RetimeRec* rec = out + d.cue_first + k;
            int32_t fl = rec->flags;
            if (fl & (RETIME_EMPTY | RETIME_INVALID)) continue;
            int64_t link = 0;
            int32_t dprev = dcur;
            if (k != first_live) {
                const int64_t g = rec->link;
                dprev = bp[(d.ws_first + k) * D + dcur + radius];
                const int64_t lin = penalty_q * (int64_t)(dcur > dprev ? dcur - dprev : dprev - dcur);
                link = lin;
                if (jumps && lin > jump_q) {
                    link = jump_q;
                    fl |= RETIME_JUMP;
                    ++n_jumps;
                }
                if (keep && g >= 0 && (int64_t)dprev == (int64_t)dcur + g) fl |= RETIME_ORDER_TIGHT;
            }
            if (dcur != 0) {
                fl |= RETIME_MOVED;
                ++n_moved;
            }
            if (radius > 0 && (dcur == radius || dcur == -radius)) fl |= RETIME_AT_EDGE;
            rec->delta = dcur;
            rec->flags = fl;
            rec->link = link;
            dcur = dprev;
        }
    }
    __syncthreads();

    // one wave per cue: own, at, best and best_delta from the cue's profile row
    int64_t own_sum = 0, best_sum = 0;
    int32_t n_live = 0;
    for (int64_t k = first_live + wave; k <= last_live; k += RETIME_DP_WAVES) {
        const int64_t entry = d.cue_first + k;
        const Cue cue = cues[entry];
        int64_t a, e;
        if (retime_cue_span(cue, d.S, a, e)) continue;  // (uniform)
        const int32_t* row = prof + (d.ws_first + k) * D;
        int32_t ms = 0, md = 0;
        bool mh = false;
        for (int i = lane; i < D; i += 64) {  // the lane's shifts ascend: the option order decides equal scores
            const int32_t c = row[i], dd = i - radius;
            if (!mh || c > ms || (c == ms && cue_delta_before(dd, md))) {
                ms = c;
                md = dd;
                mh = true;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const int32_t xs = __shfl_xor(ms, s, 64), xd = __shfl_xor(md, s, 64);
            const bool xh = __shfl_xor((int)mh, s, 64) != 0;
            if (xh && (!mh || xs > ms || (xs == ms && cue_delta_before(xd, md)))) {
                ms = xs;
                md = xd;
                mh = true;
            }
        }
        const int32_t own = row[radius];
        if (lane == 0) {
            RetimeRec* rec = out + entry;
            rec->own = own;
            rec->at = row[rec->delta + radius];
            rec->best = ms;
            rec->best_delta = md;
            rec->reserved[0] = 0;
            rec->reserved[1] = 0;
        }
        own_sum += own;
        best_sum += ms;
        ++n_live;
    }
    if (lane == 0) {
        s_red_own[wave] = own_sum;
        s_red_best[wave] = best_sum;
        s_red_n[wave] = n_live;
    }
    __syncthreads();
    if (t == 0) {
        RetimeSummary z = {};
        z.total = total;
        for (int w = 0; w < RETIME_DP_WAVES; ++w) {
            z.own_total += RETIME_Q * s_red_own[w];
            z.best_total += RETIME_Q * s_red_best[w];
            z.n_live += s_red_n[w];
        }
        z.n_moved = n_moved;
        z.n_jumps = n_jumps;
        summary[d.out_row] = z;
    }
}

}  // namespace ffsa
