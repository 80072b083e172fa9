// ffs_sweep.h -- peaks and moments of ratio profiles (gfx950): the reduction behind ffsubsync_amd/ratio_sweep.py.
//
// A ratio sweep solves every file at ~10^3 speed factors and keeps the solve records (ffs_cand_result, 24 bytes a
// point) in HBM as a [file][grid point] table.  What the host needs of a file's profile is its few best grid points and
// how far they stand above the rest, so one call reduces the table to one fixed-size record per file instead of reading
// 24 bytes a point back.  Contract (include/ffsubsync_amd.h, ffs_sweep_peaks), pinned against tests/sweep_model.py:
//   - a point is skipped when its score is not finite or its flags carry FFS_FLAG_EMPTY_WINDOW
//   - peak 1 = the largest score among the points not skipped (smaller index on ties); peak k+1 = the same over the
//     indices at least `exclusion` from every earlier peak
//   - mean and population std over the points not skipped, two passes, fixed summation order; all equal -> std = 0
//
// k_sweep_peaks: one 256-thread workgroup per file, strided over its points (the records are read from global memory in
// every pass; a profile is a few tens of KB and stays in L2).  Per pass a cross-lane reduction per wave, then LDS
// across the four waves; one pass for the sum / min / max, one for the centred squares, one per peak.  Records are read,
// never written.
#pragma once
#include "ffs_kernels.h"

namespace ffsa {

constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_WAVES = SWEEP_THREADS / 64;
constexpr int SWEEP_MAX_PEAKS = 8;
constexpr int32_t SWEEP_FLAT = 1;       // FFS_SWEEP_FLAT
constexpr int32_t SWEEP_EMPTY = 2;      // FFS_SWEEP_EMPTY
constexpr int32_t SWEEP_AMBIGUOUS = 4;  // FFS_SWEEP_AMBIGUOUS
constexpr int32_t SWEEP_REC_EMPTY_WINDOW = 1;  // FFS_FLAG_EMPTY_WINDOW
constexpr int32_t SWEEP_REC_AMBIGUOUS = 2;     // FFS_FLAG_AMBIGUOUS

struct SweepProfile {  // = ffs_sweep_profile
    double peak_score[SWEEP_MAX_PEAKS];
    int64_t peak_offset[SWEEP_MAX_PEAKS];
    int64_t peak_index[SWEEP_MAX_PEAKS];
    double mean, std;
    int64_t n_points, n_skipped;
    int32_t n_peaks, flags;
};
static_assert(sizeof(SweepProfile) == 232, "SweepProfile must match ffs_sweep_profile");

FFS_DEV bool sweep_skipped(const CandResult& r) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(r.score);
    const bool finite = (bits & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
    return !finite || (r.flags & SWEEP_REC_EMPTY_WINDOW) != 0;
}

// (value, index) maximum with the smaller index on ties; index -1 = nothing yet
FFS_DEV void sweep_max_pair(double& v, int64_t& j, double ov, int64_t oj) {
    if (oj >= 0 && (j < 0 || ov > v || (ov == v && oj < j))) {
        v = ov;
        j = oj;
    }
}

// fixed-order workgroup sum of one double per thread (the same on every thread and every run)
FFS_DEV double sweep_block_sum(double x, double* s_part) {
#pragma clang fp contract(off)
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    double sum = s_part[0];
    for (int w = 1; w < SWEEP_WAVES; ++w) sum += s_part[w];
    return sum;
}

__global__ void __launch_bounds__(SWEEP_THREADS) k_sweep_peaks(const CandResult* __restrict__ rec,
                                                               const int64_t* __restrict__ first, int top_k,
                                                               int64_t exclusion, SweepProfile* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_part[SWEEP_WAVES];
    __shared__ double s_mn[SWEEP_WAVES], s_mx[SWEEP_WAVES];
    __shared__ long long s_cnt[SWEEP_WAVES];
    __shared__ int s_amb[SWEEP_WAVES];
    __shared__ double s_v[SWEEP_WAVES];
    __shared__ int64_t s_j[SWEEP_WAVES];
    __shared__ int64_t s_peak[SWEEP_MAX_PEAKS];
    __shared__ double s_pscore[SWEEP_MAX_PEAKS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t f0 = first[blockIdx.x];
    const int64_t n = first[blockIdx.x + 1] > f0 ? first[blockIdx.x + 1] - f0 : 0;
    const CandResult* r = rec + f0;
    SweepProfile* p = out + blockIdx.x;

    // pass 1: count, sum, min and max of the points not skipped; any AMBIGUOUS record
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    long long cnt = 0;
    int amb = 0;
    for (int64_t j = t; j < n; j += SWEEP_THREADS) {
        const CandResult c = r[j];
        amb |= (c.flags & SWEEP_REC_AMBIGUOUS) != 0;
        if (sweep_skipped(c)) continue;
        sum += c.score;
        mn = fmin(mn, c.score);
        mx = fmax(mx, c.score);
        ++cnt;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, s, 64));
        mx = fmax(mx, __shfl_xor(mx, s, 64));
        cnt += __shfl_xor(cnt, s, 64);
        amb |= __shfl_xor(amb, s, 64);
    }
    if (lane == 0) {
        s_mn[wave] = mn;
        s_mx[wave] = mx;
        s_cnt[wave] = cnt;
        s_amb[wave] = amb;
    }
    const double total = sweep_block_sum(sum, s_part);  // (its barriers publish the four arrays above)
    cnt = 0;
    amb = 0;
    for (int w = 0; w < SWEEP_WAVES; ++w) {
        mn = fmin(mn, s_mn[w]);
        mx = fmax(mx, s_mx[w]);
        cnt += s_cnt[w];
        amb |= s_amb[w];
    }
    const bool flat = cnt == 0 || mn == mx;
    const double mean = cnt == 0 ? 0.0 : (flat ? mx : total / (double)cnt);

    // pass 2: the centred sum of squares
    double ss = 0.0;
    if (!flat) {
        for (int64_t j = t; j < n; j += SWEEP_THREADS) {
            const CandResult c = r[j];
            if (sweep_skipped(c)) continue;
            const double e = c.score - mean;
            ss += e * e;
        }
    }
    const double css = sweep_block_sum(ss, s_part);
    const double sd = flat ? 0.0 : sqrt(css / (double)cnt);

    // one pass per peak: workgroup argmax over the indices at least `exclusion` from every earlier peak
    int n_peaks = 0;
    for (int k = 0; k < top_k; ++k) {
        double best = -INFINITY;
        int64_t bestj = -1;
        for (int64_t j = t; j < n; j += SWEEP_THREADS) {
            bool ok = true;
            for (int q = 0; q < k; ++q) {
                const int64_t dist = j - s_peak[q];
                ok = ok && (dist >= exclusion || -dist >= exclusion);
            }
            if (!ok) continue;
            const CandResult c = r[j];
            if (!sweep_skipped(c)) sweep_max_pair(best, bestj, c.score, j);
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const double ov = __shfl_xor(best, s, 64);
            const int64_t oj = __shfl_xor(bestj, s, 64);
            sweep_max_pair(best, bestj, ov, oj);
        }
        if (lane == 0) {
            s_v[wave] = best;
            s_j[wave] = bestj;
        }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < SWEEP_WAVES; ++w) sweep_max_pair(best, bestj, s_v[w], s_j[w]);
            s_peak[k] = bestj;
            s_pscore[k] = best;
        }
        __syncthreads();
        if (s_peak[k] < 0) break;  // (uniform) no point left outside the exclusion zones
        n_peaks = k + 1;
    }
    if (t < SWEEP_MAX_PEAKS) {
        const bool has = t < n_peaks;
        p->peak_score[t] = has ? s_pscore[t] : 0.0;
        p->peak_index[t] = has ? s_peak[t] : 0;
        p->peak_offset[t] = has ? (int64_t)r[s_peak[t]].offset : 0;
    }
    if (t == 0) {
        p->mean = mean;
        p->std = sd;
        p->n_points = n;
        p->n_skipped = n - cnt;
        p->n_peaks = n_peaks;
        p->flags = (flat ? SWEEP_FLAT : 0) | (cnt == 0 ? SWEEP_EMPTY : 0) | (amb ? SWEEP_AMBIGUOUS : 0);
    }
}

}  // namespace ffsa
