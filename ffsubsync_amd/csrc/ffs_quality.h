// ffs_quality.h -- alignment quality report: runner-up peaks, mean and spread of the whole correlation curve over the
// lag window (gfx950).  Upstream's only quality signal is the raw score at the winning lag (--min-score,
// ffsubsync.py:145-174), whose magnitude grows with the file's length and speech density; the normalised statistics
// derived from this report (peak-to-sidelobe ratio, runner-up margin) do not.  The contract is this library's own,
// pinned against the numpy model tests/quality_model.py.
//
// Problem (per pair): two-level reference r (R samples) and ONE subtitle vector s (S samples), both FFS_DTYPE_U1, and
// the lag window [d_lo, d_hi] of the reference's masked `convolve` array (aligners.py:31-48, negative-slice case
// included; windowless = all N entries).  Subtitle sample i meets reference sample i+d; samples outside the vectors are
// absent.  Score of lag d: two_level_score() of the counts (n11, n1x, nx1) over the overlap -- the arithmetic of the
// solve's records, so peak 1 equals ffs_pair_result bit for bit -- and exactly 0.0 where the overlap is empty.
//
// Two kernels per sub-batch of pairs (after k_split_prefix has written the word prefix popcounts of both vectors):
//   k_quality_counts  n11 of every lag of the window's overlap range (-S, R) as uint32 in the workspace curve.  A
//                     workgroup takes one 4096-lag tile and one chunk of subtitle words: it stages the chunk and the
//                     reference window it meets in LDS; thread q holds the 32 lags 32q..32q+31 of the tile, whose
//                     reference word at subtitle word w is a funnel shift (v_alignbit) of the two staged words q+w,
//                     q+w+1 by the lag's bit offset -- one LDS read per 32 lag-word steps -- and each step is a v_bcnt
//                     accumulate.  Chunks are combined with integer atomicAdd (exact, order-independent), after an LDS
//                     transpose so that each wave's adds cover 64 consecutive lags.
//   k_quality_peaks   one workgroup per pair: scores of every lag into the workspace, their sum / min / max, the mean,
//                     the centred sum of squares (second pass over the stored scores), then top_k rounds of a block
//                     argmax over the lags at least E away from every earlier peak (largest lag on ties).  The moments
//                     and the peak rounds are the device helpers quality_curve_moments / quality_curve_peaks, which the
//                     split report (ffs_split_report.h) shares.
#pragma once
#include "ffs_kernels.h"
#include "ffs_split.h"

namespace ffsa {

constexpr int QUAL_CNT_THREADS = 128;                  // k_quality_counts workgroup: one thread per 32 lags
constexpr int QUAL_TILE = QUAL_CNT_THREADS * 32;       // lags per workgroup
constexpr int QUAL_MAX_CHUNK = 1024;                   // subtitle words per workgroup (at most)
constexpr int QUAL_PEAK_THREADS = 1024;                // k_quality_peaks workgroup (one per pair)
constexpr int QUAL_MAX_PEAKS = 8;
constexpr int32_t QUAL_FLAT = 1;                       // FFS_QUALITY_FLAT
constexpr int32_t QUAL_EMPTY_WINDOW = 2;               // FFS_QUALITY_EMPTY_WINDOW

struct QualDesc {
    const uint32_t* r;  // reference bits
    const uint32_t* s;  // subtitle bits
    int64_t R, S;
    int64_t d_lo, n_lags;   // the window: lags d_lo .. d_lo + n_lags - 1 (lag index j = d - d_lo)
    int64_t c_lo, n_count;  // lags with a non-empty overlap: c_lo .. c_lo + n_count - 1 (n_count may be 0)
    CandDesc cd;            // R, S and the mapped levels s0, s1, r0, r1 for two_level_score
    const int32_t* pre_r;   // workspace: exclusive word prefix popcounts of r (all R samples) and of s
    const int32_t* pre_s;
    uint32_t* curve;        // workspace: n11 at lag index j (zeroed before k_quality_counts)
    double* sc;             // workspace: the score of lag index j
    int64_t out_row;        // pair index in the caller's output records
};

struct QualResult {  // = ffs_quality_result
    double peak_score[QUAL_MAX_PEAKS];
    int64_t peak_offset[QUAL_MAX_PEAKS];
    double mean, std;
    int64_t n_lags;
    int32_t n_peaks, flags;
};
static_assert(sizeof(QualResult) == 160, "QualResult must match ffs_quality_result");

// n11 of a 4096-lag tile over one chunk of subtitle words; grid.x = pairs * n_tiles * n_chunks
__global__ void __launch_bounds__(QUAL_CNT_THREADS) k_quality_counts(const QualDesc* __restrict__ desc, int n_tiles,
                                                                     int n_chunks, int chunk_words) {
    __shared__ uint32_t s_sub[QUAL_MAX_CHUNK];
    __shared__ uint32_t s_ref[QUAL_MAX_CHUNK + QUAL_CNT_THREADS + 1];
    __shared__ uint32_t s_acc[QUAL_CNT_THREADS * 33];  // [q][sh], rows padded to 33 words against bank conflicts
    const int tile = blockIdx.x % n_tiles;
    const int chunk = (blockIdx.x / n_tiles) % n_chunks;
    const int slot = blockIdx.x / (n_tiles * n_chunks);
    const QualDesc d = desc[slot];
    const int64_t l0 = (int64_t)tile * QUAL_TILE;  // first lag of the tile, relative to c_lo
    const int64_t g0 = (int64_t)chunk * chunk_words;
    const int64_t sw_total = (d.S + 31) >> 5;
    if (l0 >= d.n_count || g0 >= sw_total) return;  // (uniform)
    const int nw = (int)(g0 + chunk_words < sw_total ? chunk_words : sw_total - g0);
    // reference bits [base + 32 q, +32) for q <= nw + QUAL_CNT_THREADS meet subtitle word g0 + w at tile lag 32 q' + sh
    const int64_t base = 32 * g0 + d.c_lo + l0;
    if (base + 32 * (int64_t)(nw + QUAL_CNT_THREADS + 1) <= 0 || base >= d.R) return;  // no reference sample reachable
    const int64_t gbase = base >= 0 ? (base >> 5) : -((31 - base) >> 5);  // floor(base / 32)
    const int bsh = (int)(base - gbase * 32);
    const int t = threadIdx.x;
    for (int q = t; q <= nw + QUAL_CNT_THREADS; q += QUAL_CNT_THREADS) {
        const uint32_t lo = split_word(d.r, d.R, gbase + q), hi = split_word(d.r, d.R, gbase + q + 1);
        s_ref[q] = __builtin_amdgcn_alignbit(hi, lo, bsh);
    }
    for (int w = t; w < nw; w += QUAL_CNT_THREADS) s_sub[w] = split_word(d.s, d.S, g0 + w);
    __syncthreads();
    uint32_t acc[32];
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) acc[sh] = 0;
    uint32_t lo = s_ref[t];
    for (int w = 0; w < nw; ++w) {
        const uint32_t sw = s_sub[w];  // (one address per wave: broadcast)
        const uint32_t hi = s_ref[t + w + 1];
#pragma unroll
        for (int sh = 0; sh < 32; ++sh) acc[sh] += __popc(__builtin_amdgcn_alignbit(hi, lo, sh) & sw);
        lo = hi;
    }
#pragma unroll
    for (int sh = 0; sh < 32; ++sh) s_acc[t * 33 + sh] = acc[sh];
    __syncthreads();
    uint32_t* out = d.curve + (d.c_lo - d.d_lo) + l0;
    const int64_t n_here = d.n_count - l0 < QUAL_TILE ? d.n_count - l0 : QUAL_TILE;
    for (int l = t; l < n_here; l += QUAL_CNT_THREADS) {
        const uint32_t v = s_acc[(l >> 5) * 33 + (l & 31)];
        if (v) atomicAdd(out + l, v);
    }
}

// the score of lag index j: exactly 0.0 without overlap, else two_level_score of the counts
FFS_DEV double quality_score(const QualDesc& d, int64_t j) {
    const int64_t lag = d.d_lo + j;
    const int64_t i0 = lag < 0 ? -lag : 0;
    const int64_t i1 = d.R - lag < d.S ? d.R - lag : d.S;
    if (i1 <= i0) return 0.0;
    const int n11 = (int)d.curve[j];
    const int n1x = split_prefix_at(d.pre_s, d.s, i1) - split_prefix_at(d.pre_s, d.s, i0);
    const int nx1 = split_prefix_at(d.pre_r, d.r, i1 + lag) - split_prefix_at(d.pre_r, d.r, i0 + lag);
    return two_level_score(d.cd, n11, n1x, nx1, (int)lag);
}

// (value, lag index) maximum with the largest index on ties; index -1 = nothing yet
FFS_DEV void quality_max_pair(double& v, int64_t& j, double ov, int64_t oj) {
    if (oj >= 0 && (j < 0 || ov > v || (ov == v && oj > j))) {
        v = ov;
        j = oj;
    }
}

// fixed-order block sum of one double per thread (the result is the same on every run)
FFS_DEV double quality_block_sum(double x, double* s_part) {
#pragma clang fp contract(off)
    constexpr int NW = QUAL_PEAK_THREADS / 64;
    for (int s = 32; s >= 1; s >>= 1) x += __shfl_xor(x, s, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    double sum = s_part[0];
    for (int w = 1; w < NW; ++w) sum += s_part[w];
    return sum;
}

// min / max / fixed-order sum of the n scores first(j), then the centred sum of squares over again(j) (the same
// scores, recomputed or read back): mean, population std and whether the curve is flat (every score equal: mean = that
// score, std = 0).  Every thread of the workgroup calls it; the result is the same on every thread and every run.
template <class F1, class F2>
FFS_DEV void quality_curve_moments(int64_t n, F1 first, F2 again, double& mean, double& sd, bool& flat) {
#pragma clang fp contract(off)
    constexpr int NW = QUAL_PEAK_THREADS / 64;
    __shared__ double s_part[NW];
    __shared__ double s_mn[NW], s_mx[NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double sum = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t j = t; j < n; j += QUAL_PEAK_THREADS) {
        const double v = first(j);
        sum += v;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, s, 64));
        mx = fmax(mx, __shfl_xor(mx, s, 64));
    }
    if (lane == 0) {
        s_mn[wave] = mn;
        s_mx[wave] = mx;
    }
    const double total = quality_block_sum(sum, s_part);  // (its barriers publish s_mn / s_mx)
    for (int w = 0; w < NW; ++w) {
        mn = fmin(mn, s_mn[w]);
        mx = fmax(mx, s_mx[w]);
    }
    flat = mn == mx;
    mean = flat ? mx : total / (double)n;
    double ss = 0.0;
    if (!flat) {
        for (int64_t j = t; j < n; j += QUAL_PEAK_THREADS) {
            const double e = again(j) - mean;
            ss += e * e;
        }
    }
    const double css = quality_block_sum(ss, s_part);
    sd = flat ? 0.0 : sqrt(css / (double)n);
}

// up to top_k greedy peaks of the n scores score(j): each round a block argmax (largest lag index on ties) over the lags
// at least `exclusion` from every earlier peak.  Peak k's lag index and score land in s_peak[k] / s_pscore[k] (LDS);
// returns the number of peaks (the same on every thread).
template <class F>
FFS_DEV int quality_curve_peaks(int64_t n, F score, int top_k, int64_t exclusion, int64_t* s_peak, double* s_pscore) {
    constexpr int NW = QUAL_PEAK_THREADS / 64;
    __shared__ double s_v[NW];
    __shared__ int64_t s_j[NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int n_peaks = 0;
    for (int k = 0; k < top_k; ++k) {
        double best = -INFINITY;
        int64_t bestj = -1;
        for (int64_t j = t; j < n; j += QUAL_PEAK_THREADS) {
            bool ok = true;
            for (int p = 0; p < k; ++p) {
                const int64_t dist = j - s_peak[p];
                ok = ok && (dist >= exclusion || -dist >= exclusion);
            }
            if (ok) quality_max_pair(best, bestj, score(j), j);
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const double ov = __shfl_xor(best, s, 64);
            const int64_t oj = __shfl_xor(bestj, s, 64);
            quality_max_pair(best, bestj, ov, oj);
        }
        if (lane == 0) {
            s_v[wave] = best;
            s_j[wave] = bestj;
        }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < NW; ++w) quality_max_pair(best, bestj, s_v[w], s_j[w]);
            s_peak[k] = bestj;
            s_pscore[k] = best;
        }
        __syncthreads();
        if (s_peak[k] < 0) break;  // (uniform) no lag left outside the exclusion zones
        n_peaks = k + 1;
    }
    return n_peaks;
}

// one workgroup per pair: scores, moments and greedy peaks into the pair's ffs_quality_result
__global__ void __launch_bounds__(QUAL_PEAK_THREADS) k_quality_peaks(const QualDesc* __restrict__ desc, int top_k,
                                                                     int64_t exclusion, QualResult* __restrict__ out) {
    __shared__ int64_t s_peak[QUAL_MAX_PEAKS];
    __shared__ double s_pscore[QUAL_MAX_PEAKS];
    const QualDesc d = desc[blockIdx.x];
    const int t = threadIdx.x;
    const int64_t n = d.n_lags;
    QualResult* rec = out + d.out_row;
    if (n <= 0) {  // (uniform) the reference's window is empty: no lag, no peak
        if (t < QUAL_MAX_PEAKS) {
            rec->peak_score[t] = 0.0;
            rec->peak_offset[t] = 0;
        }
        if (t == 0) {
            rec->mean = 0.0;
            rec->std = 0.0;
            rec->n_lags = 0;
            rec->n_peaks = 0;
            rec->flags = QUAL_FLAT | QUAL_EMPTY_WINDOW;
        }
        return;
    }
    double mean, sd;
    bool flat;
    quality_curve_moments(
        n,
        [&](int64_t j) {
            const double v = quality_score(d, j);
            d.sc[j] = v;  // (read back below by this same thread only)
            return v;
        },
        [&](int64_t j) { return d.sc[j]; }, mean, sd, flat);
    const int n_peaks = quality_curve_peaks(n, [&](int64_t j) { return d.sc[j]; }, top_k, exclusion, s_peak, s_pscore);
    if (t == 0) {
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
