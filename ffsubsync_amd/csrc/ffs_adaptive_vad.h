// ffs_adaptive_vad.h -- adaptive energy VAD: frame levels, their histogram, a per-file threshold and the labels (gfx950):
// the device side of ffsubsync_amd/adaptive_vad.py.
//
// The fixed rule of k_vad_energy (speech <=> sum x^2 >= 10^(50/10) n) depends on the file's gain.  Here pass 1 reduces
// every frame to a LEVEL -- the number of edges of a caller-supplied ascending table that the frame's mean square
// reaches -- and the three small kernels behind it pick one threshold bin per file from the level counts and label the
// frames with it.  Contract (include/ffsubsync_amd.h, ffs_vad_levels / ffs_vad_level_hist / ffs_vad_pick_threshold /
// ffs_vad_level_labels), pinned bit for bit against tests/adaptive_vad_model.py:
//   level(f)  = #{k : (double)E_f >= edges[k] * (double)n_f}, E_f the exact 64-bit sum of squares, n_f the sample count
//   hist[b]   = #{f : level(f) == b}
//   pick      = Otsu's between-class variance over the bins >= lo_bin in exact integers and one fp64 multiply and
//               divide per candidate, or the noise floor (a quantile of the counted bins) plus a margin
//   speech(f) = level(f) >= threshold_bin
//
// k_vad_levels: k_vad_energy's sweep (a wave owns VAD_FPT = 8 frames, 16-byte nontemporal loads, squares8 / wave_total,
// vector path and element path -- the helpers are ffs_kernels.h's) with the one compare per frame replaced by up to
// four per lane: lane l holds edges[l], edges[l + 64], ... times frame_len (staged once per wave, +inf beyond n_edges;
// only the file's short last frame reads the table again), compares the wave-uniform E_f against them, and the level is the sum of
// the ballots' popcounts on the scalar unit.  The 8 level bytes of a task leave as one 8-byte store where the address
// allows and all 8 frames exist, else byte by byte from lanes 0..7.  No atomics; nothing is written behind the last frame.
//
// k_vad_level_hist: at most HIST_MAX_BLOCKS workgroups of 256 threads; a thread takes 16 level bytes per trip from the
// 16-byte aligned body (the unaligned head and the tail go byte by byte through workgroup 0), counts into a 256-bin
// LDS histogram with LDS atomics and the workgroup adds its non-zero bins below n_bins to the global one: at most
// HIST_MAX_BLOCKS * n_bins integer atomics per call (3072 for the default table), whatever the file's length.  Integer
// adds: the result does not depend on arrival order.  The host call zeroes the histogram on the stream first.
//
// k_vad_pick_threshold: one wave per histogram, lane l owns bins 4l .. 4l + 3.  Wave scans give the exclusive prefix
// counts and first moments, every lane scores its four candidate thresholds, a butterfly keeps the smallest t of the
// largest score.  Everything but v = (double)d * (double)d / (double)m and eta is integer arithmetic.
//
// k_vad_level_labels: a lane a frame; the threshold is read from device memory (a record's first field) or is a kernel
// argument.  fp32 labels are stored coalesced, the packed form is the wave's ballot, a byte from each of lanes 0..7.
#pragma once
#include "ffs_kernels.h"

namespace ffsa {

constexpr int VAD_MAX_EDGES = 255;      // FFS_VAD_MAX_EDGES
constexpr int VAD_MAX_BINS = 256;       // FFS_VAD_MAX_BINS
constexpr long long VAD_MAX_FRAMES = 1ll << 23;  // FFS_VAD_MAX_FRAMES: above it the pick falls back (TOO_LONG)
constexpr int VAD_RULE_OTSU = 0;        // FFS_VAD_RULE_OTSU
constexpr int VAD_RULE_FLOOR = 1;       // FFS_VAD_RULE_FLOOR
constexpr int32_t VAD_THR_FALLBACK = 1;     // FFS_VAD_THR_FALLBACK
constexpr int32_t VAD_THR_TOO_LONG = 2;     // FFS_VAD_THR_TOO_LONG
constexpr int32_t VAD_THR_EMPTY = 4;        // FFS_VAD_THR_EMPTY
constexpr int32_t VAD_THR_FLAT = 8;         // FFS_VAD_THR_FLAT
constexpr int32_t VAD_THR_CLAMPED_LO = 16;  // FFS_VAD_THR_CLAMPED_LO
constexpr int32_t VAD_THR_CLAMPED_HI = 32;  // FFS_VAD_THR_CLAMPED_HI
constexpr int HIST_THREADS = 256;
constexpr int HIST_MAX_BLOCKS = 16;     // workgroups of ffs_vad_level_hist, at most
constexpr int HIST_BYTES_PER_TRIP = HIST_THREADS * 16;  // level bytes a workgroup takes per trip
constexpr int LABEL_THREADS = 256;
constexpr int LABEL_MAX_BLOCKS = 2048;

struct VadThreshold {  // = ffs_vad_threshold
    int32_t threshold_bin, flags, floor_bin, top_bin;
    int64_t n_frames, n_counted, n_speech;
    double eta;
};
static_assert(sizeof(VadThreshold) == 48, "VadThreshold must match ffs_vad_threshold");

// number of the lane's (pre-multiplied) edges that e reaches, summed over the wave: wave-uniform
FFS_DEV unsigned level_of(unsigned long long e, const double (&thr)[4], int ngroups) {
    const double x = (double)e;
    unsigned level = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < ngroups) level += (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(x >= thr[j]));
    return level;
}

__global__ __launch_bounds__(256) void k_vad_levels(const int16_t* __restrict__ pcm, long long n_samples, int frame_len,
                                                    long long n_frames, const double* __restrict__ edges, int n_edges,
                                                    unsigned char* __restrict__ levels) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
    const long long nwaves = (long long)gridDim.x * (blockDim.x / 64);
    const long long n_tasks = (n_frames + VAD_FPT - 1) / VAD_FPT;
    const int nvec = frame_len / 8;
    const bool vec_ok = (frame_len % 8 == 0) && nvec <= 64 && ((reinterpret_cast<uintptr_t>(pcm) & 15) == 0);
    const int ngroups = (n_edges + 63) / 64;  // <= 4
    // the lane's edges times n; an edge beyond the table is +inf: never reached.  Whole frames use thr_full, staged once
    // per wave; the element path's short frame reads the table again (from cache) instead of holding it in registers
    auto stage = [&](double (&thr)[4], int n) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            thr[j] = (lane + 64 * j < n_edges ? edges[lane + 64 * j] : __builtin_huge_val()) * (double)n;
    };
    double thr_full[4];
    stage(thr_full, frame_len);
    for (long long t = wave0; t < n_tasks; t += nwaves) {
        const long long f0 = t * VAD_FPT;
        unsigned long long word = 0;  // byte i = level of frame f0 + i
#pragma unroll
        for (int g = 0; g < VAD_FPT; g += 4) {
            const long long fg = f0 + g;
            if (fg >= n_frames) break;
            if (vec_ok && (fg + 4) * frame_len <= n_samples) {  // four whole frames: wave-uniform fast path
                const vad_v4i* p = reinterpret_cast<const vad_v4i*>(pcm + fg * frame_len);
                vad_v4i w[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    w[i] = lane < nvec ? __builtin_nontemporal_load(p + i * nvec + lane) : vad_v4i{0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned long long e = wave_total(squares8(w[i]));
                    word |= (unsigned long long)level_of(e, thr_full, ngroups) << (8 * (g + i));
                }
            } else {  // short tail frame, unaligned buffer, odd frame length: one frame at a time, element loop
                for (int i = 0; i < 4 && fg + i < n_frames; ++i) {
                    const long long s0 = (fg + i) * frame_len;
                    const long long s1 = (s0 + frame_len) < n_samples ? (s0 + frame_len) : n_samples;
                    const int n = (int)(s1 - s0);
                    unsigned long long e = 0;
                    for (int base = 0; base < n; base += 512) {  // <= 8 samples per lane per round: part < 2^34
                        unsigned long long part = 0;
                        for (int j = base + lane; j < n && j < base + 512; j += 64) {
                            const int x = pcm[s0 + j];
                            part += (unsigned)(x * x);
                        }
                        e += wave_total(part);
                    }
                    unsigned level;
                    if (n == frame_len) {
                        level = level_of(e, thr_full, ngroups);
                    } else {  // the file's short last frame
                        double thr[4];
                        stage(thr, n);
                        level = level_of(e, thr, ngroups);
                    }
                    word |= (unsigned long long)level << (8 * (g + i));
                }
            }
        }
        unsigned char* out = levels + f0;
        if (f0 + VAD_FPT <= n_frames && (reinterpret_cast<uintptr_t>(out) & 7) == 0) {
            if (lane == 0) *reinterpret_cast<unsigned long long*>(out) = word;
        } else if (lane < VAD_FPT && f0 + lane < n_frames) {
            out[lane] = (unsigned char)(word >> (8 * lane));
        }
    }
}

__global__ __launch_bounds__(HIST_THREADS) void k_vad_level_hist(const unsigned char* __restrict__ levels, long long n_frames,
                                                                 int n_bins, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[VAD_MAX_BINS];
    for (int b = threadIdx.x; b < VAD_MAX_BINS; b += HIST_THREADS) s_hist[b] = 0;
    __syncthreads();
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(levels) & 15)) & 15);
    if (head > n_frames) head = n_frames;
    const long long nvec = (n_frames - head) / 16;
    const long long tail0 = head + nvec * 16;
    const uint4* body = reinterpret_cast<const uint4*>(levels + head);
    for (long long v = (long long)blockIdx.x * HIST_THREADS + threadIdx.x; v < nvec; v += (long long)gridDim.x * HIST_THREADS) {
        const uint4 q = body[v];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&s_hist[(w[k] >> (8 * i)) & 255u], 1u);
    }
    if (blockIdx.x == 0) {  // fewer than 16 bytes at either end
        if ((long long)threadIdx.x < head) atomicAdd(&s_hist[levels[threadIdx.x]], 1u);
        if (tail0 + threadIdx.x < n_frames) atomicAdd(&s_hist[levels[tail0 + threadIdx.x]], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bins; b += HIST_THREADS)  // a level byte of n_bins or more is counted nowhere
        if (s_hist[b]) atomicAdd(&hist[b], s_hist[b]);
}

FFS_DEV long long wave_excl_scan(long long x, int lane, long long* total) {  // exclusive prefix sum over the 64 lanes
    long long incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    *total = __shfl(incl, 63, 64);
    return incl - x;
}

__global__ __launch_bounds__(64) void k_vad_pick_threshold(const unsigned* __restrict__ hist, int n_bins, int rule, int lo_bin,
                                                           int t_min, int t_max, int fallback_bin, int floor_ppm,
                                                           int margin_bins, VadThreshold* __restrict__ out) {
    const int lane = threadIdx.x;
    const unsigned* h = hist + (long long)blockIdx.x * n_bins;
    long long raw[4], cnt[4];  // hist and h' of bins 4 lane .. 4 lane + 3
    long long l_raw = 0, l_n = 0, l_s = 0, l_q = 0;
    int l_top = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = 4 * lane + k;
        raw[k] = b < n_bins ? (long long)h[b] : 0;
        cnt[k] = b >= lo_bin ? raw[k] : 0;
        l_raw += raw[k];
        l_n += cnt[k];
        l_s += (long long)b * cnt[k];
        l_q += (long long)b * b * cnt[k];
        if (cnt[k]) l_top = b;
    }
    long long total, N, S, Q;
    wave_excl_scan(l_raw, lane, &total);
    const long long n_before = wave_excl_scan(l_n, lane, &N);
    const long long s_before = wave_excl_scan(l_s, lane, &S);
    wave_excl_scan(l_q, lane, &Q);
    int top = l_top;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(top, d, 64);
        top = o > top ? o : top;
    }
    // the noise floor: the smallest bin whose cumulative counted frames reach need (reported under either rule)
    const long long need0 = (N * (long long)floor_ppm + 999999) / 1000000;
    const long long need = need0 < 1 ? 1 : need0;
    int floor_bin = 1 << 30;
    {
        long long c = n_before;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c += cnt[k];
            if (c >= need && floor_bin == (1 << 30)) floor_bin = 4 * lane + k;
        }
    }
    int bottom = l_n ? 0 : (1 << 30);  // lowest occupied counted bin
    if (l_n) {
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (cnt[k]) bottom = 4 * lane + k;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_xor(floor_bin, d, 64);
        floor_bin = o < floor_bin ? o : floor_bin;
        const int p = __shfl_xor(bottom, d, 64);
        bottom = p < bottom ? p : bottom;
    }
    // Otsu: v(t) = d^2 / m over the lane's four candidates t = 4 lane + k, n0 / s0 the counts and moments below t
    double best_v = -1.0;
    int best_t = 1 << 30;
    if (N > 0 && total <= VAD_MAX_FRAMES) {
        long long n0 = n_before, s0 = s_before;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = 4 * lane + k;
            if (t > lo_bin && t < n_bins && n0 > 0 && n0 < N) {
                const long long d = S * n0 - N * s0;
                const long long m = n0 * (N - n0);
                const double v = ((double)d * (double)d) / (double)m;
                if (v > best_v) {
                    best_v = v;
                    best_t = t;
                }
            }
            n0 += cnt[k];
            s0 += (long long)t * cnt[k];
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ov = __shfl_xor(best_v, d, 64);
        const int ot = __shfl_xor(best_t, d, 64);
        if (ov > best_v || (ov == best_v && ot < best_t)) {
            best_v = ov;
            best_t = ot;
        }
    }
    if (lane == 0) {
        VadThreshold r;
        r.flags = 0;
        r.eta = 0.0;
        r.floor_bin = N > 0 ? floor_bin : -1;
        r.top_bin = top;
        r.n_frames = total;
        r.n_counted = N;
        int thr = fallback_bin;
        if (total > VAD_MAX_FRAMES) {
            r.flags = VAD_THR_TOO_LONG | VAD_THR_FALLBACK;
        } else if (N == 0) {
            r.flags = VAD_THR_EMPTY | VAD_THR_FALLBACK;
        } else {
            bool have = true;
            if (rule == VAD_RULE_OTSU) {
                if (best_t == (1 << 30)) {
                    r.flags = VAD_THR_FLAT | VAD_THR_FALLBACK;
                    have = false;
                } else {
                    thr = best_t;
                    r.eta = best_v / (double)(N * Q - S * S);
                }
            } else {
                thr = floor_bin + margin_bins;
                if (bottom == top) r.flags |= VAD_THR_FLAT;
            }
            if (have) {
                if (thr < t_min) {
                    thr = t_min;
                    r.flags |= VAD_THR_CLAMPED_LO;
                } else if (thr > t_max) {
                    thr = t_max;
                    r.flags |= VAD_THR_CLAMPED_HI;
                }
            }
        }
        r.threshold_bin = thr;
        long long sp = 0;
        for (int b = thr < 0 ? 0 : thr; b < n_bins; ++b) sp += (long long)h[b];
        r.n_speech = sp;
        out[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(LABEL_THREADS) void k_vad_level_labels(const unsigned char* __restrict__ levels, long long n_frames,
                                                                    const int* __restrict__ thr_dev, int thr_host, float non_speech,
                                                                    float* __restrict__ labels, unsigned char* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int thr = thr_dev ? *thr_dev : thr_host;
    const long long wave0 = (long long)blockIdx.x * (LABEL_THREADS / 64) + (threadIdx.x / 64);
    const long long nwaves = (long long)gridDim.x * (LABEL_THREADS / 64);
    for (long long base = wave0 * 64; base < n_frames; base += nwaves * 64) {  // wave-uniform trip count
        const long long f = base + lane;
        const bool speech = f < n_frames && (int)levels[f] >= thr;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(speech);
        if (labels && f < n_frames) labels[f] = speech ? 1.0f : non_speech;
        if (bits && lane < 8 && base + 8 * lane < n_frames) bits[base / 8 + lane] = (unsigned char)(mask >> (8 * lane));
    }
}

}  // namespace ffsa
