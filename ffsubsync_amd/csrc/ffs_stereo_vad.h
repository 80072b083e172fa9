// ffs_stereo_vad.h -- centre-channel VAD: mid and side levels of stereo PCM and the centre gate (gfx950): the device
// side of adaptive_vad.stereo_levels / centre_gate.  Dialogue is mixed to the centre (L ~ R), music,
// ambience and audiences are mixed wide, so a frame whose mid level (L + R) does not stand min_contrast_bins above its
// side level (L - R) is not dialogue, however loud.  The project's own rule, no upstream counterpart: pinned bit for bit
// against tests/stereo_vad_model.py only.  Contract (include/ffsubsync_amd.h, ffs_vad_stereo_levels / ffs_vad_centre_gate):
//   M_f = sum (L_i + R_i)^2, S_f = sum (L_i - R_i)^2 over the frame's n_f pairs, exact 64-bit integers
//   mid[f]  = #{k : (double)M_f >= edges[k] * (double)(4 n_f)},  side[f] likewise from S_f
//   out[f]  = mid[f] if (int)mid[f] - (int)side[f] >= c else 0;  active(f) = mid[f] >= t;  kept(f) = active and contrast >= c
//
// k_vad_stereo_levels: k_vad_levels' sweep (a wave owns VAD_FPT = 8 frames and walks them four at a time, 16-byte
// nontemporal loads, the lane's edges staged once per wave, level_of) over interleaved (L, R) pairs.  Which path a group
// of four frames takes is wave-uniform:
//   VECTOR path   frame_len % 4 == 0 (a frame is a whole number of 16-byte vectors of four pairs), frame_len <=
//                 STEREO_MAX_FRAME_VEC = 512 pairs (nvec = frame_len / 4 <= STEREO_MAX_VEC = 128: lane l takes vector l
//                 and, when nvec > 64, vector l + 64 of each frame -- 480 pairs at 48 kHz are 120 vectors), the PCM
//                 16-byte aligned, and all four frames whole.  Eight loads per lane in flight.
//   ELEMENT path  everything else -- frame_len not a multiple of 4 or above 512, PCM only 2-, 4- or 8-byte aligned, the
//                 last (up to four) frames of the buffer, the short last frame: one frame at a time, a pair a lane.
// Arithmetic.  P = sum (L^2 + R^2) is squares2 per pair word.  X = sum L R is one more v_dot2c_i32_i16 of the word against
// itself shifted right by 16 (halves R, 0); M = P + 2 X, S = P - 2 X.  The mono helpers' preconditions do not carry over:
// (L + R)^2 reaches 2^32 and 2 L R reaches 2^31 at L = R = -32768, so neither is ever formed in 32 bits.  L R lies in
// [-32768 * 32767, 2^30]; with the bias STEREO_X_BIAS = 32768 * 32767 it lies in [0, 2^31 - 32768], so TWO pairs chain
// through one dot2c accumulator that starts at 2 * bias (at most 2^32 - 65536: the bit pattern is the unsigned sum),
// and the bias leaves again in 64 bits.  A lane's M or S over its eight pairs is at most 2^35, above wave_total's
// stated 2^34: wave_total40 is the same two-halves DPP reduction with the halves cut for parts below 2^40, and the
// element loop takes at most 64 pairs per lane per round (2^38).
// No atomics, no LDS, nothing written behind the last frame; the 8 level bytes of a task leave as one 8-byte store per
// output where its address allows and all 8 frames exist, else byte by byte from lanes 0..7.
//
// k_centre_gate: a lane a frame, at most CENTRE_MAX_BLOCKS workgroups of 256 threads in a grid-stride loop; byte loads
// and stores, so every input and the output may sit at any address.  Each thread counts in integers, the workgroup
// reduces (wave butterflies, then LDS) and thread 0 adds its non-zero sums into the record with integer atomics (add,
// and max for max_side): at most 4 * CENTRE_MAX_BLOCKS per call, order-independent, as k_vad_level_hist's.  The host
// call zeroes the record on the stream first; k_centre_finish, one wave behind it, writes threshold_bin,
// min_contrast_bins, n_frames and the flags.  No workgroup waits for another.
#pragma once
#include "ffs_vad_gate.h"

namespace ffsa {

constexpr int STEREO_MAX_VEC = 128;                        // 16-byte vectors of a frame on the vector path: two per lane
constexpr int STEREO_MAX_FRAME_VEC = STEREO_MAX_VEC * 4;   // 512 pairs: the longest frame of the vector path
constexpr int STEREO_ELEM_ROUND = 64 * 64;                 // pairs of one element-path round: 64 per lane, part <= 2^38
constexpr unsigned STEREO_X_BIAS = 32768u * 32767u;        // -min(L R): L R + bias lies in [0, 2^31 - 32768]
constexpr int CENTRE_THREADS = 256;
constexpr int CENTRE_MAX_BLOCKS = 256;                     // workgroups of k_centre_gate, at most
constexpr int32_t VAD_CENTRE_MONO = 1;                     // FFS_VAD_CENTRE_MONO
constexpr int32_t VAD_CENTRE_ALL_REJECTED = 2;             // FFS_VAD_CENTRE_ALL_REJECTED

struct VadCentre {  // = ffs_vad_centre
    int32_t threshold_bin, flags, min_contrast_bins, max_side;
    int64_t n_frames, n_active, n_kept, sum_contrast;
};
static_assert(sizeof(VadCentre) == 48, "VadCentre must match ffs_vad_centre");

FFS_DEV unsigned long long wave_total40(unsigned long long part) {  // part < 2^40 per lane; wave-uniform result
    const unsigned lo = row_total((unsigned)part & 0xFFFFFu), hi = row_total((unsigned)(part >> 20));
    unsigned long long t = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        t += (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)lo, 16 * r) +
             ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi, 16 * r) << 20);
    return t;
}

// L0 R0 + L1 R1 + 2 * STEREO_X_BIAS of two pair words (low half L, high half R), at most 2^32 - 65536: the bit pattern
// is the unsigned sum.  Inline asm as squares2.
FFS_DEV unsigned cross2x2(int w0, int w1) {
    int d = (int)(2u * STEREO_X_BIAS);
    const int r0 = (int)((unsigned)w0 >> 16), r1 = (int)((unsigned)w1 >> 16);
    asm("v_dot2c_i32_i16 %0, %1, %2" : "+v"(d) : "v"(w0), "v"(r0));
    asm("v_dot2c_i32_i16 %0, %1, %2" : "+v"(d) : "v"(w1), "v"(r1));
    return (unsigned)d;
}

// the four pairs of a 16-byte vector added into p = sum (L^2 + R^2) and xb = sum (L R + STEREO_X_BIAS)
FFS_DEV void stereo_acc4(vad_v4i w, unsigned long long& p, unsigned long long& xb) {
    p += squares8(w);
    xb += cross2x2(w[0], w[1]);
    xb += cross2x2(w[2], w[3]);
}

__global__ __launch_bounds__(256) void k_vad_stereo_levels(const int16_t* __restrict__ pcm, long long n_pairs, int frame_len,
                                                           long long n_frames, const double* __restrict__ edges, int n_edges,
                                                           unsigned char* __restrict__ mid, unsigned char* __restrict__ side) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
    const long long nwaves = (long long)gridDim.x * (blockDim.x / 64);
    const long long n_tasks = (n_frames + VAD_FPT - 1) / VAD_FPT;
    const int nvec = frame_len / 4;
    const bool vec_ok = (frame_len % 4 == 0) && nvec <= STEREO_MAX_VEC && ((reinterpret_cast<uintptr_t>(pcm) & 15) == 0);
    const bool two = nvec > 64;               // wave-uniform: a lane holds a second vector of each frame
    const int ngroups = (n_edges + 63) / 64;  // <= 4
    // the lane's edges times 4 n (an exact scaling); an edge beyond the table is +inf: never reached
    auto stage = [&](double (&thr)[4], int n) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            thr[j] = (lane + 64 * j < n_edges ? edges[lane + 64 * j] : __builtin_huge_val()) * (double)(4ll * n);
    };
    double thr_full[4];
    stage(thr_full, frame_len);
    for (long long t = wave0; t < n_tasks; t += nwaves) {
        const long long f0 = t * VAD_FPT;
        unsigned long long wm = 0, ws = 0;  // byte i = mid / side level of frame f0 + i
#pragma unroll
        for (int g = 0; g < VAD_FPT; g += 4) {
            const long long fg = f0 + g;
            if (fg >= n_frames) break;
            if (vec_ok && (fg + 4) * frame_len <= n_pairs) {  // four whole frames: wave-uniform vector path
                const vad_v4i* p = reinterpret_cast<const vad_v4i*>(pcm + 2 * fg * frame_len);
                vad_v4i a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[i] = lane < nvec ? __builtin_nontemporal_load(p + i * nvec + lane) : vad_v4i{0, 0, 0, 0};
                if (two) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        b[i] = lane + 64 < nvec ? __builtin_nontemporal_load(p + i * nvec + lane + 64) : vad_v4i{0, 0, 0, 0};
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned long long pp = 0, xb = 0;
                    stereo_acc4(a[i], pp, xb);
                    long long x = (long long)xb - 4ll * STEREO_X_BIAS;  // a zero vector holds four times the bias too
                    if (two) {
                        unsigned long long xb2 = 0;
                        stereo_acc4(b[i], pp, xb2);
                        x += (long long)xb2 - 4ll * STEREO_X_BIAS;
                    }
                    const unsigned long long m = wave_total40((unsigned long long)((long long)pp + 2 * x));
                    const unsigned long long s = wave_total40((unsigned long long)((long long)pp - 2 * x));
                    wm |= (unsigned long long)level_of(m, thr_full, ngroups) << (8 * (g + i));
                    ws |= (unsigned long long)level_of(s, thr_full, ngroups) << (8 * (g + i));
                }
            } else {  // tail frames, unaligned buffer, other frame lengths: one frame at a time, a pair a lane
                for (int i = 0; i < 4 && fg + i < n_frames; ++i) {
                    const long long s0 = (fg + i) * frame_len;
                    const long long s1 = (s0 + frame_len) < n_pairs ? (s0 + frame_len) : n_pairs;
                    const int n = (int)(s1 - s0);
                    unsigned long long m = 0, s = 0;
                    for (long long base = 0; base < n; base += STEREO_ELEM_ROUND) {  // <= 64 pairs per lane per round: part <= 2^38
                        unsigned long long pm = 0, ps = 0;
                        for (long long j = base + lane; j < n && j < base + STEREO_ELEM_ROUND; j += 64) {
                            const int l = pcm[2 * (s0 + j)], r = pcm[2 * (s0 + j) + 1];
                            const long long u = l + r, v = l - r;
                            pm += (unsigned long long)(u * u);
                            ps += (unsigned long long)(v * v);
                        }
                        m += wave_total40(pm);
                        s += wave_total40(ps);
                    }
                    unsigned lm, ls;
                    if (n == frame_len) {
                        lm = level_of(m, thr_full, ngroups);
                        ls = level_of(s, thr_full, ngroups);
                    } else {  // the buffer's short last frame
                        double thr[4];
                        stage(thr, n);
                        lm = level_of(m, thr, ngroups);
                        ls = level_of(s, thr, ngroups);
                    }
                    wm |= (unsigned long long)lm << (8 * (g + i));
                    ws |= (unsigned long long)ls << (8 * (g + i));
                }
            }
        }
        const bool whole = f0 + VAD_FPT <= n_frames;
        unsigned char* om = mid + f0;
        unsigned char* os = side + f0;
        if (whole && (reinterpret_cast<uintptr_t>(om) & 7) == 0) {
            if (lane == 0) *reinterpret_cast<unsigned long long*>(om) = wm;
        } else if (lane < VAD_FPT && f0 + lane < n_frames) {
            om[lane] = (unsigned char)(wm >> (8 * lane));
        }
        if (whole && (reinterpret_cast<uintptr_t>(os) & 7) == 0) {
            if (lane == 0) *reinterpret_cast<unsigned long long*>(os) = ws;
        } else if (lane < VAD_FPT && f0 + lane < n_frames) {
            os[lane] = (unsigned char)(ws >> (8 * lane));
        }
    }
}

FFS_DEV long long centre_wave_sum(long long v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(CENTRE_THREADS) void k_centre_gate(const unsigned char* __restrict__ mid,
                                                                const unsigned char* __restrict__ side, long long n_frames,
                                                                const int* __restrict__ thr_dev, int thr_host, int min_contrast,
                                                                unsigned char* __restrict__ out, VadCentre* __restrict__ record) {
    __shared__ long long s_sum[CENTRE_THREADS / 64][3];
    __shared__ int s_max[CENTRE_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int thr = thr_dev ? *thr_dev : thr_host;
    long long n_active = 0, n_kept = 0, sum_contrast = 0;
    int max_side = 0;
    for (long long f = (long long)blockIdx.x * CENTRE_THREADS + threadIdx.x; f < n_frames; f += (long long)gridDim.x * CENTRE_THREADS) {
        const int m = (int)mid[f], s = (int)side[f];
        const int contrast = m - s;
        const bool pass = contrast >= min_contrast;
        if (out) out[f] = pass ? (unsigned char)m : (unsigned char)0;
        if (m >= thr) {
            n_active += 1;
            n_kept += pass ? 1 : 0;
            sum_contrast += contrast;
        }
        max_side = s > max_side ? s : max_side;
    }
    n_active = centre_wave_sum(n_active);
    n_kept = centre_wave_sum(n_kept);
    sum_contrast = centre_wave_sum(sum_contrast);
    max_side = gate_wave_max(max_side);
    if (lane == 0) {
        s_sum[wave][0] = n_active;
        s_sum[wave][1] = n_kept;
        s_sum[wave][2] = sum_contrast;
        s_max[wave] = max_side;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CENTRE_THREADS / 64; ++w) {
            n_active += s_sum[w][0];
            n_kept += s_sum[w][1];
            sum_contrast += s_sum[w][2];
            max_side = s_max[w] > max_side ? s_max[w] : max_side;
        }
        // two's complement: the signed sum adds as an unsigned one
        if (n_active) atomicAdd(reinterpret_cast<unsigned long long*>(&record->n_active), (unsigned long long)n_active);
        if (n_kept) atomicAdd(reinterpret_cast<unsigned long long*>(&record->n_kept), (unsigned long long)n_kept);
        if (sum_contrast) atomicAdd(reinterpret_cast<unsigned long long*>(&record->sum_contrast), (unsigned long long)sum_contrast);
        if (max_side) atomicMax(&record->max_side, max_side);
    }
}

__global__ __launch_bounds__(64) void k_centre_finish(long long n_frames, const int* __restrict__ thr_dev, int thr_host,
                                                      int min_contrast, VadCentre* __restrict__ record) {
    if (threadIdx.x != 0) return;
    record->threshold_bin = thr_dev ? *thr_dev : thr_host;
    record->min_contrast_bins = min_contrast;
    record->n_frames = n_frames;
    record->flags = (n_frames > 0 && record->max_side == 0 ? VAD_CENTRE_MONO : 0) |
                    (record->n_active > 0 && record->n_kept == 0 ? VAD_CENTRE_ALL_REJECTED : 0);
}

}  // namespace ffsa
