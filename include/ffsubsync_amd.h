/*
 * ffsubsync_amd.h -- C ABI of libffsalign.so, the MI355X (gfx950) implementation of
 * ffsubsync's alignment hot path.
 *
 * The reference (smacke/ffsubsync) is pure Python and has no FFI of its own for this path;
 * each entry point below names the reference interface (file:line under
 * /root/reference/ffsubsync/) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative FFS_E_* code; nothing throws across
 *     the ABI; ffs_last_error() returns a thread-local message for the last failure.
 *   - "_dev" pointers are device (HBM) addresses owned by the caller (e.g. torch tensors'
 *     data_ptr()); all other pointers are host memory.  `hip_stream` is a hipStream_t
 *     (0 = the null stream).  Calls are asynchronous with respect to the host unless stated;
 *     results land in caller-owned device buffers in stream order.  ffs_align_batch* may copy
 *     their own descriptors to the device on an internal copy stream (one per device); the kernels
 *     that read the caller's vectors and write its results run on `hip_stream` only, after the
 *     stream has waited for those copies.
 *   - a plan owns its twiddle tables and workspace in HBM and may be used by one host thread
 *     at a time; successive calls on different streams are ordered by the library (a call waits
 *     for the plan's previous call before it touches the workspace).
 *   - entry points without a plan run on the device that owns their output buffer.
 */
#ifndef FFSUBSYNC_AMD_H
#define FFSUBSYNC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFS_OK 0
#define FFS_E_INVALID (-1) /* bad argument */
#define FFS_E_HIP (-2)     /* a HIP runtime call failed */
#define FFS_E_NOMEM (-3)
#define FFS_E_TOO_LONG (-4) /* R+S exceeds the plan's transform length */
#define FFS_E_EMPTY (-5)    /* empty reference or candidate (aligners.py:58-66) */
#define FFS_E_RCCL (-6)     /* librccl could not be loaded or an RCCL call failed */

/* element types of the activity vectors */
#define FFS_DTYPE_U8 0  /* two-level signal: byte==0 -> lo, byte!=0 -> hi  */
#define FFS_DTYPE_F32 1 /* arbitrary float samples (lo/hi = bounds, used for the tie margin) */
#define FFS_DTYPE_F64 3 /* as FFS_DTYPE_F32 with double samples: the transforms still nominate in fp32, the winning
                           lags are re-evaluated in fp64 from the caller's own samples (the reference's arithmetic,
                           aligners.py:55-57, without any input rounding) */
#define FFS_DTYPE_U1 2  /* two-level signal, one bit per sample: sample i = bit (i & 31) of the 32-bit
                           little-endian word i >> 5 (numpy.packbits(..., bitorder="little")); 0 -> lo, 1 -> hi.
                           The native format of the 0/1 activity vectors: an eighth of the HBM and PCIe bytes of
                           FFS_DTYPE_U8.  Pointers 4-byte aligned; the buffer must cover whole 32-bit words. */
#define FFS_DTYPE_RUNS 5 /* two-level signal as its BOUNDARY LIST (what speech_transformers.py:957-980 is handed: the
                           subtitles' intervals).  The pointer is a device block `ffs_runs_list` (8-byte aligned):
                             int32 n, ones, len, cap;           -- boundaries, samples at the upper level, samples, entries
                             struct { int32 pos, ones_before; } e[cap];
                           e[k].pos (k < n, ascending, n even) = a sample where the value changes -- even k: a run of
                           the upper level starts, odd k: one past its last sample (a run that reaches the end closes at
                           `len`); e[k].ones_before = upper-level samples in front of it; e[n] = (INT32_MAX, ones).
                           Producers: ffs_rasterize_batch_runs, ffs_runs_from_bits.  A list with n >= cap is truncated
                           and unusable.  ffs_runs_list_bytes(cap) = 16 + 8 * cap. */
/* What every entry point keeps to, for vectors of all these types (pinned by tests/test_gpu_layout.py on vectors at
 * exactly these alignments, with 0xFF -- ones, NaNs -- in every byte around them and other vectors right behind them):
 *   - alignment: FFS_DTYPE_U8 pointers need none, FFS_DTYPE_U1 and FFS_DTYPE_F32 4 bytes, FFS_DTYPE_F64 and
 *     `ffs_runs_list` blocks 8 bytes; nothing assumes more (no 16- or 64-byte alignment, no padding behind a vector);
 *   - the bits of the last FFS_DTYPE_U1 word at positions >= len, and all bytes outside a vector, are never
 *     interpreted: they may hold anything, the neighbouring vector's samples included (a kernel may load them, inside
 *     the words the vector covers, but no result depends on them);
 *   - the entries of a list block behind the sentinel e[n] are never read;
 *   - inputs are never written;
 *   - outputs are written only inside their documented extent: ceil(len/32) words of a bit-packed output (its unused
 *     last bits are written as 0), ffs_runs_list_bytes(cap) bytes of a list block, n records of a record array. */

/* result flags */
#define FFS_FLAG_EMPTY_WINDOW 1 /* every lag masked: score=-inf, offset=N-1-S (aligners.py:45-48) */
#define FFS_FLAG_AMBIGUOUS 2    /* more near-ties than the nominee list holds; best of list returned */
#define FFS_FLAG_FILTERED 4     /* |offset| > filter_max_offset: dropped by MaxScoreAligner.transform */
#define FFS_FLAG_DIRECT 8       /* solved by the exact direct-correlation kernel (short inputs) */

typedef struct ffs_plan ffs_plan;

/* One FFTAligner solve: FFTAligner.best_score_ / best_offset_ (aligners.py:45-48). */
typedef struct ffs_cand_result {
    double score;    /* correlation at `offset`, re-evaluated exactly (integer counts for
                        two-level inputs, fp64 dot product for float inputs) */
    int64_t offset;  /* samples; subtitle must be shifted by +offset/sample_rate seconds */
    float score_f32; /* the fp32 FFT's value at that lag (diagnostic) */
    int32_t flags;
} ffs_cand_result;

/* One MaxScoreAligner solve: the winning ((score, offset), candidate) (aligners.py:154-167). */
typedef struct ffs_pair_result {
    double score;
    int64_t offset;
    int32_t best_cand; /* index into the pair's candidate list; -1 = none survived the filter */
    int32_t flags;
} ffs_pair_result;

/* Smallest transform length the reference would use for these lengths:
 * 2**ceil(log2(R+S)) (aligners.py:67-68).  Returns 0 if either length is <= 0. */
int64_t ffs_fft_length(int64_t ref_len, int64_t sub_len);

/* Smallest supported transform length (2^k, or 3*2^k in [12288, 3145728]) a plan needs for one
 * (reference, candidate) solve.
 * Only lags with a non-empty overlap, d in (-S, R), ever need a transform: every other lag the reference
 * looks at has c(d) = 0 exactly and is handled as one virtual nominee (score 0, the largest such lag).
 * Without a lag window the R+S-1 overlap lags need a circular correlation of length >= R+S (3*2^19 =
 * 1 572 864 instead of the reference's 2^21 for 2 h @ 100 Hz inputs).  With
 * max_offset_samples >= 0 only lags inside the reference's window [d_lo, d_hi] are ever looked at:
 * only the prefixes S' = min(S, R - d_lo) and R' = min(R, S + d_hi) of the two vectors can meet at
 * such a lag (the rest is multiplied by zero padding), and a circular correlation of any length
 * n >= max(S' + d_hi, R' - d_lo) + 1 over them reproduces those lags exactly (no product wraps), so
 * a shorter transform gives bit-identical results:
 * 3*2^18 = 786 432 instead of 2^21 for 2 h @ 100 Hz inputs with the default +-6000 window.
 * (FFS_DISABLE_RADIX3=1 in the environment restricts the answer to powers of two.) */
int64_t ffs_plan_length(int64_t ref_len, int64_t sub_len, int64_t max_offset_samples);

/* Create a plan for transform length n_fft (a power of two in [2, 2^24], or 3*2^k in
 * [12288, 3145728]) on `device`.
 * pairs_in_flight: how many (reference, candidates) problems share one sweep of the
 * A/mid/C kernels (sizes the workspace: pairs_in_flight * (1+ceil(max_cand/2)) * n_fft * 8 B; twice
 * that for n_fft = 3*2^k >= 3*2^16, which also carries the block-segmented pipeline used under
 * narrow lag windows).
 * Replaces: the per-call np.fft plan + temporaries of FFTAligner.fit (aligners.py:67-74). */
int ffs_plan_create(int device, int64_t n_fft, int pairs_in_flight, int max_cand, ffs_plan** out);
int ffs_plan_destroy(ffs_plan* plan);
int64_t ffs_plan_workspace_bytes(const ffs_plan* plan);

/* Batched MaxScoreAligner(FFTAligner).fit(...).transform() over n_pairs independent problems,
 * each one reference vector and n_cand candidate vectors (aligners.py:50-80, 131-167).
 *
 * Vectors are listed pair-major: index p*(1+n_cand) is pair p's reference, the next n_cand
 * entries its candidates.  vec_ptr[i] is a DEVICE pointer to vec_len[i] elements of `dtype`
 * (vec_len counts samples for every dtype);
 * vec_lo/vec_hi give the two sample values of a FFS_DTYPE_U8 / FFS_DTYPE_U1 vector *before* the reference's
 * 2*x-1 map (aligners.py:55-57), e.g. (0, 1) for a 0/1 vector or (0, 1/ratio) for a subtitle
 * track rasterised at a framerate ratio > 1 (speech_transformers.py:977).
 *
 * max_offset_samples: FFTAligner(max_offset_samples) lag window, -1 = None; the window is the
 *   reference's, including Python negative-slice semantics (aligners.py:31-43).
 * filter_max_offset: MaxScoreAligner.max_offset_samples used to drop candidates
 *   (aligners.py:156-159), -1 = None.
 * cand_out_dev[n_pairs*n_cand], pair_out_dev[n_pairs]: device buffers, written in stream order.
 * Every (R, S) must satisfy ffs_plan_length(R, S, max_offset_samples) <= plan n_fft.
 * Host arrays may be freed after return. */
int ffs_align_batch(ffs_plan* plan, int n_pairs, int n_cand, int dtype,
                    const void* const* vec_ptr, const int64_t* vec_len,
                    const double* vec_lo, const double* vec_hi,
                    int64_t max_offset_samples, int64_t filter_max_offset,
                    ffs_cand_result* cand_out_dev, ffs_pair_result* pair_out_dev,
                    void* hip_stream);

/* The same solve with one element type PER VECTOR: vec_dtype[i] is the FFS_DTYPE_* of vec_ptr[i] (pair-major like the
 * other arrays).  Within one call every reference must share one type and every candidate one type; the two may
 * differ.  The case this exists for: a multi-level float reference -- the `weighted` fused VAD emits
 * {0, 0.4, 0.6, 1} (speech_transformers.py:290-293), non_speech_label may be != 0 -- against two-level subtitle
 * rasters (speech_transformers.py:957-980), which then stay bit-packed (FFS_DTYPE_U1): the first pass reads each role
 * in its own format, the fp32 transforms nominate, and the nominees are re-evaluated in fp64 from the caller's own
 * samples (sum_i s'[i] * (2 r[i+d] - 1) with s' the candidate's fp64 level values).  vec_lo / vec_hi of a float vector
 * are bounds of its samples (used for the tie margin).  With all types equal this is ffs_align_batch.
 * Replaces: aligners.py:50-80, 131-167 for float-valued inputs. */
int ffs_align_batch_typed(ffs_plan* plan, int n_pairs, int n_cand, const int32_t* vec_dtype,
                          const void* const* vec_ptr, const int64_t* vec_len,
                          const double* vec_lo, const double* vec_hi,
                          int64_t max_offset_samples, int64_t filter_max_offset,
                          ffs_cand_result* cand_out_dev, ffs_pair_result* pair_out_dev,
                          void* hip_stream);

/* ffs_align_batch_typed plus, for FFS_DTYPE_RUNS vectors, vec_max_boundaries[i] (may be NULL; other types: ignored) = a
 * HOST-KNOWN upper bound of list i's length (0 = unknown) -- the rasteriser's lists have at most two entries per
 * subtitle.  When every vector of the call is a list with a bound and no candidate can exceed the coincidence budget
 * even at the bounds, the call queues its kernels and returns without waiting for anything from the device; otherwise it
 * waits once for one int per sub-batch (which sub-batches need the transforms).  A call whose lists break their stated
 * bounds has undefined results.
 * Replaces: aligners.py:50-80, 131-167 fed straight from speech_transformers.py:957-980 (no raster in between). */
int ffs_align_batch_runs(ffs_plan* plan, int n_pairs, int n_cand, const int32_t* vec_dtype,
                         const void* const* vec_ptr, const int64_t* vec_len,
                         const double* vec_lo, const double* vec_hi, const int32_t* vec_max_boundaries,
                         int64_t max_offset_samples, int64_t filter_max_offset,
                         ffs_cand_result* cand_out_dev, ffs_pair_result* pair_out_dev,
                         void* hip_stream);

/* Bytes of an `ffs_runs_list` block with room for `cap` entries (sentinel included): 16 + 8 * cap. */
int64_t ffs_runs_list_bytes(int64_t cap);
/* Boundary list of a bit-packed vector (FFS_DTYPE_U1, `len` samples at bits_dev) into the caller's block list_dev of
 * capacity `cap` entries (8-byte aligned, ffs_runs_list_bytes(cap) bytes): one pass over the bits.  A vector with cap
 * boundaries or more leaves n >= cap in the header (truncated).  Convert once -- VAD labels, a deserialised reference
 * (speech_transformers.py:993-1005) -- and every later solve skips the pass over the bits. */
int ffs_runs_from_bits(const uint32_t* bits_dev, int64_t len, void* list_dev, int64_t cap, void* hip_stream);
/* The same for n_vec vectors in one launch (host tables of device pointers / lengths / capacities). */
int ffs_runs_from_bits_batch(const uint32_t* const* bits_dev, const int64_t* len, void* const* list_dev, const int64_t* cap,
                             int64_t n_vec, void* hip_stream);
/* The inverse (parity tests; the transform path uses the same kernel for list-only vectors): `len` samples of the
 * list's vector as FFS_DTYPE_U1 words at bits_out_dev (ceil(len/32) words). */
int ffs_runs_to_bits(const void* list_dev, int64_t len, uint32_t* bits_out_dev, void* hip_stream);

/* How ffs_align_batch / ffs_align_batch_typed evaluate the correlation of aligners.py:50-80.  Results are identical
 * either way (same exact scores, same tie rule); only the time differs.
 *   FFS_ALGO_AUTO (default): two-level vectors given as bits or as boundary lists (FFS_DTYPE_U1 / FFS_DTYPE_RUNS on both
 *     sides) first go through the run-boundary path -- the exact integer correlation of the two run-length-coded vectors
 *     over every lag of the window, no transform (csrc/ffs_runs.h) -- and the call waits once (an event, not the stream,
 *     after all of its kernels are queued) for one int per sub-batch: whether it needs the transforms; sub-batches (pairs_in_flight pairs) holding a vector with 32 768 boundaries or more, or a candidate
 *     whose expected number of boundary coincidences inside its lag window (boundaries of the candidate x boundaries of
 *     the reference x window lags / reference length) exceeds the budget -- by default twelve per point of the plan's
 *     transform length and packed transform slot the candidate occupies, (n_cand + 1) / (2 n_cand) of one: the measured
 *     break-even -- are solved by the transforms instead.  A FLOAT reference (FFS_DTYPE_F32 / F64) with at most four
 *     distinct sample values whose steps are small integer multiples of one quantum -- the `weighted` fused VAD's
 *     {l, .4 + .6 l, .6 + .4 l, 1}, speech_transformers.py:290-293 -- against two-level candidates takes the same path:
 *     its threshold vectors are made on the device and their coincidences added with integer multiplicities; any other
 *     float vector (more levels, no common quantum, noise) and every other element type go through the transforms.
 *   FFS_ALGO_FFT: transforms only (the path of rounds 1-3).
 *   FFS_ALGO_RUNS: like AUTO without the coincidence budget (truncated boundary lists still fall back).
 *   Boundary lists of vectors that arrive as bits live in the plan, 4 096 entries per vector to start with (FFS_RUNS_STRIDE);
 *   a call that meets a longer list is solved again with four times the room (at most twice, up to 32 768 entries) and
 *   the plan keeps the longer stride -- which path solves what does not depend on it.
 * Environment: FFS_ALGORITHM=auto|fft|runs presets new plans, FFS_RUNS_BUDGET=<coincidences> the budget. */
#define FFS_ALGO_AUTO 0
#define FFS_ALGO_FFT 1
#define FFS_ALGO_RUNS 2
int ffs_plan_set_algorithm(ffs_plan* plan, int algorithm);
/* Since plan creation: calls that tried the run-boundary path, their sub-batches, and how many of those went through
 * the transforms after all; boundaries_last_call = boundary-list entries of all vectors of the most recent such call
 * (what k_runs_extract wrote: 8 bytes each).  Any pointer may be NULL. */
int ffs_plan_runs_stats(ffs_plan* plan, int64_t* calls, int64_t* sub_batches, int64_t* sub_batches_through_transforms,
                        int64_t* boundaries_last_call);
/* What the most recent ffs_align_batch* call on the plan launched for the sub-batches it sent through the transforms
 * (read-only; noted by the launch functions themselves, no device work, no synchronisation).  All zero when no
 * sub-batch took the transforms (run-boundary path, direct kernel).  The sub-batches of one call share every choice.
 *   transform_sub_batches  sub-batches that went through the transforms
 *   transform_length       length the transform kernels ran at: the plan's N, or N/3 in block-segmented mode
 *   n1, n2                 its column and row lengths (transform_length = n1 * n2)
 *   seg_blocks             blocks per vector in block-segmented mode (2 or 3), 0 otherwise
 *   half_flags             1: the reference slot holds half of its rows, 2: so does a single-candidate last slot
 *   pass_a_family          first pass of the candidate slots: FFS_DISPATCH_PASS_A (k_pass_a) or _PASS_A3 (k_pass_a3)
 *   pass_a_ref_family      the same for the reference slots when they are launched on their own (reference and
 *                          candidates of different element types), 0 otherwise
 *   pass_a_paired          0: one column transform per slot; 1: reference and the only candidate slot paired;
 *                          2: reference and the single-candidate last slot paired
 *   mid_family             FFS_DISPATCH_MID (k_mid), _MID_SEG_ONE_1 / _MID_SEG_ONE_4 (k_mid_seg_one with one / four
 *                          accumulator rows), _MID_SEG_PIPE (k_mid_seg_pipe)
 *   last_family            FFS_DISPATCH_LAST_FULL (k_pass_c), _LAST_C3 (k_pass_c3), _LAST_PRUNED (k_pass_c_pruned)
 *   sweep_family           the exhaustive sweep over flagged candidates: _LAST_FULL or _LAST_PRUNED (whether any
 *                          candidate was flagged is known on the device only) */
#define FFS_DISPATCH_PASS_A 1
#define FFS_DISPATCH_PASS_A3 2
#define FFS_DISPATCH_MID 1
#define FFS_DISPATCH_MID_SEG_ONE_1 2
#define FFS_DISPATCH_MID_SEG_ONE_4 3
#define FFS_DISPATCH_MID_SEG_PIPE 4
#define FFS_DISPATCH_LAST_FULL 1
#define FFS_DISPATCH_LAST_C3 2
#define FFS_DISPATCH_LAST_PRUNED 3
typedef struct ffs_dispatch_report {
    int32_t transform_sub_batches;
    int32_t transform_length;
    int32_t n1, n2;
    int32_t seg_blocks;
    int32_t half_flags;
    int32_t pass_a_family;
    int32_t pass_a_ref_family;
    int32_t pass_a_paired;
    int32_t mid_family;
    int32_t last_family;
    int32_t sweep_family;
} ffs_dispatch_report;
int ffs_plan_dispatch_report(ffs_plan* plan, ffs_dispatch_report* out);

/* Full correlation of one reference with one or two candidates (b_dev may be NULL):
 *   out_x_dev[m] = sum_i x'[i] * ref'[(i + m) mod n_fft],  m in [0, n_fft)
 * i.e. the reference's `convolve` array (aligners.py:74) with convolve[k] = out[(N-1-S-k) mod N].
 * Used by the parity tests to compare the raw fp32 correlation against np.fft. */
int ffs_correlate_full(ffs_plan* plan, int dtype,
                       const void* ref_dev, int64_t ref_len, double ref_lo, double ref_hi,
                       const void* a_dev, int64_t a_len, double a_lo, double a_hi,
                       const void* b_dev, int64_t b_len, double b_lo, double b_hi,
                       float* out_a_dev, float* out_b_dev, void* hip_stream);

/* Frame-energy voice-activity sweep over s16le mono PCM resident in HBM.
 * labels_dev[f] = (10*log10(mean(x^2) over frame f) >= energy_threshold_db) ? 1.0f
 *                                                                           : non_speech_label
 * for f in [0, ceil(n_samples/frame_len)); the last frame may be short.  Replaces the
 * per-frame Python loop of the detector closures (speech_transformers.py:133-150, 169-181)
 * with the AudioEnergyValidator rule (threshold 50 dB in the reference, :124).  The rule is evaluated as
 * sum(x^2) >= 10^(energy_threshold_db/10) * n on the exact 64-bit sum, so a frame exactly at the threshold is
 * speech.  The labels are float32: a non_speech_label that float32 cannot hold (0.1) comes back rounded, and a
 * caller that owes float64 labels (the detector closures) maps the speech flags on the host instead. */
int ffs_vad_energy(const int16_t* pcm_dev, int64_t n_samples, int frame_len,
                   double energy_threshold_db, float non_speech_label,
                   float* labels_dev, void* hip_stream);

/* The same sweep with the labels written bit-packed, straight into the form the aligner reads
 * (FFS_DTYPE_U1): bit (f & 7) of bits_dev[f >> 3] = 1 iff frame f is speech, for
 * f in [0, ceil(n_samples/frame_len)); the unused high bits of the last byte are written as 0.
 * ceil(n_frames/8) bytes are written, nothing beyond them -- a caller that sweeps a file chunk by
 * chunk (the reference's 100 s buffers, speech_transformers.py:683-685, are 10 000 frames = 1250
 * bytes) points each call at byte (first_frame / 8) of one zero-initialised word buffer.  Replaces
 * the label vector of speech_transformers.py:133-150 plus the host-side 0/1 conversion in front of
 * aligners.py:55-57. */
int ffs_vad_energy_bits(const int16_t* pcm_dev, int64_t n_samples, int frame_len,
                        double energy_threshold_db, uint8_t* bits_dev, void* hip_stream);

/* Token smoothing of a frame-validity sweep, as the reference's auditok detector applies it
 * (speech_transformers.py:125-131, 140-150): auditok 0.1.5's StreamTokenizer state machine
 * (min_length, max_length, max_continuous_silence in frames; default mode) run independently on
 * every chunk of `chunk_frames` frames (the reference re-opens the tokenizer per 100 s buffer), then
 * the reference's rasterisation: marker[start] = 1, marker[end+1] = non_speech_label - 1 (assigned in
 * token order), out = clip(cumsum(marker)[:-1], 0, 1).
 * valid_dev[f] != 0  <=>  frame f passed the energy test.  PARITY UNPINNED: auditok is not available
 * to check against; restated from its published source (oracle/vad_oracle.py, tokenize()).
 * Chunks of up to 28672 frames with max_length >= min_length >= 0 run as one workgroup per chunk (k_vad_tokenize_scan:
 * validity and island starts as bit words, markers written island by island; model:
 * oracle/vad_oracle.py::tokenize_chunk_words); anything else as one thread per chunk walking the state machine.
 * Identical outputs, bit for bit.
 * Precision: the labels are float32 and non_speech_label arrives as a float.  With cp / cm the number of start / end
 * markers at or in front of a frame, labels_dev[f] = (float)clip(cp + cm * ((double)non_speech_label - 1), 0, 1),
 * evaluated in fp64 and rounded once: equal to the reference's float64 result for labels float32 holds exactly
 * (0, 0.25, -1), within (cm + 1) * 2^-25 of it otherwise, and the first silence behind a token is
 * (float)non_speech_label itself, as ffs_vad_energy writes it. */
int ffs_vad_tokenize(const float* valid_dev, int64_t n_frames, int64_t chunk_frames, int min_length,
                     int max_length, int max_continuous_silence, float non_speech_label,
                     float* labels_dev, void* hip_stream);

/* ComputeSpeechFrameBoundariesMixin.fit_boundaries (speech_transformers.py:310-317):
 * bounds_dev[0] = first index with frames[i] > 0.5, bounds_dev[1] = last such index;
 * both -1 when there is none.  The comparison is float32's (NaN is not speech): a caller whose values are wider
 * than float32 compares them itself and passes the 0/1 outcome (fit_boundaries does), because a float64 just above
 * 0.5 narrows to 0.5. */
int ffs_speech_bounds(const float* frames_dev, int64_t n_frames, int64_t* bounds_dev,
                      void* hip_stream);

/* ---- subtitle rasteriser (the step immediately before the aligner) ----------
 * SubtitleScaler.fit (subtitle_transformers.py:35-47) followed by SubtitleSpeechTransformer.fit
 * (speech_transformers.py:957-980) for one framerate ratio, from subtitle start/end times given as
 * integer microseconds (datetime.timedelta's resolution) in HOST arrays:
 *   scaled = timedelta(seconds = total_seconds * ratio)         (microsecond rounding, half-even)
 *   start  = int(round((scaled_start - start_seconds) * sample_rate))
 *   end    = start + int(round((scaled_end - scaled_start) * sample_rate))
 *   out[start:end] = 1   (Python slice semantics, union over subtitles; metadata lines skipped)
 * ffs_raster_length = int(max scaled end * sample_rate) + 2 over ALL subtitles (metadata too).
 * The sample value min(1/ratio, 1) (speech_transformers.py:977) is passed to ffs_align_batch as the
 * vector's `hi` level; out_dev holds 0/1 bytes. */
int64_t ffs_raster_length(const int64_t* end_us, int64_t n_subs, double ratio, double sample_rate);
/* Host-only, many vectors at once: len_out[v] = ffs_raster_length of a track whose largest end time is
 * track_end_us_max[v], scaled by ratio[v] (the scaling is monotone, so the largest end decides). */
int ffs_raster_lengths(const int64_t* track_end_us_max, const double* ratio, int64_t n_vec, double sample_rate,
                       int64_t* len_out);
/* Host-only: the clamped [start, end) sample intervals ffs_rasterize_subtitles fills, written as
 * pairs into iv_out[2*n_subs]; returns how many intervals were produced. */
int64_t ffs_raster_intervals(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata,
                             int64_t n_subs, double ratio, double sample_rate, double start_seconds,
                             int64_t out_len, int32_t* iv_out);
int ffs_rasterize_subtitles(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata,
                            int64_t n_subs, double ratio, double sample_rate, double start_seconds,
                            uint8_t* out_dev, int64_t out_len, void* hip_stream);

/* Bit-packed (FFS_DTYPE_U1) variant: out_dev holds ceil(out_len/32) 32-bit words (zeroed, then filled). */
int ffs_rasterize_subtitles_bits(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata,
                                 int64_t n_subs, double ratio, double sample_rate, double start_seconds,
                                 uint32_t* out_dev, int64_t out_len, void* hip_stream);

/* Batched form, interval arithmetic on the device: n_vec bit-packed rasters from one call -- a file's seven framerate
 * ratios, or every vector of a batch of files, written straight into the buffer ffs_align_batch reads.  The subtitle
 * tracks are concatenated in start_us / end_us / is_metadata (host arrays of n_subs_total entries; is_metadata may be
 * NULL); vector v rasterises the subtitles [vec_sub_first[v], vec_sub_first[v] + vec_sub_count[v]) -- several vectors
 * may name the same track -- with times scaled by vec_ratio[v], as vec_len[v] samples (ffs_raster_length) whose bit 0
 * is bit 0 of word out_dev[vec_out_word[v]].  out_dev[0, out_words) is zeroed first.  Same results, bit for bit, as
 * one ffs_rasterize_subtitles_bits call per vector (the arithmetic is IEEE fp64 on both sides).  The host arrays may
 * be freed after return (they are staged in pinned memory; the caller's stream is NOT synchronised); the upload and
 * the rasterisation are enqueued on hip_stream. */
int ffs_rasterize_batch_bits(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata,
                             int64_t n_subs_total, const int64_t* vec_sub_first, const int64_t* vec_sub_count,
                             const double* vec_ratio, const int64_t* vec_out_word, const int64_t* vec_len, int64_t n_vec,
                             double sample_rate, double start_seconds, uint32_t* out_dev, int64_t out_words,
                             void* hip_stream);

/* The same tracks as BOUNDARY LISTS (FFS_DTYPE_RUNS): no bitmap is written -- the union of a track's scaled sample
 * intervals, overlapping and touching subtitles merged, IS the list (samples[start:end] = ... for every subtitle,
 * speech_transformers.py:966-977, then read back as runs).  Vector v's block starts at byte vec_out_off[v] of out_dev
 * (multiple of 8) and has room for vec_cap[v] >= 2 * vec_sub_count[v] + 1 entries (ffs_runs_list_bytes).  Expanded to
 * bits (ffs_runs_to_bits) a list equals ffs_rasterize_batch_bits' raster bit for bit.  Subtitles need not be sorted (a
 * track that is not sorted by start time is sorted in a staging copy); requires start_seconds <= 0 (a positive one can
 * make start samples negative, which Python's slice semantics wrap around: use the bit rasteriser then).
 * start_us / end_us / is_metadata may be DEVICE pointers (all of them): tracks that are rasterised again and again -- the
 * steps of a golden-section search, one subtitle file against many references -- are uploaded once, nothing of them is
 * copied per call; device-resident tracks must already be sorted by start time.  PINNED host tables (hipHostMalloc /
 * hipHostRegister, sorted) are copied to the device straight from the caller's memory, without a staging copy: the caller
 * keeps them alive and unchanged until the stream has passed the call (pageable tables may be freed after return).
 * Replaces: subtitle_transformers.py:35-47 + speech_transformers.py:957-980 for the device-resident pipeline. */
int ffs_rasterize_batch_runs(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata,
                             int64_t n_subs_total, const int64_t* vec_sub_first, const int64_t* vec_sub_count,
                             const double* vec_ratio, const int64_t* vec_out_off, const int64_t* vec_cap,
                             const int64_t* vec_len, int64_t n_vec, double sample_rate, double start_seconds,
                             void* out_dev, int64_t out_bytes, void* hip_stream);

/* Host-only helper of the drop-in classes: the float64 vectors FFTAligner.fit receives (aligners.py:51-57) are
 * two-level activity vectors in practice.  Returns 1 and writes lo = min, hi = max and the samples as bits
 * (bit i = (x[i] == hi); ceil(n/32) words; all zero when hi == lo) when every sample equals one of the two levels
 * and both are finite; returns 0 (words unspecified) otherwise -- such vectors go to the device as floats. */
int ffs_two_level_pack(const double* x, int64_t n, double* lo_out, double* hi_out, uint32_t* words);

/* Two-level vector -> FFS_DTYPE_U1 on the device.  src_dtype FFS_DTYPE_U8: bit = (byte != 0);
 * FFS_DTYPE_F32: bit = (x > threshold), e.g. VAD labels against 0.5 or (lo+hi)/2, decided against the double
 * threshold exactly (the kernel compares with the largest float not above it, which is the same predicate for a
 * float x: float32(0.1) > 0.1 is 1); NaN samples give 0.  Writes ceil(n/32) words; unused high bits of the last
 * word are 0. */
int ffs_pack_bits(const void* src_dev, int src_dtype, int64_t n, double threshold, uint32_t* dst_dev,
                  void* hip_stream);

/* Sparse reference assembly of MultiSegmentVideoSpeechTransformer.fit (speech_transformers.py:871-890):
 * out = zeros(out_len); out[dst_start[i] : dst_start[i]+len[i]] = labels[src_off[i] : src_off[i]+len[i]]
 * for every sampled window i (clipped at out_len, Python slice semantics), in one device pass.
 * seg_* are HOST arrays of n_segments entries; seg_labels_dev holds the windows' VAD labels (it may be null when
 * every window is empty).  Windows of ONE call must not overlap inside [0, out_len): they are copied concurrently
 * and overlapping ones race.  A caller with overlapping windows splits them into calls of non-overlapping runs and
 * applies those in order, later window wins, as the reference's loop does (assemble_sparse_reference). */
int ffs_scatter_segments(const float* seg_labels_dev, const int64_t* seg_src_off, const int64_t* seg_dst_start,
                         const int64_t* seg_len, int n_segments, float* out_dev, int64_t out_len,
                         void* hip_stream);

/* ---- multi-GPU: RCCL all-gather of the per-pair results over xGMI --------------------
 * Problems are sharded by pair, one process per GPU; nothing is exchanged during the solves.  The
 * single collective of the path gathers every rank's n_local 24-byte ffs_pair_result records:
 *   recv_dev[r * n_local + i] = rank r's send_dev[i]      (ncclAllGather, latency-bound)
 * Bootstrap as with NCCL: rank 0 calls ffs_comm_unique_id and publishes the 128 bytes out of band
 * (torch.distributed's store, MPI, a file); every rank then calls ffs_comm_create.  librccl is
 * resolved with dlopen at the first call (the copy already loaded in the process, e.g. torch's).
 * Replaces: nothing in the reference (single process); the per-file call being sharded is
 * ffsubsync.py:230-235. */
typedef struct ffs_comm ffs_comm;
typedef struct ffs_comm_id {
    char internal[128];
} ffs_comm_id;
int ffs_comm_unique_id(ffs_comm_id* id_out);
int ffs_comm_create(int device, int rank, int world_size, const ffs_comm_id* id, ffs_comm** out);
int ffs_gather_results(ffs_comm* comm, const ffs_pair_result* send_dev, int64_t n_local,
                       ffs_pair_result* recv_dev, void* hip_stream);
int ffs_comm_destroy(ffs_comm* comm);

/* Per-kernel timing with HIP events recorded on the caller's stream around every launch of the
 * hot kernels (used by bench.py for the roofline figures).  Kernel ids: */
#define FFS_K_PASS_A 0   /* load/map/pad + column FFT + twiddle                    */
#define FFS_K_MID 1      /* row FFT * conj(ref spectrum), row FFT, twiddle (in place) */
#define FFS_K_PASS_C 2   /* column FFT + lag-window mask + block argmax nominees    */
#define FFS_K_NOMINEES 3 /* nominee gather per candidate                            */
#define FFS_K_RESCORE 4  /* exact re-evaluation of nominee lags                     */
#define FFS_K_RUNS_EXTRACT 5 /* run-boundary path: boundary lists of every vector (reads the bit-packed vectors) */
#define FFS_K_RUNS_CORR 6    /* run-boundary path: exact correlation over the lag window + argmax           */
#define FFS_K_LEVELS 7       /* multi-level float references: level detection + threshold planes (reads the float vectors) */
#define FFS_K_COUNT 8
int ffs_plan_profile(ffs_plan* plan, int enable);
/* Synchronises the recorded events, adds their durations to ms_total[FFS_K_COUNT] /
 * launches[FFS_K_COUNT] (caller-zeroed or accumulating) and clears the recording. */
int ffs_plan_profile_read(ffs_plan* plan, double* ms_total, int64_t* launches);

/* ---- split-aware alignment: piecewise offsets for videos with breaks or cuts (csrc/ffs_split.h) ---------------
 * Replaces: nothing in the reference -- its README names mid-video splits (ad breaks, recaps, cuts the subtitles do not
 * share) as its one algorithmic limitation; FFTAligner finds one offset per file (aligners.py:45-80).  No upstream
 * parity exists: the contract below is pinned against the numpy model tests/split_model.py, bit for bit.
 *
 * One problem = a two-level reference r (R samples, levels ref_lo/ref_hi) and a two-level subtitle vector s (S samples,
 * e.g. the candidate at the chosen framerate ratio), both FFS_DTYPE_U1 in HBM (4-byte aligned).  Blocks of K =
 * block_samples subtitle samples (a multiple of 32 in [256, 32768]); block b = [bK, min((b+1)K, S)), B = ceil(S/K).
 * Lags d in [-W+1, W], W = max_offset_samples (1 <= W, 2W <= 262144): the reference's window without its short-input
 * negative-slice quirk; subtitle sample i meets reference sample i+d.
 * Block score m_b(d): over the samples i of block b with 0 <= i+d < R (others are absent, not zeros) count ov, n11, n1x
 * (subtitle bit set), nx1 (reference bit set); n10 = n1x-n11, n01 = nx1-n11, n00 = ov-n11-n10-n01; with s0/s1/r0/r1 =
 * 2*level-1 in fp64, m = ((n00*(s0*r0) + n01*(s0*r1)) + n10*(s1*r0)) + n11*(s1*r1), every operation rounded on its own
 * (no fused multiply-add).
 * DP: V_0 = m_0; for b >= 1: J = max_d V_{b-1}(d), a_{b-1} = the largest d attaining it, T = J - P,
 * stay_b(d) = V_{b-1}(d) >= T, V_b(d) = (stay_b(d) ? V_{b-1}(d) : T) + m_b(d).  End lag = the largest d attaining
 * max V_{B-1} (= total); backtrack o_{B-1} = end lag, o_{b-1} = stay_b(o_b) ? o_b : a_{b-1}.  P = split_penalty >= 0;
 * +inf never splits (one piece at the windowed argmax of the whole-vector correlation).
 *
 * A plan owns the workspace for pairs_in_flight problems of up to max_samples subtitle samples, max_blocks blocks and
 * max_lags = 2W lags: per pair max_blocks * max_lags * 2 bytes of uint16 counts (170 MB at 2 h, +-10 min, K = 1024) plus
 * one stay bit per (block, lag) and one fp64 row of max_lags.  A plan serves one host thread at a time; successive calls
 * (any streams) are ordered by the library. */
typedef struct ffs_split_plan ffs_split_plan;
int ffs_split_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                          ffs_split_plan** out);
int ffs_split_plan_destroy(ffs_split_plan* plan);
int64_t ffs_split_plan_workspace_bytes(const ffs_split_plan* plan);
/* Solve n_pairs problems (host arrays of n_pairs entries; ref_ptr / sub_ptr hold DEVICE pointers).  Outputs are
 * caller-owned device buffers written in stream order on hip_stream: with max_b = max over the pairs of ceil(S/K),
 * block_offset_out_dev[p * max_b + b] = o_b (int32 lag), block_score_out_dev[p * max_b + b] = m_b(o_b) (entries
 * b >= B_p are written as 0), total_out_dev[p] = max V_{B-1}.  Pieces (maximal runs of equal o_b) are formed by the
 * caller.  FFS_E_EMPTY for a vector of length 0. */
int ffs_align_split_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                          const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                          const double* sub_lo, const double* sub_hi, int64_t block_samples, int64_t max_offset_samples,
                          double split_penalty, int32_t* block_offset_out_dev, double* block_score_out_dev,
                          double* total_out_dev, void* hip_stream);

/* ---- alignment quality report: runner-up peaks and spread of the correlation curve (csrc/ffs_quality.h) ---------
 * Replaces: nothing in the reference -- its only quality signal is the raw score at the winning lag (--min-score,
 * ffsubsync.py:145-174), whose magnitude grows with the file's length and speech density.  The contract below is pinned
 * against the numpy model tests/quality_model.py.
 *
 * One problem = a two-level reference r (R samples, levels ref_lo/ref_hi) and ONE two-level subtitle vector s (S
 * samples), both FFS_DTYPE_U1 in HBM (4-byte aligned), and the lag window max_offset_samples W (>= 0, or -1 for none).
 * Lag set: exactly the entries of the reference's masked `convolve` array that its argmax reads (aligners.py:31-48,
 * Python slice semantics included): d in [-W+1, W] when R, S > W; all N = ffs_fft_length(R, S) entries without a
 * window.  Score of lag d: over the samples i with 0 <= i+d < R, the counts ov, n11, n1x, nx1 scored by the arithmetic
 * of ffs_pair_result.score (so peak 1 equals the solve's record bit for bit); exactly 0.0 where the overlap is empty.
 * Peaks: peak 1 = the window maximum (largest lag on ties); peak k+1 = the maximum over the lags d with |d - d_j| >=
 * exclusion_samples (E >= 1) for every earlier peak j, same tie rule; fewer than top_k (1..8) when no lag is eligible.
 * Moments over the whole lag set (zero-overlap lags included): mean and population std (ddof = 0), two passes; when every
 * score is equal, mean = that score and std = 0 exactly (FFS_QUALITY_FLAT).  An empty window gives n_lags = 0, no peak,
 * and FFS_QUALITY_FLAT | FFS_QUALITY_EMPTY_WINDOW.
 *
 * A plan owns the workspace for pairs_in_flight problems of up to max_samples samples per vector and max_lags lags:
 * per pair max_lags * 12 bytes (uint32 n11 curve + fp64 scores; 144 KB at +-60 s) plus the word prefix popcounts of both
 * vectors.  Calls with more pairs run in sub-batches.  A plan serves one host thread at a time; successive calls (any
 * streams) are ordered by the library. */
#define FFS_QUALITY_FLAT 1         /* every score of the lag set is equal: std = 0 */
#define FFS_QUALITY_EMPTY_WINDOW 2 /* the lag set is empty */

typedef struct ffs_quality_result {
    double peak_score[8];   /* peaks 0 .. n_peaks-1 (entries beyond: 0) */
    int64_t peak_offset[8]; /* samples; subtitle shifted by +offset/sample_rate seconds */
    double mean, std;       /* of the scores over the lag set */
    int64_t n_lags;
    int32_t n_peaks, flags; /* flags: FFS_QUALITY_* */
} ffs_quality_result;
#ifdef __cplusplus
static_assert(sizeof(ffs_quality_result) == 160, "ffs_quality_result is 160 bytes");
#else
_Static_assert(sizeof(ffs_quality_result) == 160, "ffs_quality_result is 160 bytes");
#endif

typedef struct ffs_quality_plan ffs_quality_plan;
int ffs_quality_plan_create(int device, int pairs_in_flight, int64_t max_lags, int64_t max_samples, ffs_quality_plan** out);
int ffs_quality_plan_destroy(ffs_quality_plan* plan);
int64_t ffs_quality_plan_workspace_bytes(const ffs_quality_plan* plan);
/* Report n_pairs problems (host arrays of n_pairs entries; ref_ptr / sub_ptr hold DEVICE pointers) into out_dev[p]
 * (caller-owned device array of n_pairs records, 8-byte aligned), in stream order on hip_stream.  FFS_E_EMPTY for a
 * vector of length 0; FFS_E_INVALID for top_k outside [1, 8], exclusion_samples < 1, max_offset_samples < -1, or a
 * problem beyond the plan's max_samples / max_lags. */
int ffs_align_quality_batch(ffs_quality_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                            const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                            const double* sub_lo, const double* sub_hi, int64_t max_offset_samples, int top_k,
                            int64_t exclusion_samples, ffs_quality_result* out_dev, void* hip_stream);

/* ---- all-pairs quality report from boundary lists: which subtitle belongs to which video (csrc/ffs_match.h) ------
 * Replaces: nothing in the reference.  The records are those of ffs_align_quality_batch, byte for byte; the contract of
 * the lag set, the scores, the moments and the peaks is the section above and is pinned by the same model
 * (tests/quality_model.py; tests/match_model.py states the matrix and the assignment built on it).
 *
 * Inputs: two TABLES of device-resident two-level vectors, n_ref references and n_sub subtitle vectors, each an
 * `ffs_runs_list` block (FFS_DTYPE_RUNS, 8-byte aligned) with its length in samples and its two levels, and n_pairs
 * index pairs (pair_ref[p], pair_sub[p]) in host arrays -- any order, repeats allowed; an N x M call lists all N * M.
 * Output: out_dev[p] = the ffs_quality_result of reference pair_ref[p] against subtitle vector pair_sub[p], equal to
 * what ffs_align_quality_batch writes for the same two vectors as bits, on every `algorithm`.
 *
 * Work per VECTOR, once per call whatever the number of its partners: its bits (one expansion launch over the table) and
 * their word prefix popcounts, into the plan's workspace.  Work per PAIR: the n11 curve over the lag window straight from
 * the two lists (k_runs_curve: ~|P| * |Q| * lags / R boundary coincidences; FFS_MATCH_RUNS), or the bit-parallel count of
 * ffs_align_quality_batch on the per-vector bits (FFS_MATCH_BITS); FFS_MATCH_AUTO picks per pair: lists while
 * |P| * |Q| * FFS_MATCH_AUTO_COST <= R * S / 32 (DESIGN 3.13 has the measurement behind the constant).
 *
 * A plan owns the workspace: per pair in flight max_lags * 12 bytes (uint32 n11 curve + fp64 scores), per vector
 * ~max_samples / 4 bytes (bits + prefixes; 180 KB for a 2 h vector) for up to max_vectors vectors (references and
 * subtitle vectors together).  max_samples < 2^29.  Calls with more pairs run in sub-batches of pairs_in_flight on the
 * caller's stream.  A plan serves one host thread at a time; successive calls (any streams) are ordered by the library.
 *
 * Refused with nothing written to out_dev, each with a message naming the cause: FFS_E_EMPTY for a vector of length 0;
 * FFS_E_INVALID for top_k outside [1, 8], exclusion_samples < 1, max_offset_samples < -1, an unknown algorithm, a null or
 * misaligned block, non-finite levels, n_ref + n_sub > max_vectors, a vector longer than max_samples, a lag set larger
 * than max_lags, a pair index out of range -- all before any device work -- and a truncated list (n >= cap) or one whose
 * header names another length.  The list headers live on the device: the call gathers them into the workspace and waits
 * for that copy (one synchronisation of hip_stream per call) before it launches anything that depends on them. */
#define FFS_MATCH_AUTO 0 /* per pair, from the list lengths */
#define FFS_MATCH_RUNS 1 /* every pair from its boundary lists */
#define FFS_MATCH_BITS 2 /* every pair by the bit-parallel count on the per-vector bits */

typedef struct ffs_match_plan ffs_match_plan;
int ffs_match_plan_create(int device, int pairs_in_flight, int64_t max_lags, int64_t max_samples, int64_t max_vectors,
                          ffs_match_plan** out);
int ffs_match_plan_destroy(ffs_match_plan* plan);
int64_t ffs_match_plan_workspace_bytes(const ffs_match_plan* plan);
int ffs_match_quality_batch(ffs_match_plan* plan, int n_ref, const void* const* ref_list, const int64_t* ref_len,
                            const double* ref_lo, const double* ref_hi, int n_sub, const void* const* sub_list,
                            const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int n_pairs,
                            const int32_t* pair_ref, const int32_t* pair_sub, int64_t max_offset_samples, int top_k,
                            int64_t exclusion_samples, int algorithm, ffs_quality_result* out_dev, void* hip_stream);

/* ---- per-piece quality report of a split solve: break evidence (csrc/ffs_split_report.h) -------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/split_report_model.py.
 *
 * The split solve of ffs_align_split_batch (same arguments, same block_offset / block_score / total outputs bit for
 * bit), then per pair its pieces -- maximal runs [f_i, e_i) of equal block offsets, subtitle samples
 * [f_i K, min(e_i K, S)), offset o_i -- in report_out_dev[p * max_b + i] (max_b = the call's largest block count, as for
 * the block outputs; records past the piece count are zero) and the piece count in n_pieces_out_dev[p].
 * Piece curve c_i(d), d in [-W+1, W]: over the piece's samples j with 0 <= j+d < R, the counts ov, n1x, nx1 and
 * n11 (the exact sum of the piece's block counts), scored ((n00*c00 + n01*c01) + n10*c10) + n11*c11 in fp64 with every
 * operation rounded on its own (the block scores' arithmetic); exactly 0.0 where the overlap is empty.  Moments over the
 * 2W lags (two passes, population std) and up to top_k greedy peaks with exclusion distance E, largest lag on ties, as
 * ffs_quality_result (FFS_QUALITY_FLAT when every score is equal).  own_score = c_i(o_i); prev_score = c_i(o_{i-1}),
 * next_score = c_i(o_{i+1}), NaN without that neighbour.  FFS_PIECE_OWN_NOT_PEAK: peak 1 is not at o_i.
 *
 * The first report call on a plan adds a workspace of one uint32 n11 row per block and lag (2x the block counts:
 * max_blocks * max_lags * 4 bytes per pair in flight), counted by ffs_split_plan_workspace_bytes from then on; plans
 * that never report keep the split workspace alone. */
#define FFS_PIECE_OWN_NOT_PEAK 4   /* the piece's peak 1 is not at its own offset */

typedef struct ffs_piece_report {
    int64_t first_block, end_block;   /* blocks [first_block, end_block) */
    int64_t start_sample, end_sample; /* subtitle samples [start_sample, end_sample) */
    int64_t offset;                   /* the piece's offset o_i (samples) */
    double own_score;                 /* c_i(o_i) */
    double prev_score, next_score;    /* c_i(o_{i-1}), c_i(o_{i+1}); NaN without that neighbour */
    double mean, std;                 /* of c_i over the 2W lags */
    int64_t n_lags;                   /* 2W */
    double peak_score[8];             /* peaks 0 .. n_peaks-1 (entries beyond: 0) */
    int64_t peak_offset[8];           /* samples */
    int32_t n_peaks, flags;           /* flags: FFS_QUALITY_FLAT, FFS_QUALITY_EMPTY_WINDOW, FFS_PIECE_OWN_NOT_PEAK */
} ffs_piece_report;
#ifdef __cplusplus
static_assert(sizeof(ffs_piece_report) == 224, "ffs_piece_report is 224 bytes");
#else
_Static_assert(sizeof(ffs_piece_report) == 224, "ffs_piece_report is 224 bytes");
#endif

/* ffs_align_split_batch plus the piece reports, in one call on hip_stream.  report_out_dev: n_pairs * max_b records
 * (8-byte aligned); n_pieces_out_dev: n_pairs int32.  FFS_E_INVALID / FFS_E_EMPTY as ffs_align_split_batch, and
 * FFS_E_INVALID for top_k outside [1, 8], exclusion_samples < 1 or a null / misaligned report output; all before any
 * launch. */
int ffs_align_split_report_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int top_k, int64_t exclusion_samples,
                                 int32_t* block_offset_out_dev, double* block_score_out_dev, double* total_out_dev,
                                 ffs_piece_report* report_out_dev, int32_t* n_pieces_out_dev, void* hip_stream);

/* ---- sample-exact break refinement after a split solve (csrc/ffs_split_refine.h) ----------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/split_refine_model.py.
 *
 * The split DP puts every break on a block boundary.  Per pair (the vectors as ffs_align_split_batch takes them, its
 * block offsets o_b in block_offset_dev[p * max_b + b], max_b = the call's largest ceil(S/K)): breaks are the blocks f_j
 * (j = 1..n) with o_{f_j} != o_{f_j - 1}, cut c_j = f_j K, between o_a = o_{f_j - 1} and o_b = o_{f_j}; c_0 = 0,
 * c_{n+1} = S.  Window [L_j, U_j]: L_j = max(c_j - Rr, j == 1 ? 0 : floor((c_{j-1} + c_j) / 2)),
 * U_j = min(c_j + Rr, j == n ? S : floor((c_j + c_{j+1}) / 2)), Rr = radius_samples in [1, FFS_REFINE_MAX_RADIUS].
 * A(t) = the split's two-level score ((n00*c00 + n01*c01) + n10*c10) + n11*c11 of subtitle samples [L, t) at lag o_a,
 * B(t) = that of [t, U) at lag o_b (samples whose partner lies outside the reference are absent).  Null score
 * z_x = s~_x * rbar + beta * |s~_x|, s~_x = 2 lvl_s[x] - 1, rbar = ((R - P1) * r~_0 + P1 * r~_1) / R with P1 the
 * reference's popcount and r~_y = 2 lvl_r[y] - 1; N(t) = n0 * z0 + n1 * z1 over [L, t).  F(t) = A(t) - N(t),
 * G(t) = N(t) + B(t).  t2 = the smallest maximiser over [L, U] of G(t) + max_{L <= t' <= t} F(t'); t1 = the smallest
 * maximiser of F on [L, t2].  beta = unmatched_margin >= 0 (finite), or NaN for a single cut: t1 = t2 = the smallest
 * maximiser of A(t) + B(t).  Every value is fp64 with each operation rounded on its own.  Subtitle samples before t1
 * keep o_a, samples in [t1, t2) match neither neighbour, samples from t2 on take o_b.
 *
 * Records: out_dev[p * max_b + j] for j < n (records past the count are zero), the count in n_breaks_out_dev[p].
 * The call uses the split plan's pairs_in_flight for its sub-batches and none of its split workspace; the first refine
 * call on a plan adds a few hundred bytes per pair in flight, counted by ffs_split_plan_workspace_bytes from then on. */
#define FFS_REFINE_MAX_RADIUS 131072
#define FFS_REFINE_CLIPPED 1   /* the window was narrowed by a neighbouring break's midpoint */
#define FFS_REFINE_AT_EDGE 2   /* t1 = L > 0 or t2 = U < S: the radius may be too small */
#define FFS_REFINE_UNMATCHED 4 /* t1 < t2 */

typedef struct ffs_break_refine {
    int64_t block, cut;               /* f_j and c_j = f_j K */
    int64_t lo, hi;                   /* the window [L, U] */
    int64_t t1, t2;                   /* the cut points, L <= t1 <= t2 <= U */
    int64_t offset_prev, offset_next; /* o_a, o_b (samples) */
    double coarse_score;              /* A(c) + B(c): the block cut's score */
    double refined_score;             /* F(t1) + G(t2); A(t1) + B(t1) for a single cut */
    int32_t flags, reserved;          /* flags: FFS_REFINE_*; reserved = 0 */
} ffs_break_refine;
#ifdef __cplusplus
static_assert(sizeof(ffs_break_refine) == 88, "ffs_break_refine is 88 bytes");
#else
_Static_assert(sizeof(ffs_break_refine) == 88, "ffs_break_refine is 88 bytes");
#endif

/* Refine the breaks of n_pairs split solves on hip_stream (host arrays of n_pairs entries; ref_ptr / sub_ptr and
 * block_offset_dev are DEVICE pointers).  out_dev: n_pairs * max_b records (8-byte aligned); n_breaks_out_dev: n_pairs
 * int32.  FFS_E_INVALID / FFS_E_EMPTY as ffs_align_split_batch (no limit from the plan's sizes), and FFS_E_INVALID for a
 * radius outside [1, FFS_REFINE_MAX_RADIUS], a negative or infinite margin, or a null / misaligned output; all before
 * any launch, the outputs untouched. */
int ffs_split_refine_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                           const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                           const double* sub_lo, const double* sub_hi, int64_t block_samples,
                           const int32_t* block_offset_dev, int64_t radius_samples, double unmatched_margin,
                           ffs_break_refine* out_dev, int32_t* n_breaks_out_dev, void* hip_stream);

/* ---- sample-exact jumps of a drift solve (csrc/ffs_drift_refine.h) ------------------------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/drift_refine_model.py.
 *
 * ffs_split_refine_batch's contract (the windows, N, F, G, beta = NaN for a single cut, the tie rules,
 * coarse_score = A(c) + B(c), the flags, the 88-byte record, the zeroed tail, the count, the refusals) for a path that
 * changes offset inside its segments -- the block offsets o_b and jump flags of ffs_align_drift_batch,
 * ffs_align_drift_range_batch or a smooth fit (block_jump_dev[p * max_b + b], uint8) -- with two changes:
 *   Jumps, not offset changes.  The refined positions are the blocks f_j >= 1 with block_jump[f_j] != 0, whether or not
 *   the offset changes there (a fitted path may have equal offsets on both sides); block_jump[0] is ignored.
 *   Lags follow the path.  For a subtitle sample x of the window, b(x) = floor(x / K): lag_a(x) = o[min(b(x), f_j - 1)]
 *   and lag_b(x) = o[max(b(x), f_j)] -- each segment's own per-block lag where the segment exists, held at the segment's
 *   last (first) block's value on the far side of the coarse cut.  The windows are clipped at the midpoints to the
 *   neighbouring jumps, so only these two segments' blocks are read.  A(t) = split_mix of the integer sums
 *   (ov, n11, n1x, nx1) over x in [L, t) at lag_a(x), B(t) the same over [t, U) at lag_b(x); a sample whose partner
 *   x + lag(x) lies outside [0, R) is absent.
 * In the record offset_prev = o[f_j - 1] and offset_next = o[f_j].  Lags are any int32; the call takes no window, so it
 * serves the windowed and the range solves alike.  For block offsets that are constant inside every segment, with
 * block_jump set exactly where the offset changes, records and counts are byte-identical to ffs_split_refine_batch's.
 *
 * The call runs on the split plan as ffs_split_refine_batch does (its pairs_in_flight and the same few hundred bytes per
 * pair in flight, made by the first call of either kind; none of the split workspace).  FFS_E_INVALID / FFS_E_EMPTY as
 * ffs_split_refine_batch, and FFS_E_INVALID for a null block_jump_dev; all before any launch, the outputs untouched. */
int ffs_drift_refine_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                           const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                           const double* sub_lo, const double* sub_hi, int64_t block_samples,
                           const int32_t* block_offset_dev, const uint8_t* block_jump_dev, int64_t radius_samples,
                           double unmatched_margin, ffs_break_refine* out_dev, int32_t* n_jumps_out_dev, void* hip_stream);

/* ---- per-cue evidence report (csrc/ffs_cue_report.h) ----------------------------------------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/cue_model.py.
 *
 * Every sync ends in cue times; this call reports on each cue by itself.  Per pair: the vectors as
 * ffs_split_refine_batch takes them, and cue_count[p] entries of the device table cue_dev from entry cue_first[p] on:
 * start / end in samples of s, lag = the offset the sync applied to that cue.  Cues may be unsorted, may overlap and may
 * number zero; their contents are not validated on the host and may be any int64.  Per cue: a = clamp(start, 0, S),
 * e = clamp(end, 0, S); e <= a sets FFS_CUE_EMPTY, |lag| > 2^31 sets FFS_CUE_INVALID, and in both cases the record
 * holds start, end, lag and the flags, everything else zero.  Otherwise the window is L = max(0, a - m),
 * U = min(S, e + m), m = context_samples in [0, FFS_CUE_MAX_CONTEXT], and for every delta in [-rho, rho],
 * rho = radius_samples in [0, FFS_CUE_MAX_RADIUS], with d = lag + delta:
 *   window counts ov, n11, n1x (s = 1), nx1 (r = 1) over subtitle samples i in [L, U) whose partner i + d lies in
 *   [0, R) (other samples are absent, as in the split); c(delta) = ((n00*c00 + n01*c01) + n10*c10) + n11*c11, fp64, each
 *   operation rounded on its own;
 *   cue counts cov(delta), c11(delta): the partners inside the reference and the reference ones over i in [a, e).
 * best_delta maximises c, cue_max_delta maximises c11; ties go to the smallest |delta|, then to +delta over -delta.
 * n_best = the number of delta with c(delta) equal to the maximum (fp64 equality).
 *
 * Records: out_dev[k] for table entry k, for every entry inside a pair's range (other entries are not written).  The
 * call uses the split plan's pairs_in_flight for its sub-batches and none of its split workspace; the first cue report
 * call on a plan adds one descriptor block per pair in flight, counted by ffs_split_plan_workspace_bytes from then on. */
#define FFS_CUE_MAX_RADIUS 4096
#define FFS_CUE_MAX_CONTEXT 65536
#define FFS_CUE_EMPTY 1        /* e <= a */
#define FFS_CUE_INVALID 2      /* |lag| > 2^31 */
#define FFS_CUE_NO_OVERLAP 4   /* ov = 0 at delta = 0 */
#define FFS_CUE_BEST_AT_EDGE 8 /* rho > 0 and |best_delta| = rho */
#define FFS_CUE_FLAT 16        /* rho > 0 and n_best = 2 rho + 1 */
#define FFS_CUE_SILENT 32      /* cue_max_n11 = 0: no reference speech under the cue at any lag within rho */

typedef struct ffs_cue {
    int64_t start, end; /* [start, end) in samples of s */
    int64_t lag;        /* the offset applied to the cue (samples) */
} ffs_cue;

typedef struct ffs_cue_report {
    int64_t start, end;        /* as given */
    int64_t lo, hi;            /* the window [L, U) */
    int64_t lag;               /* as given */
    int32_t own[4];            /* ov, n11, n1x, nx1 at delta = 0 */
    int32_t best[4];           /* the same at best_delta */
    double own_score;          /* c(0) */
    double best_score;         /* c(best_delta) */
    int32_t best_delta, n_best;
    int32_t cue_own_n11, cue_own_ov;      /* c11(0), cov(0) */
    int32_t cue_max_n11, cue_max_delta;   /* max c11 and where */
    int32_t flags, reserved;   /* flags: FFS_CUE_*; reserved = 0 */
} ffs_cue_report;
#ifdef __cplusplus
static_assert(sizeof(ffs_cue) == 24, "ffs_cue is 24 bytes");
static_assert(sizeof(ffs_cue_report) == 120, "ffs_cue_report is 120 bytes");
#else
_Static_assert(sizeof(ffs_cue) == 24, "ffs_cue is 24 bytes");
_Static_assert(sizeof(ffs_cue_report) == 120, "ffs_cue_report is 120 bytes");
#endif

/* Report on the cues of n_pairs pairs on hip_stream (host arrays of n_pairs entries; ref_ptr / sub_ptr, cue_dev and
 * out_dev are DEVICE pointers, 8-byte aligned; n_cues = the entries of the table and of out_dev).  FFS_E_INVALID /
 * FFS_E_EMPTY as ffs_split_refine_batch, and FFS_E_INVALID for a radius or context out of range, a negative count, a
 * range outside the table, or a null / misaligned table or output when there is a cue to report; all before any launch,
 * the output untouched.  n_pairs = 0 or zero cues in total is not an error. */
int ffs_cue_report_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                         const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                         const double* sub_lo, const double* sub_hi, const ffs_cue* cue_dev, int64_t n_cues,
                         const int64_t* cue_first, const int64_t* cue_count, int64_t radius_samples,
                         int64_t context_samples, ffs_cue_report* out_dev, void* hip_stream);

/* ---- joint cue retiming: order-preserving per-cue shifts (csrc/ffs_cue_retime.h) -----------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/retime_model.py and
 * the enumeration of every path in tests/retime_reference.py.
 *
 * One residual shift delta_k in [-rho, rho] per cue, chosen jointly by a Viterbi pass over (cue x shift).  Inputs per
 * pair exactly as ffs_cue_report_batch; THE TABLE ORDER IS THE CHAIN ORDER (pass cues in file order).  Everything is
 * exact integer arithmetic.  Live and skipped cues: a = clamp(start, 0, S), e = clamp(end, 0, S); e <= a sets
 * FFS_RETIME_EMPTY, |lag| > 2^31 sets FFS_RETIME_INVALID; such a cue is skipped (its record holds start, end, lag and
 * the flag, everything else zero; it takes no part in the chain; its neighbours link to each other).  The other cues
 * are live, 1..K in table order.  Node score: the window and the counts ov, n11, n1x, nx1 at d = lag + delta are
 * ffs_cue_report_batch's (m = context_samples), and A_k(delta) = ov - 2 n1x - 2 nx1 + 4 n11, the agreeing minus the
 * disagreeing samples that have a partner: c(delta) at levels (0,1)/(0,1).  THE PAIR'S LEVELS DO NOT ENTER THE RETIME
 * (they are checked as ffs_cue_report_batch checks them and otherwise unused): a max-plus recurrence over a thousand
 * fp64 sums cannot be pinned against an independent optimum, integers can.  u_k(delta) = 64 A_k(delta).
 * Link from live cue k-1 (shift d') to live cue k (shift d): w = penalty_q |d - d'|, and with jump_q >= 0
 * w = min(w, jump_q) (both in 64ths of a score sample, FFS_RETIME_Q); g_k = (a_k + lag_k) - (a_{k-1} + lag_{k-1}); with
 * FFS_RETIME_KEEP_ORDER and g_k >= 0 only d' <= d + g_k is admissible (the shifted start of cue k is not before that of
 * cue k-1); with g_k < 0 or without the flag every d' is; with the flag, g_k < 0 sets FFS_RETIME_UNORDERED on cue k.
 *   V_1(d) = u_1(d);  V_k(d) = u_k(d) + max over admissible d' of (V_{k-1}(d') - w(d', d))   (int64)
 * The backpointer is the maximising d'; delta_K = argmax V_K; every tie goes to the option order on the candidate
 * itself: the smallest |.|, then + over -.  The path delta_1..delta_K is the backtrack from delta_K.
 * Invariants: own_total <= total <= best_total, and total = 64 * sum(at) - sum(link).
 *
 * Records: out_dev[k] for table entry k, for every entry inside a pair's range (other entries are not written);
 * summary_out_dev[p] for every pair (all zeros for a pair without a live cue).
 *
 * Stream and workspace: the call runs on the split plan as ffs_cue_report_batch does (asynchronous on hip_stream; the
 * plan orders its calls among themselves).  It uses none of the split workspace.  The first retime call adds one
 * descriptor block per pair in flight; every call whose largest sub-batch needs more than the plan holds grows the
 * retime workspace to 6 bytes per (cue, delta) of that sub-batch (an int32 profile and an int16 backpointer), rounded
 * up to 256 bytes: growing waits for the plan's earlier calls and allocates, so such a call cannot be captured into a
 * graph.  Both are counted by ffs_split_plan_workspace_bytes from then on.  Sub-batches are cut so that the pair count
 * stays within pairs_in_flight and the workspace within FFS_RETIME_WORK_CAP (a sub-batch takes pairs in order while
 * both hold). */
#define FFS_RETIME_MAX_RADIUS 1024
#define FFS_RETIME_Q 64
#define FFS_RETIME_NO_JUMP (-1)
#define FFS_RETIME_WORK_CAP (256ll << 20) /* bytes of retime workspace one sub-batch may use (256 MiB) */
#define FFS_RETIME_KEEP_ORDER 1   /* call flag */
#define FFS_RETIME_EMPTY 1        /* e <= a */
#define FFS_RETIME_INVALID 2      /* |lag| > 2^31 */
#define FFS_RETIME_MOVED 4        /* delta != 0 */
#define FFS_RETIME_JUMP 8         /* jump_q >= 0 and penalty_q |delta - delta'| > jump_q on the incoming link */
#define FFS_RETIME_UNORDERED 16   /* KEEP_ORDER and g_k < 0 */
#define FFS_RETIME_ORDER_TIGHT 32 /* the order constraint is active and delta_{k-1} = delta_k + g_k */
#define FFS_RETIME_AT_EDGE 64     /* rho > 0 and |delta| = rho */

typedef struct ffs_cue_retime {
    int64_t start, end, lag;   /* the cue as given */
    int32_t delta;             /* delta_k */
    int32_t flags;             /* FFS_RETIME_* */
    int32_t own;               /* A_k(0) */
    int32_t at;                /* A_k(delta_k) */
    int32_t best;              /* max over delta of A_k */
    int32_t best_delta;        /* where, in the option order */
    int64_t link;              /* w paid on the link into this cue; 0 for the first live cue */
    int32_t reserved[2];       /* zero */
} ffs_cue_retime;

typedef struct ffs_retime_summary {
    int64_t total;             /* V_K(delta_K) */
    int64_t own_total;         /* 64 * sum of A_k(0) */
    int64_t best_total;        /* 64 * sum of max A_k */
    int32_t n_live, n_moved, n_jumps, reserved;
} ffs_retime_summary;
#ifdef __cplusplus
static_assert(sizeof(ffs_cue_retime) == 64, "ffs_cue_retime is 64 bytes");
static_assert(sizeof(ffs_retime_summary) == 40, "ffs_retime_summary is 40 bytes");
#else
_Static_assert(sizeof(ffs_cue_retime) == 64, "ffs_cue_retime is 64 bytes");
_Static_assert(sizeof(ffs_retime_summary) == 40, "ffs_retime_summary is 40 bytes");
#endif

/* Retime the cues of n_pairs pairs on hip_stream (host arrays of n_pairs entries; ref_ptr / sub_ptr, cue_dev, out_dev and
 * summary_out_dev are DEVICE pointers, 8-byte aligned; n_cues = the entries of the table and of out_dev;
 * summary_out_dev holds n_pairs entries).  radius_samples in [0, FFS_RETIME_MAX_RADIUS], context_samples in
 * [0, FFS_CUE_MAX_CONTEXT], penalty_q in [0, 2^20], jump_q = FFS_RETIME_NO_JUMP or in [0, 2^40], flags = 0 or
 * FFS_RETIME_KEEP_ORDER.  Refusals, all before any launch with both outputs untouched: everything
 * ffs_cue_report_batch refuses; FFS_E_INVALID for a radius, context, penalty_q or jump_q out of range, unknown flag
 * bits, a null or misaligned summary output, and a pair whose own cue_count * (2 radius + 1) * 6 bytes exceed
 * FFS_RETIME_WORK_CAP (named in the message).  Cue contents are never validated on the host.  n_pairs = 0 is not an
 * error; with zero cues in total the summaries are still written (cue_dev and out_dev may then be null). */
int ffs_cue_retime_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                         const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                         const double* sub_lo, const double* sub_hi, const ffs_cue* cue_dev, int64_t n_cues,
                         const int64_t* cue_first, const int64_t* cue_count, int64_t radius_samples,
                         int64_t context_samples, int64_t penalty_q, int64_t jump_q, int flags, ffs_cue_retime* out_dev,
                         ffs_retime_summary* summary_out_dev, void* hip_stream);

/* ---- split-aware alignment over any lag range: subtitles for another cut of the video (csrc/ffs_split_range.h) -----
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/cut_model.py.
 *
 * ffs_align_split_batch's contract (block counts with absent samples, the no-FMA fp64 score, the DP, its tie rules and
 * backtrack, the output layout) with the lag set d in [lag_lo_p, lag_hi_p] per pair instead of [-W+1, W]: any
 * lag_lo <= lag_hi inside the int32 range, not clipped to the overlap range [-(S-1), R-1]; lags without overlap score 0.
 * At [-W+1, W] the records are bit-identical to ffs_align_split_batch's.
 *
 * One lag row is spread over many workgroups: one launch per block step covers every pair in flight, and block counts
 * are computed inside the step, never stored.  A plan owns the workspace for pairs_in_flight (<= 65535) problems with up
 * to max_samples samples in EITHER vector (<= 2^30 - 1), max_blocks blocks and max_lags lags (<= 2^31 - 1): per pair
 * one stay bit per (block, lag) (127 MB at 2 h against 2 h over the full range, K = 1024), one fp64 row of max_lags,
 * the word prefixes of both vectors and a few bytes per 2048 lags.  A plan serves one host thread at a time; successive
 * calls (any streams) are ordered by the library. */
typedef struct ffs_split_range_plan ffs_split_range_plan;
int ffs_split_range_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                                ffs_split_range_plan** out);
int ffs_split_range_plan_destroy(ffs_split_range_plan* plan);
int64_t ffs_split_range_plan_workspace_bytes(const ffs_split_range_plan* plan);
/* ffs_align_split_batch with host arrays lag_lo / lag_hi (n_pairs entries) in place of max_offset_samples; the same
 * outputs (block_offset_out_dev[p * max_b + b] = o_b as an int32 lag).  FFS_E_INVALID / FFS_E_EMPTY for the arguments
 * ffs_align_split_batch refuses, a range with lag_lo > lag_hi, outside the int32 range or wider than max_lags, or a
 * vector longer than max_samples; all before any launch, the outputs untouched. */
int ffs_align_split_range_batch(ffs_split_range_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                const int64_t* lag_lo, const int64_t* lag_hi, double split_penalty,
                                int32_t* block_offset_out_dev, double* block_score_out_dev, double* total_out_dev,
                                void* hip_stream);

/* ---- per-piece report of a split over any lag range (csrc/ffs_cut_report.h) ---------------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/cut_report_model.py.
 *
 * ffs_align_split_report_batch's piece records for the block offsets of a split solve (block_offset_dev[p * max_b + b],
 * as ffs_align_split_range_batch writes them, every o_b inside [lag_lo_p, lag_hi_p]) over the lag set
 * d in [lag_lo_p, lag_hi_p] instead of [-W+1, W]: each piece's curve has n11 counted exactly from the bits, lags without
 * overlap score exactly 0.0 and count, and n_lags = lag_hi - lag_lo + 1.  At [-W+1, W], given the windowed split's block
 * offsets, the records are bit-identical to ffs_align_split_report_batch's.  report_out_dev: n_pairs * max_b records
 * (8-byte aligned; records past the count zero); n_pieces_out_dev: n_pairs int32.
 *
 * The call reads the block offsets back once (it waits for hip_stream's earlier work) to check them and to schedule its
 * rounds; the kernels run on hip_stream.  Pieces are reported 8 per pair and round, so the first report call on a plan
 * adds pairs_in_flight * 8 uint32 rows of max_lags plus a small work-item table, whatever the piece count; it is counted
 * by ffs_split_range_plan_workspace_bytes from then on.  FFS_E_INVALID / FFS_E_EMPTY as ffs_align_split_range_batch,
 * and FFS_E_INVALID for top_k outside [1, 8], exclusion_samples < 1, a null / misaligned offset or report pointer, or a
 * block offset outside its pair's range; all before any launch, the outputs untouched. */
int ffs_split_range_report_batch(ffs_split_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                 const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                 const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                 const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                 const int64_t* lag_hi, const int32_t* block_offset_dev, int top_k,
                                 int64_t exclusion_samples, ffs_piece_report* report_out_dev,
                                 int32_t* n_pieces_out_dev, void* hip_stream);

/* ---- drift-tolerant alignment: the split DP with small offset steps between blocks (csrc/ffs_drift.h) -------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model tests/drift_model.py, bit
 * for bit.
 *
 * ffs_align_split_batch's problem, blocks, lag window and block scores m_b(d), unchanged.  The DP may also take a
 * block's offset from a NEIGHBOURING lag of the block before it: a residual framerate ratio or a slowly wandering clock
 * moves the offset by a sample or two per block, which a jump (P for any change) cannot follow.  With s = max_step in
 * [0, 7], Q = step_cost (finite, >= 0), c_a = Q * a (one fp64 product), lag index j in [0, L), L = 2W:
 * V_0 = m_0; for b >= 1: J = max_j V_{b-1}(j), a_{b-1} = the largest j attaining it, T = J - P, and per j
 *     best, code = V_{b-1}(j), STAY
 *     for a = 1..s, for e in (+a, -a): if 0 <= j-e < L and V_{b-1}(j-e) - c_a > best: best, code = that, e
 *     if T > best: best, code = T, JUMP
 *     V_b(j) = best + m_b(j)
 * (every comparison strict: ties keep the earlier option; every fp64 operation rounded on its own, no fused
 * multiply-add).  End = the largest j attaining max V_{B-1} (= total); backtrack o_{b-1} = a_{b-1} after JUMP, else
 * o_b - e.  At max_step = 0 every output equals ffs_align_split_batch's bit for bit.
 *
 * A plan owns the workspace for pairs_in_flight problems of up to max_samples subtitle samples, max_blocks blocks and
 * max_lags = 2W lags: per pair max_blocks * max_lags * 2 bytes of uint16 counts plus a 4-bit code per (block, lag)
 * (max_blocks * max_lags / 2 bytes) and two fp64 rows of max_lags (211 MB at 2 h, +-10 min, K = 1024).  A plan of its
 * own: split plans do not grow.  A plan serves one host thread at a time; successive calls (any streams) are ordered
 * by the library. */
typedef struct ffs_drift_plan ffs_drift_plan;
int ffs_drift_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                          ffs_drift_plan** out);
int ffs_drift_plan_destroy(ffs_drift_plan* plan);
int64_t ffs_drift_plan_workspace_bytes(const ffs_drift_plan* plan);
/* Solve n_pairs problems; arguments, limits, errors and sub-batching as ffs_align_split_batch, and FFS_E_INVALID for
 * max_step outside [0, 7] or a step_cost that is negative, NaN or infinite (all before any launch).  Outputs as
 * ffs_align_split_batch's (block_offset_out_dev, block_score_out_dev: n_pairs * max_b; total_out_dev: n_pairs) plus
 * block_jump_out_dev[p * max_b + b] (uint8): 1 where block b >= 1 was entered by JUMP, else 0 (block 0 and entries
 * b >= B_p are 0) -- a jump and a step can give the same offset difference, so the flag is an output.  Segments (maximal
 * runs of blocks with no jump inside) are formed by the caller. */
int ffs_align_drift_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                          const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                          const double* sub_lo, const double* sub_hi, int64_t block_samples, int64_t max_offset_samples,
                          double split_penalty, int max_step, double step_cost, int32_t* block_offset_out_dev,
                          double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                          void* hip_stream);

/* ---- drift-tolerant alignment over any lag range: another cut AND a residual ratio (csrc/ffs_drift_range.h) --------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model
 * tests/drift_range_model.py, bit for bit.
 *
 * ffs_align_drift_batch's DP over ffs_align_split_range_batch's lag set: d in [lag_lo_p, lag_hi_p] per pair, lag index
 * j = d - lag_lo, L = lag_hi - lag_lo + 1, any contiguous int32 range, not clipped to the overlap range; the block scores
 * m_b(j) are the range split's (absent samples, the no-FMA fp64 score; lags without overlap score 0).  Per block b >= 1
 * and lag index j the options are tried in the order STAY; +1, -1, ..., +s, -s (each needing 0 <= j - e < L and costing
 * c_a = Q * a, one fp64 product); JUMP to T = J_{b-1} - P, each replacing the best so far only when strictly greater; the
 * largest lag index wins every maximum; backtrack and block_jump as ffs_align_drift_batch.  s = max_step in [0, 7],
 * Q = step_cost finite and >= 0.  Two identities: at max_step = 0 offsets, scores and total equal
 * ffs_align_split_range_batch's bit for bit (block_jump[b] = 1 exactly where the offset changes); at [-W+1, W] all four
 * outputs equal ffs_align_drift_batch's bit for bit.
 *
 * One launch per block step covers every pair in flight, as the range split; a cell reads its neighbours of the previous
 * row, so a pair keeps TWO fp64 rows of max_lags, and a code per (block, lag) in bit planes: ceil(log2(2s + 2)) planes
 * for a plan made with max_step_cap = s (1 at 0, 2 at 1, 3 at 2..3, 4 at 4..7), max_blocks * max_lags / 8 bytes each
 * (127 MB per plane at 2 h against 2 h over the full range, K = 1024: 380 MB at max_step_cap 2).  A call at a smaller
 * max_step writes only the planes it needs.  A plan of its own: split range and drift plans do not grow.  Limits as
 * ffs_split_range_plan_create, and max_step_cap in [0, 7].  A plan serves one host thread at a time; successive calls
 * (any streams) are ordered by the library. */
typedef struct ffs_drift_range_plan ffs_drift_range_plan;
int ffs_drift_range_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                                int max_step_cap, ffs_drift_range_plan** out);
int ffs_drift_range_plan_destroy(ffs_drift_range_plan* plan);
int64_t ffs_drift_range_plan_workspace_bytes(const ffs_drift_range_plan* plan);
/* ffs_align_split_range_batch's arguments plus max_step, step_cost and block_jump_out_dev (uint8, n_pairs * max_b, as
 * ffs_align_drift_batch writes it); sub-batches of pairs_in_flight on hip_stream.  FFS_E_INVALID / FFS_E_EMPTY for
 * everything ffs_align_split_range_batch refuses, max_step outside [0, max_step_cap], or a step_cost that is negative,
 * NaN or infinite; all before any launch, the outputs untouched. */
int ffs_align_drift_range_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                const int64_t* lag_lo, const int64_t* lag_hi, double split_penalty, int max_step,
                                double step_cost, int32_t* block_offset_out_dev, double* block_score_out_dev,
                                uint8_t* block_jump_out_dev, double* total_out_dev, void* hip_stream);

/* ---- per-segment path report of a drift solve: segment, jump and drift evidence (csrc/ffs_drift_report.h) ----------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model
 * tests/drift_report_model.py, bit for bit.
 *
 * The drift solve of ffs_align_drift_batch (same arguments, same block_offset / block_score / block_jump / total outputs
 * bit for bit), then per pair its segments -- maximal runs [f_i, e_i) of blocks with no jump inside, subtitle samples
 * [f_i K, min(e_i K, S)), block offsets o_b, o_min / o_max over the run -- in report_out_dev[p * max_b + i] (records past
 * the segment count are zero) and the segment count in n_segments_out_dev[p].
 * Shift set delta in [-W+1-o_min, W-o_max]: exactly the shifts for which every block's lag o_b + delta stays inside the
 * window; it always holds 0, n_lags = 2W - (o_max - o_min) >= 1.  Path curve p_i(delta): for block b at lag
 * d = o_b + delta, a = max(bK, -d), e = min((b+1)K, S, R-d); where e > a, ov = e - a, n1x = ones of s in [a, e), nx1 = ones
 * of r in [a+d, e+d), n11 = the drift solve's uint16 block count (else all 0); the four are summed over the segment's
 * blocks as exact integers and scored ONCE, ((n00*c00 + n01*c01) + n10*c10) + n11*c11 in fp64 with every operation
 * rounded on its own; exactly 0.0 where the summed overlap is 0.  (own_score is therefore not in general the sum of the
 * block scores -- different rounding; with 0/1 levels every term is an integer and they are equal.)  Moments over the
 * n_lags shifts (two passes, population std) and up to top_k greedy peaks with exclusion distance E, largest shift on
 * ties, as ffs_quality_result; peaks are reported as shifts, 0 being the path itself.
 * own_score = p_i(0); prev_score = p_i(last_offset_{i-1} - first_offset_i) -- the path moved so that it continues the
 * previous segment without a jump -- and next_score = p_i(first_offset_{i+1} - last_offset_i); NaN without that
 * neighbour or when that shift lies outside the shift set.  flat_score = max over d in [o_min, o_max] of the constant-lag
 * piece curve of the segment's samples (ffs_piece_report's c at d, n11 = the uint32 sum of the segment's block counts),
 * flat_offset the largest d attaining it: the best the segment can do without drifting.
 * At max_step = 0 every segment is a piece and its record equals ffs_align_split_report_batch's in every shared field
 * (peak_shift + offset = peak_offset), flat_score has the bits of own_score and flat_offset = offset.
 *
 * Segments are reported 8 per pair and round; the call reads each sub-batch's segment counts back to size its rounds, so
 * it waits for hip_stream.  The first report call on a plan adds pairs_in_flight * 8 fp64 rows of max_lags, counted by
 * ffs_drift_plan_workspace_bytes from then on; plans that never report keep the drift workspace alone. */
#define FFS_SEGMENT_OWN_NOT_PEAK 4 /* the segment's peak 1 is not at shift 0 */

typedef struct ffs_segment_report {
    int64_t first_block, end_block;     /* blocks [first_block, end_block) */
    int64_t start_sample, end_sample;   /* subtitle samples [start_sample, end_sample) */
    int64_t first_offset, last_offset;  /* o_b of the first and of the last block (samples) */
    int64_t min_offset, max_offset;     /* o_min, o_max over the blocks */
    double own_score;                   /* p_i(0) */
    double prev_score, next_score;      /* p_i at the shift continuing that neighbour; NaN without it / outside the set */
    double flat_score;                  /* the best constant lag of [o_min, o_max] */
    int64_t flat_offset;                /* the largest lag attaining it */
    double mean, std;                   /* of p_i over the n_lags shifts */
    int64_t n_lags;                     /* 2W - (o_max - o_min) */
    double peak_score[8];               /* peaks 0 .. n_peaks-1 (entries beyond: 0) */
    int64_t peak_shift[8];              /* samples; 0 = the path itself */
    int32_t n_peaks, flags;             /* flags: FFS_QUALITY_FLAT, FFS_SEGMENT_OWN_NOT_PEAK */
} ffs_segment_report;
#ifdef __cplusplus
static_assert(sizeof(ffs_segment_report) == 264, "ffs_segment_report is 264 bytes");
#else
_Static_assert(sizeof(ffs_segment_report) == 264, "ffs_segment_report is 264 bytes");
#endif

/* ffs_align_drift_batch plus the segment reports, in one call on hip_stream.  report_out_dev: n_pairs * max_b records
 * (8-byte aligned); n_segments_out_dev: n_pairs int32.  FFS_E_INVALID / FFS_E_EMPTY as ffs_align_drift_batch, and
 * FFS_E_INVALID for top_k outside [1, 8], exclusion_samples < 1 or a null / misaligned report output; all before any
 * launch, the outputs untouched. */
int ffs_align_drift_report_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int max_step, double step_cost, int top_k,
                                 int64_t exclusion_samples, int32_t* block_offset_out_dev, double* block_score_out_dev,
                                 uint8_t* block_jump_out_dev, double* total_out_dev, ffs_segment_report* report_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream);

/* ---- smooth drift fit: each segment's path as a polyline of knots (csrc/ffs_drift_smooth.h) ------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model
 * tests/drift_smooth_model.py, bit for bit.
 *
 * The drift solve of ffs_align_drift_batch (same arguments, same four outputs bit for bit), then inside every segment
 * [f, e) of it (as ffs_align_drift_report_batch forms them), with M = knot_blocks in [1, 256], R = radius in [0, 16],
 * lambda = bend_cost (finite, >= 0) and n = e - 1 - f:
 *   a one-block segment is returned as it is (its block is its one knot; fit_total = line_score = bend_total = 0.0);
 *   knots: I = max(1, (n + M/2) / M) intervals (integer division), knot blocks k_i = f + i M for i < I and k_I = e - 1;
 *     interval i has n_i = k_{i+1} - k_i blocks and holds the blocks k_i <= b < k_{i+1}, the last interval b = k_I too;
 *   candidates: knot i at lag c_i = o_{k_i} + u, u in [-R, R], only where -W + 1 <= c_i <= W;
 *   digital line: block b of interval i has lag d_b = c_i + floor((2 (c_{i+1} - c_i)(b - k_i) + n_i) / (2 n_i));
 *   line score T_i(c_i, c_{i+1}): ov, n1x, nx1, n11 of ffs_segment_report's path curve summed as exact integers over the
 *     interval's blocks at their lags d_b, then scored ONCE by that expression; exactly 0.0 where the overlap is 0;
 *   bend cost at an interior knot i between intervals of n_a and n_b blocks, D1 = c_i - c_{i-1}, D2 = c_{i+1} - c_i:
 *     g = |D2 n_a - D1 n_b| (int64), then ((lambda * (double)g) * (double)M) / (double)(n_a n_b), every fp64 operation
 *     rounded on its own -- lambda |D2 - D1| between equal intervals, nothing for a straight line of any slope;
 *   optimum: V_1 = T_0, V_{i+1}(c_i, c_{i+1}) = max over c_{i-1} of (V_i(c_{i-1}, c_i) - bend_i) + T_i(c_i, c_{i+1}),
 *     fit_total = max V_I.  Ties: candidates are tried in the order u = 0, +1, -1, +2, -2, ... and one replaces the best
 *     so far only when strictly greater -- over the predecessor at every step, over the final state with u_I as the
 *     outer and u_{I-1} as the inner loop.  Ties stay on the path.
 * Outputs: smooth_offset_out_dev[p * max_b + b] = d_b (int32; entries b >= B_p are 0); knot_out_dev[p * max_b + b]
 * (uint8) = 1 where b is a knot; segment_out_dev[p * max_b + i] for segment i (records past the segment count are zero):
 * fit_total, line_score (the chosen T_i summed in interval order from 0.0), bend_total (the chosen bend costs in knot
 * order from 0.0) and n_knots; n_segments_out_dev[p].  Nothing is read back: the call is asynchronous.
 * The first smooth call on a plan adds some pairs_in_flight * max_blocks * 9837 bytes (33 * 33 fp64 line scores and
 * back-pointer bytes per interval, the segment and interval tables; 6.9 MB per pair at 2 h, K = 1024), counted by ffs_drift_plan_workspace_bytes from then on; plans that never call it keep
 * their size, and drift results after it stay bit-identical.
 * FFS_E_INVALID / FFS_E_EMPTY as ffs_align_drift_batch, and FFS_E_INVALID for knot_blocks, radius or bend_cost outside
 * the ranges above or a null / misaligned output (smooth offsets and counts 4-byte, records 8-byte aligned); all before
 * any launch, the outputs untouched. */
#define FFS_SMOOTH_MAX_KNOT_BLOCKS 256
#define FFS_SMOOTH_MAX_RADIUS 16

typedef struct ffs_smooth_segment {
    double fit_total;          /* the Viterbi maximum: line scores minus bend costs */
    double line_score;         /* sum of the chosen lines' scores */
    double bend_total;         /* sum of the chosen knots' bend costs */
    int32_t n_knots, reserved; /* I + 1 (1 for a one-block segment); 0 */
} ffs_smooth_segment;
#ifdef __cplusplus
static_assert(sizeof(ffs_smooth_segment) == 32, "ffs_smooth_segment is 32 bytes");
#else
_Static_assert(sizeof(ffs_smooth_segment) == 32, "ffs_smooth_segment is 32 bytes");
#endif

int ffs_align_drift_smooth_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int max_step, double step_cost,
                                 int knot_blocks, int radius, double bend_cost, int32_t* block_offset_out_dev,
                                 double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                                 int32_t* smooth_offset_out_dev, uint8_t* knot_out_dev, ffs_smooth_segment* segment_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream);

/* ---- smooth drift fit over any lag range (csrc/ffs_drift_range_smooth.h) --------------------------------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model
 * tests/drift_range_smooth_model.py, bit for bit.
 *
 * ffs_align_drift_range_batch (same arguments, same four outputs bit for bit) followed, in the same sub-batch, by
 * ffs_align_drift_smooth_batch's fit of every segment, with ONE change: a knot candidate c_i = o_{k_i} + u is valid
 * where lag_lo_p <= c_i <= lag_hi_p (the pair's range) instead of -W + 1 <= c_i <= W.  Segments, knot blocks, digital
 * lines, the uint32 sums of ov / n11 / n1x / nx1 scored once, 0.0 for an empty overlap, -inf for an invalid end, the
 * bend cost, the Viterbi pass, its tie rule and fit_total are as stated there; the block terms are the range path's
 * (absent samples; a block whose lag leaves it no overlap contributes nothing).  At [-W+1, W] all eight outputs equal
 * ffs_align_drift_smooth_batch's bit for bit.  knot_blocks in [1, FFS_SMOOTH_MAX_KNOT_BLOCKS], radius in
 * [0, FFS_SMOOTH_MAX_RADIUS], bend_cost finite and >= 0, max_step <= the plan's max_step_cap.  Outputs as
 * ffs_align_drift_smooth_batch (smooth offsets are lags in samples, 0 past B_p; records past the segment count are
 * zero).  Nothing is read back: the call is asynchronous.
 *
 * The range solve stores no (block, lag) counts; the fit counts n11 again in a band around the path: per block
 * max_step * ceil(3 knot_blocks / 2) + 2 radius + 1 uint16 cells (81 at max_step 2, knot_blocks 16, radius 16).  The
 * first smooth call on a plan adds pairs_in_flight * max_blocks' (max_blocks rounded up to 16) *
 * (9837 + 2 * (max_step_cap * 384 + 33)) bytes -- ffs_align_drift_smooth_batch's tables and band rows for the plan's
 * max_step_cap at knot_blocks 256, radius 16, so later calls need nothing more -- plus fewer than 128 bytes of padding:
 * 8.1 MB per pair at 2 h, K = 1024 and max_step_cap 2 (704 blocks; 10.8 MB at max_step_cap 7) against 403 MB of codes
 * and rows.  ffs_drift_range_plan_workspace_bytes counts it from then on; plans that never call it keep their size, and
 * drift results after it stay bit-identical.
 * FFS_E_INVALID / FFS_E_EMPTY as ffs_align_drift_range_batch, and FFS_E_INVALID for knot_blocks, radius or bend_cost
 * outside the ranges above or a null / misaligned output (smooth offsets and counts 4-byte, records 8-byte aligned); all
 * before any launch, the outputs untouched. */
int ffs_align_drift_range_smooth_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                       const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                       const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                       const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                       const int64_t* lag_hi, double split_penalty, int max_step, double step_cost,
                                       int knot_blocks, int radius, double bend_cost, int32_t* block_offset_out_dev,
                                       double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                                       int32_t* smooth_offset_out_dev, uint8_t* knot_out_dev,
                                       ffs_smooth_segment* segment_out_dev, int32_t* n_segments_out_dev, void* hip_stream);

/* ---- per-segment path report of a drift solve over any lag range (csrc/ffs_drift_range_report.h) --------------------
 * Replaces: nothing in the reference.  The contract below is pinned against the numpy model
 * tests/drift_range_report_model.py and the independent reference tests/report_reference.py.
 *
 * ffs_align_drift_report_batch's segment records (ffs_segment_report, unchanged, the same flags) for a finished path
 * -- block_offset_dev[p * max_b + b] and block_jump_dev[p * max_b + b] as ffs_align_drift_range_batch writes them,
 * every o_b inside [lag_lo_p, lag_hi_p] -- over the lag set d in [lag_lo_p, lag_hi_p], L = lag_hi - lag_lo + 1, instead
 * of [-W+1, W].  Segments are formed from block_jump as there.  Shift set delta in [lag_lo - o_min, lag_hi - o_max]:
 * n_lags = L - (o_max - o_min) >= 1, shift index t puts block b at the lag lag_lo + t + (o_b - o_min).  Per block and
 * lag d: a = max(bK, -d), e = min((b+1)K, S, R-d); where e > a, ov / n1x / nx1 as there and n11 counted exactly from the
 * bits; where e <= a all four are 0.  The four are summed over the segment's blocks as exact integers and scored once
 * (split_mix, no FMA); the score is exactly 0.0 where the summed overlap is 0, and such shifts count in the moments.
 * Moments and greedy peaks over the n_lags shifts as there (peaks reported as shifts, 0 the path itself); own = p(0),
 * prev = p(last_offset_{i-1} - first_offset_i), next = p(first_offset_{i+1} - last_offset_i), NaN without that neighbour
 * or outside the shift set; flat_score / flat_offset the maximum over d in [o_min, o_max] of the constant-lag score of
 * the segment's samples on their exact n11, the largest d on ties.  At [-W+1, W], given ffs_align_drift_batch's path,
 * the records are bit-identical to ffs_align_drift_report_batch's; at max_step = 0 they equal
 * ffs_split_range_report_batch's in the shared fields.  report_out_dev: n_pairs * max_b records (8-byte aligned;
 * records past the count zero); n_segments_out_dev: n_pairs int32.
 *
 * The range solve stores no counts, so the report neither needs nor touches the DP: it is a post-pass.  The call reads
 * the offsets and jump flags back once (it waits for hip_stream's earlier work) to check them and to schedule its
 * rounds; the kernels run on hip_stream.  Segments are reported 8 per pair and round.  The first report call on a plan
 * adds pairs_in_flight * 8 rows of max_lags + 1 cells (padded to 64) of 12 bytes -- a uint32 n11 row, whose last
 * o_max - o_min + 1 cells hold the constant-lag counts, and an fp64 score row -- plus a work-item table of
 * pairs_in_flight * 2 * (ceil(ceil(max_samples / 32) / 512) + max_blocks) * 32 bytes: 138 MB per pair at 2 h over the
 * full range (1 439 999 lags).  ffs_drift_range_plan_workspace_bytes counts it from then on; a plan that never reports
 * keeps its size, and drift results after a report stay bit-identical.
 * FFS_E_INVALID / FFS_E_EMPTY for everything ffs_align_drift_range_batch refuses of these arguments, and FFS_E_INVALID
 * for top_k outside [1, 8], exclusion_samples < 1, a null or misaligned offset, jump or output pointer, or a block
 * offset outside its pair's range; all before any launch, the outputs untouched. */
int ffs_drift_range_report_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                 const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                 const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                 const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                 const int64_t* lag_hi, const int32_t* block_offset_dev, const uint8_t* block_jump_dev,
                                 int top_k, int64_t exclusion_samples, ffs_segment_report* report_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream);

/* ---- ratio sweep: peaks and moments of ratio profiles (csrc/ffs_sweep.h) ---------------------------------------
 * Replaces: nothing in the reference.  A ratio sweep (ffsubsync_amd/ratio_sweep.py) solves every file at a grid of speed
 * factors with the batch solve above and keeps the ffs_cand_result records in HBM; this call reduces each file's
 * profile to one record.  Stateless: no plan, everything is queued on hip_stream.  Pinned against tests/sweep_model.py.
 *
 * File f owns the points rec_dev[first_dev[f] .. first_dev[f+1]) (first_dev: n_files + 1 ascending int64 on the device;
 * point index j = position in that range).  A point is SKIPPED when its score is not finite or its flags carry
 * FFS_FLAG_EMPTY_WINDOW.  Peak 1 = the largest score among the points not skipped, the smaller index on ties; peak k+1 =
 * the same over the indices j with |j - j_i| >= exclusion_steps for every earlier peak i; fewer than top_k (1..8) peaks
 * when no point is eligible.  Moments: mean and population std (ddof = 0) over the points not skipped, two passes, in a
 * fixed summation order; when all of them are equal, mean = that score and std = 0 exactly (FFS_SWEEP_FLAT).  No point
 * left: mean = std = 0, no peak, FFS_SWEEP_FLAT | FFS_SWEEP_EMPTY.  FFS_SWEEP_AMBIGUOUS: some point of the file (skipped
 * or not) carried FFS_FLAG_AMBIGUOUS.  Records are read, never written; exactly n_files output records are written.
 * FFS_E_INVALID for top_k outside [1, 8], exclusion_steps < 1, n_files < 0, or a null or misaligned (8 bytes)
 * pointer: refused before any launch, the outputs untouched. */
#define FFS_SWEEP_FLAT 1      /* every point not skipped scores the same (or none is left): std = 0 */
#define FFS_SWEEP_EMPTY 2     /* no point left after skipping */
#define FFS_SWEEP_AMBIGUOUS 4 /* some point carried FFS_FLAG_AMBIGUOUS */

typedef struct ffs_sweep_profile {
    double peak_score[8];       /* peaks 0 .. n_peaks-1 (entries beyond: 0) */
    int64_t peak_offset[8];     /* the peak record's offset (samples) */
    int64_t peak_index[8];      /* the peak's point index inside the file */
    double mean, std;           /* of the scores of the points not skipped */
    int64_t n_points, n_skipped;
    int32_t n_peaks, flags;     /* flags: FFS_SWEEP_* */
} ffs_sweep_profile;
#ifdef __cplusplus
static_assert(sizeof(ffs_sweep_profile) == 232, "ffs_sweep_profile is 232 bytes");
#else
_Static_assert(sizeof(ffs_sweep_profile) == 232, "ffs_sweep_profile is 232 bytes");
#endif

int ffs_sweep_peaks(const ffs_cand_result* rec_dev, const int64_t* first_dev, int n_files, int top_k,
                    int64_t exclusion_steps, ffs_sweep_profile* out_dev, void* hip_stream);

/* ---- shuffled-cue significance: surrogate lists and the empirical null of their scores (csrc/ffs_surrogate.h) ---
 * Replaces: nothing in the reference.  "Is this subtitle related to this audio at all?" answered without a tuned
 * threshold (ffsubsync_amd/surrogate.py): the window-maximum score of the real subtitle is compared with the scores of K
 * surrogate subtitles that keep every cue, every silence, the length, the number of speech samples and the reference,
 * and differ only in which cue sits where.  Both calls are stateless: no plan, everything is queued on hip_stream,
 * nothing is waited for or read back.  Pinned against tests/surrogate_model.py.
 *
 * ffs_surrogate_lists.  Vector v: a valid ffs_runs_list at list_dev[v] (device, 8-byte aligned) with n boundaries,
 * m = n / 2 runs; n_bound[v] = a host-known upper bound of n (the convention of vec_max_boundaries); seed[v].  Unit j,
 * j < m - 1, is run j together with the silence behind it: pos[2j+2] - pos[2j] samples of which pos[2j+1] - pos[2j]
 * are ones.  The silence in front of run 0, the last run and the tail behind it stay where they are.  The U = m - 1
 * units are cut into nb = ceil(U / block_units) blocks of block_units consecutive units (the last may be short).
 * Surrogate s (0 <= s < n_surrogates) places the blocks in ascending order of (key(seed, s, b), b),
 *   key = fmix32(fmix32(seed + 0x9E3779B9 * (s + 1)) ^ b),
 *   fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16   (all uint32),
 * units keeping their order inside a block (fmix32 is a bijection of uint32, so two blocks of one surrogate never share
 * a key: the index completes the order's statement and never decides it).  Its list -- the same n, ones and len, cap = out_cap[v], pos strictly
 * ascending, ones_before exact, e[n] = (INT32_MAX, ones) -- is written to out_dev + out_off[v] + s *
 * ffs_runs_list_bytes(out_cap[v]): the K blocks of a vector lie back to back.  With m <= 2 it equals the input.  Only
 * the header and the n + 1 entries are written.  status_dev[v] (int32, always written) = 0, or FFS_SURR_BAD_* bits for
 * a list whose header is odd, truncated (n >= cap, or negative), above its bound or above the unit limit: all K
 * surrogates of such a list are empty lists (n = 0, ones = 0, the same len, the sentinel only); other vectors of the
 * call are not affected.  Host arrays may be freed after return.
 * FFS_E_INVALID, before any launch, outputs and status untouched: n_surrogates outside [1, FFS_SURR_MAX_K], block_units
 * outside [1, FFS_SURR_MAX_UNITS], a negative n_vec, out_bytes or n_bound, a null or misaligned pointer (lists and
 * output 8 bytes, status 4), out_off not a multiple of 8, out_cap < n_bound + 1 or out_cap >= 2^28, K blocks that do
 * not fit [out_off, out_bytes), or n_vec * n_surrogates >= 2^31 (one workgroup per surrogate: more than a grid holds).
 *
 * ffs_null_stats.  File f owns the n_surrogates + 1 records rec_dev[f * (n_surrogates + 1) ..]: record 0 the real
 * list's solve, the others the surrogates'.  A record is USABLE when its score is finite and its flags do not carry
 * FFS_FLAG_EMPTY_WINDOW.  real_score = record 0's score; n_null = usable null records; null_mean / null_std
 * (population, two passes in a fixed order; std exactly 0 and mean = that score when min == max) and null_min /
 * null_max over them (all 0 with none); n_ge / n_gt = usable nulls with score >= / > real_score (0 when record 0 is not
 * usable).  flags: FFS_NULL_FLAT (no usable null, or all equal), FFS_NULL_EMPTY (no usable null, or record 0 not
 * usable), FFS_NULL_AMBIGUOUS (some record of the file carried FFS_FLAG_AMBIGUOUS).  The host derives
 * z = (real_score - null_mean) / null_std (0 when FLAT) and p = (1 + n_ge) / (1 + n_null).  Records are read, never
 * written; exactly n_files output records are written.  FFS_E_INVALID for n_surrogates outside [1, FFS_SURR_MAX_K],
 * n_files < 0, or a null or misaligned (8 bytes) pointer: refused before any launch, the outputs untouched. */
#define FFS_SURR_MAX_UNITS 8192 /* units of a list: lists of up to 16 386 boundaries */
#define FFS_SURR_MAX_K 4096     /* surrogates per vector */
#define FFS_SURR_BAD_ODD 1       /* status: n is odd */
#define FFS_SURR_BAD_TRUNCATED 2 /* status: n >= cap (or negative) */
#define FFS_SURR_BAD_BOUND 4     /* status: n > n_bound */
#define FFS_SURR_BAD_UNITS 8     /* status: more than FFS_SURR_MAX_UNITS units */
#define FFS_NULL_FLAT 1      /* every usable null scores the same (or none is left): std = 0 */
#define FFS_NULL_EMPTY 2     /* no usable null record, or the real record is not usable */
#define FFS_NULL_AMBIGUOUS 4 /* some record carried FFS_FLAG_AMBIGUOUS */

typedef struct ffs_null_result {
    double real_score;           /* record 0's score */
    double null_mean, null_std;  /* of the usable null scores */
    double null_min, null_max;
    int32_t n_null, n_ge, n_gt;
    int32_t flags;               /* FFS_NULL_* */
} ffs_null_result;
#ifdef __cplusplus
static_assert(sizeof(ffs_null_result) == 56, "ffs_null_result is 56 bytes");
#else
_Static_assert(sizeof(ffs_null_result) == 56, "ffs_null_result is 56 bytes");
#endif

int ffs_surrogate_lists(const void* const* list_dev, const int32_t* n_bound, const uint32_t* seed, const int64_t* out_off,
                        const int64_t* out_cap, int64_t n_vec, int n_surrogates, int block_units, void* out_dev,
                        int64_t out_bytes, int32_t* status_dev, void* hip_stream);
int ffs_null_stats(const ffs_cand_result* rec_dev, int n_files, int n_surrogates, ffs_null_result* out_dev,
                   void* hip_stream);

/* ---- half-sample stability: thinned lists and the order statistics of their solved offsets (csrc/ffs_stability.h) ---
 * Replaces: nothing in the reference.  "How precisely is this offset known, and would the peak that won still win on
 * another half of the cues?" answered without a tuned score threshold (ffsubsync_amd/stability.py): K subtitles that
 * each keep a hashed half of the cue blocks, positions untouched, are solved beside the real one; a real sync peaks at
 * the same lag on every half, a chance maximum all over the window.  Both calls are stateless: no plan, everything is
 * queued on hip_stream, nothing is waited for or read back.  Pinned against tests/stability_model.py.
 *
 * ffs_subsample_lists.  The argument shapes and conventions of ffs_surrogate_lists.  Vector v: a valid ffs_runs_list
 * at list_dev[v] (device, 8-byte aligned) with n boundaries, m = n / 2 runs; n_bound[v] = a host-known upper bound of
 * n; seed[v].  The m runs -- all of them, the first and the last included -- are cut into nb = ceil(m / block_runs)
 * blocks of block_runs consecutive runs (the last may be short).  Subsample s (0 <= s < n_subsamples) keeps block b iff
 *   ((key(seed, s >> 1, b) >> 31) ^ (s & 1)) == 1,   key = the hash of ffs_surrogate_lists with p = s >> 1 for its s,
 * so subsamples 2j and 2j + 1 are complementary: every run of the input is in exactly one of them (with an odd
 * n_subsamples the last has no partner).  Its list -- the kept runs in input order: n' = 2 kept, pos copied unchanged,
 * ones_before the prefix sum of the kept runs' lengths, ones' their total, the same len, cap = out_cap[v],
 * e[n'] = (INT32_MAX, ones') -- is written to out_dev + out_off[v] + s * ffs_runs_list_bytes(out_cap[v]): the K blocks
 * of a vector lie back to back.  A subsample may keep nothing (n' = 0, the sentinel only) or everything.  Only the
 * header and the n' + 1 entries are written.  status_dev[v] (int32, always written) = 0, or FFS_SUB_BAD_* bits for a
 * list whose header is odd, truncated (n >= cap, or negative) or above its bound: all K subsamples of such a list are
 * empty lists of the same len; other vectors of the call are not affected.  There is no unit limit.  Host arrays may
 * be freed after return.
 * FFS_E_INVALID, before any launch, outputs and status untouched: n_subsamples outside [1, FFS_STAB_MAX_K], block_runs
 * outside [1, FFS_STAB_MAX_BLOCK_RUNS], a negative n_vec, out_bytes or n_bound, a null or misaligned pointer (lists and
 * output 8 bytes, status 4), out_off not a multiple of 8, out_cap < n_bound + 1 or out_cap >= 2^28, K blocks that do
 * not fit [out_off, out_bytes), or n_vec * n_subsamples >= 2^31.  n_vec == 0 returns 0.
 *
 * ffs_offset_stats.  File f owns the n_subsamples + 1 records rec_dev[f * (n_subsamples + 1) ..]: record 0 the real
 * list's solve, record 1 + s subsample s.  A record is USABLE by the rule of ffs_null_stats.  With the c usable
 * subsample offsets sorted ascending: off_min, off_max, off_median = sorted[(c - 1) / 2], off_lo = sorted[(c - 1) / 20],
 * off_hi = sorted[c - 1 - (c - 1) / 20] (integer division: the central 90 %); max_dev = max |off - real_offset| and
 * n_within = those with |off - real_offset| <= tol.  Over the pairs (2j, 2j + 1) with both members usable: n_pairs,
 * max_pair_gap = max |off(2j) - off(2j + 1)|, n_pairs_within = pairs whose gap <= tol, pair_score_min = min of
 * score(2j) + score(2j + 1) (one addition of two doubles; -0.0 orders below +0.0); all 0 without such a pair.
 * flags: FFS_STAB_EMPTY (record 0 not usable, or c = 0: the five order statistics, max_dev and n_within are then 0),
 * FFS_STAB_AMBIGUOUS (some record of the file carried FFS_FLAG_AMBIGUOUS), FFS_STAB_NO_PAIRS (n_pairs = 0).  Offsets
 * are 64-bit all the way.  Records are read, never written; exactly n_files output records are written, every byte of
 * them.  FFS_E_INVALID for n_subsamples outside [1, FFS_STAB_MAX_K], n_files < 0, tol < 0, or a null or misaligned
 * (8 bytes) pointer: refused before any launch, the outputs untouched. */
#define FFS_STAB_MAX_K 4096              /* subsamples per vector */
#define FFS_STAB_MAX_BLOCK_RUNS 16777216 /* 2^24 */
#define FFS_SUB_BAD_ODD 1       /* status: n is odd (= FFS_SURR_BAD_ODD) */
#define FFS_SUB_BAD_TRUNCATED 2 /* status: n >= cap (or negative) */
#define FFS_SUB_BAD_BOUND 4     /* status: n > n_bound */
#define FFS_STAB_EMPTY 1     /* the real record is not usable, or no subsample record is */
#define FFS_STAB_AMBIGUOUS 2 /* some record carried FFS_FLAG_AMBIGUOUS */
#define FFS_STAB_NO_PAIRS 4  /* no pair (2j, 2j + 1) with both members usable */

typedef struct ffs_stability_result {
    double real_score;            /* record 0's score */
    int64_t real_offset;          /* record 0's offset */
    int64_t off_min, off_max, off_median, off_lo, off_hi; /* of the usable subsample offsets */
    int64_t max_dev, max_pair_gap;
    double pair_score_min;
    int32_t n_sub, n_within, n_pairs, n_pairs_within;
    int64_t tol;
    int32_t flags;                /* FFS_STAB_* */
    int32_t reserved;             /* 0 */
} ffs_stability_result;
#ifdef __cplusplus
static_assert(sizeof(ffs_stability_result) == 112, "ffs_stability_result is 112 bytes");
#else
_Static_assert(sizeof(ffs_stability_result) == 112, "ffs_stability_result is 112 bytes");
#endif

int ffs_subsample_lists(const void* const* list_dev, const int32_t* n_bound, const uint32_t* seed, const int64_t* out_off,
                        const int64_t* out_cap, int64_t n_vec, int n_subsamples, int block_runs, void* out_dev,
                        int64_t out_bytes, int32_t* status_dev, void* hip_stream);
int ffs_offset_stats(const ffs_cand_result* rec_dev, int n_files, int n_subsamples, int64_t tol,
                     ffs_stability_result* out_dev, void* hip_stream);

/* ---- adaptive energy VAD: a per-file threshold from frame-level counts (csrc/ffs_adaptive_vad.h) -----------------
 * Replaces: nothing in the reference.  This is the project's own rule with no upstream counterpart (the reference's
 * adaptive detector is WebRTC's, a third-party wheel): parity is against the in-repo numpy model
 * tests/adaptive_vad_model.py only, bit for bit.  ffs_vad_energy and its fixed threshold are unchanged.
 *
 * Edges.  edges[0 .. n_edges) are doubles, ascending, positive and finite, 1 <= n_edges <= FFS_VAD_MAX_EDGES, supplied
 * by the caller in device memory (adaptive_vad.default_edges(): 10^(k / 20), k = 1 .. 191, i.e. half-dB steps; edges[99]
 * is 10^5 = 50 dB).  B = n_edges + 1 level bins.
 * Level of frame f.  E_f the exact 64-bit sum of squares and n_f the sample count of the frame (the last one may be
 * short), as in ffs_vad_energy:  level[f] = #{k : (double)E_f >= edges[k] * (double)n_f}  -- one fp64 multiply and one
 * compare per edge, the evaluation ffs_vad_energy uses for its one threshold.  A count of satisfied edges: defined for
 * any table; for an ascending one  level >= t  <=>  the fixed rule with threshold edges[t - 1].  uint8, in [0, n_edges].
 * Histogram.  hist[b] = number of frames with level b, uint32[n_bins]; a level byte >= n_bins is counted nowhere.
 * Pick.  0 <= lo_bin < t_min <= t_max <= B - 1, 0 <= fallback_bin <= B, 0 <= floor_ppm <= 10^6, 0 <= margin_bins <= 255.
 *   h'[b] = hist[b] for b >= lo_bin, else 0 (frames below lo_bin are silence and never counted, so stretches of
 *   digital silence cannot become one of the two classes);  N' = sum h', S = sum b h', Q = sum b^2 h'.  In order:
 *   1. sum hist > FFS_VAD_MAX_FRAMES (2^23): TOO_LONG | FALLBACK.
 *   2. N' == 0: EMPTY | FALLBACK.
 *   3. FFS_VAD_RULE_OTSU: for t in lo_bin + 1 .. B - 1 with n0 = sum_{b<t} h', s0 = sum_{b<t} b h' and 0 < n0 < N':
 *      d = S n0 - N' s0 and m = n0 (N' - n0) in exact int64, v(t) = ((double)d * (double)d) / (double)m (conversions
 *      round to nearest; one multiply, one correctly rounded divide, no add).  The smallest t of the largest v wins;
 *      eta = v_max / (double)(N' Q - S S), the share of the counted levels' variance the split explains, in [0, 1].
 *      No such t (all counted frames in one bin): FLAT | FALLBACK, eta = 0.
 *   4. FFS_VAD_RULE_FLOOR: need = max(1, (N' floor_ppm + 999999) / 1000000) in integers, floor_bin the smallest b with
 *      sum_{lo_bin <= b' <= b} h' >= need, t = floor_bin + margin_bins; FLAT is flagged when it holds, the result
 *      stands; eta = 0.
 *   5. A rule's result outside [t_min, t_max] is clamped and flagged CLAMPED_LO / CLAMPED_HI.
 *   6. A fallback sets threshold_bin = fallback_bin, unclamped (100 with the default table: the fixed 50 dB rule).
 *   floor_bin is reported under either rule with the given floor_ppm (-1 when N' == 0), top_bin is the highest occupied
 *   counted bin (-1 when N' == 0), n_speech = sum_{b >= threshold_bin} hist[b].
 * Labels.  Frame f is speech iff level[f] >= threshold_bin.
 *
 * ffs_vad_levels streams the PCM once and writes ceil(n_samples / frame_len) level bytes, nothing behind them; it can
 * be called chunk by chunk (a caller sweeping 100 s buffers points each call at levels_dev + first_frame; any byte
 * address).  ffs_vad_level_hist zeroes hist_dev on the stream and counts (n_frames == 0 leaves the zeros: the
 * histogram of no frames); a few thousand integer atomics per call whatever the length, so the result does not depend
 * on arrival order.  ffs_vad_pick_threshold reduces n_hist >= 0 histograms, n_bins apart, to one 48-byte record each.
 * ffs_vad_level_labels reads the threshold ON THE DEVICE from threshold_dev when that is not NULL -- a record's
 * address works, threshold_bin is its first field, and nothing waits for a read-back -- else it is threshold_host in
 * [0, 256].  Its outputs are ffs_vad_energy's two forms, either may be NULL: labels_dev[f] = 1.0f / non_speech_label,
 * and bits_dev as ffs_vad_energy_bits writes it (ceil(n_frames / 8) bytes, the unused high bits of the last byte 0,
 * nothing beyond them).
 * FFS_E_INVALID with a message, before any launch: negative counts, frame_len < 1, n_edges outside [1, 255], n_bins
 * outside [2, 256], an unknown rule, a parameter outside the ranges above, a null or misaligned pointer.  A count of 0
 * is FFS_OK with nothing written (but for ffs_vad_level_hist's zeros).  The calls are stateless. */
#define FFS_VAD_MAX_EDGES 255
#define FFS_VAD_MAX_BINS 256
#define FFS_VAD_MAX_FRAMES 8388608 /* 2^23: frames of one histogram the Otsu arithmetic is exact for */
#define FFS_VAD_RULE_OTSU 0
#define FFS_VAD_RULE_FLOOR 1
#define FFS_VAD_THR_FALLBACK 1    /* threshold_bin is fallback_bin */
#define FFS_VAD_THR_TOO_LONG 2    /* more than FFS_VAD_MAX_FRAMES frames */
#define FFS_VAD_THR_EMPTY 4       /* no frame at or above lo_bin */
#define FFS_VAD_THR_FLAT 8        /* all counted frames share one bin */
#define FFS_VAD_THR_CLAMPED_LO 16 /* the rule's result was below t_min */
#define FFS_VAD_THR_CLAMPED_HI 32 /* the rule's result was above t_max */

typedef struct ffs_vad_threshold {
    int32_t threshold_bin;        /* speech <=> level >= threshold_bin (first field: ffs_vad_level_labels reads it in place) */
    int32_t flags;                /* FFS_VAD_THR_* */
    int32_t floor_bin;            /* the floor_ppm quantile of the counted bins, or -1 */
    int32_t top_bin;              /* the highest occupied counted bin, or -1 */
    int64_t n_frames;             /* sum hist */
    int64_t n_counted;            /* N' */
    int64_t n_speech;             /* frames at or above threshold_bin */
    double eta;                   /* Otsu's separability, 0 otherwise */
} ffs_vad_threshold;
#ifdef __cplusplus
static_assert(sizeof(ffs_vad_threshold) == 48, "ffs_vad_threshold is 48 bytes");
#else
_Static_assert(sizeof(ffs_vad_threshold) == 48, "ffs_vad_threshold is 48 bytes");
#endif

int ffs_vad_levels(const int16_t* pcm_dev, int64_t n_samples, int frame_len, const double* edges_dev, int n_edges,
                   uint8_t* levels_dev, void* hip_stream);
int ffs_vad_level_hist(const uint8_t* levels_dev, int64_t n_frames, int n_bins, uint32_t* hist_dev, void* hip_stream);
int ffs_vad_pick_threshold(const uint32_t* hist_dev, int n_hist, int n_bins, int rule, int lo_bin, int t_min, int t_max,
                           int fallback_bin, int floor_ppm, int margin_bins, ffs_vad_threshold* records_dev,
                           void* hip_stream);
int ffs_vad_level_labels(const uint8_t* levels_dev, int64_t n_frames, const int32_t* threshold_dev, int threshold_host,
                         float non_speech_label, float* labels_dev, uint8_t* bits_dev, void* hip_stream);

/* ---- steady-run gate behind the adaptive VAD: drop music, hum and hiss by length (csrc/ffs_vad_gate.h) -----------
 * Replaces: nothing in the reference.  An energy rule labels every loud frame as speech, a music bed, a tone or an
 * audience included.  A person does not talk for ten seconds without one 10 ms frame falling below the file's threshold,
 * and the reference clamps every cue to DEFAULT_MAX_SUBTITLE_SECONDS = 10 (constants.py:14, subtitle_parser.py:163), so a
 * stretch of uninterrupted activity longer than that carries no alignment evidence and is dropped whole, edges
 * included.  Integers only: pinned bit for bit against tests/steady_gate_model.py.  ffs_vad_level_labels is unchanged.
 *
 * Inputs.  level[0 .. n) as ffs_vad_levels writes them; t the threshold bin, read ON THE DEVICE from threshold_dev when
 * that is not NULL (a record's address works, as for ffs_vad_level_labels; the value is taken as it stands), else
 * threshold_host in [0, 256]; dip_bins in [0, 255]; max_run in [1, 2^31 - 1] frames.
 * Classes.  Frame i is ACTIVE iff level[i] >= t, QUIET iff (int)level[i] < t - dip_bins (never when t - dip_bins <= 0),
 * else a KEEP frame.
 * State.  s[-1] = quiet; s[i] = the class of the last active or quiet frame at or before i.
 * Stretches.  A stretch opens at a rise (i active, s[i-1] quiet) and closes at the next fall (i quiet, s[i-1] active)
 * or at the end of the file.  Its extent is [b, e], b the rise, e the last active frame before the fall (trailing keep
 * frames do not count); its length is e - b + 1.
 * Decision.  speech(f) = active(f) and length(stretch(f)) <= max_run.
 * It follows: max_run >= n gives ffs_vad_level_labels' outputs byte for byte; dip_bins = 0 removes exactly the runs of
 * ones longer than max_run from them; for fixed t and max_run the kept set shrinks as dip_bins grows.
 *
 * Record (one per call, 48 bytes): the t that was used, the flags, the stretches, those longer than max_run, the longest
 * length (0: none), the frames, the active frames and the active frames kept.  Flags, in order of evaluation:
 *   FFS_VAD_GATE_TOO_LONG      n_frames > FFS_VAD_MAX_FRAMES: the gate is skipped, the outputs are exactly
 *                              ffs_vad_level_labels', and of the counts only n_frames is set (the pick's own fallback
 *                              at this length);
 *   FFS_VAD_GATE_NO_QUIET      t - dip_bins <= 0: no frame can close a stretch (set beside TOO_LONG too);
 *   FFS_VAD_GATE_ALL_REJECTED  n_active > 0 and n_kept == 0.
 *
 * ffs_vad_steady_gate queues three ordered launches on the stream -- per-tile summaries of 4096 frames, one workgroup
 * that carries the state over the summaries forward and backward and writes the record, the labels per tile -- and
 * returns; no workgroup waits for another, nothing is allocated and nothing synchronises.  The carries live in the
 * caller's workspace_dev: ffs_vad_steady_gate_workspace_bytes(n_frames) bytes (56 per tile; 0 for no frames and for
 * more than FFS_VAD_MAX_FRAMES, when workspace_dev may be NULL), 8-byte aligned, free again when the stream has passed
 * the call.  Outputs in ffs_vad_level_labels' two forms, either or both may be NULL: labels_dev[f] = 1.0f /
 * non_speech_label, bits_dev ceil(n_frames / 8) bytes with the unused high bits of the last byte 0; nothing is written
 * behind them.  levels_dev may be any byte address (16-byte loads where it is 16-byte aligned).  n_frames == 0 is FFS_OK
 * and writes the record alone, all counts 0.
 * FFS_E_INVALID with a message, before any launch: a negative count, threshold_host (without threshold_dev), dip_bins or
 * max_run outside the ranges above, a null levels_dev (n_frames > 0) or record_dev, a misaligned threshold_dev or
 * labels_dev (4 bytes), record_dev or workspace_dev (8 bytes), a workspace that is too small.  Stateless. */
#define FFS_VAD_GATE_NO_QUIET 1     /* t - dip_bins <= 0 */
#define FFS_VAD_GATE_ALL_REJECTED 2 /* active frames, none kept */
#define FFS_VAD_GATE_TOO_LONG 4     /* more than FFS_VAD_MAX_FRAMES frames: plain labels */

typedef struct ffs_vad_gate {
    int32_t threshold_bin;        /* the t that was used */
    int32_t flags;                /* FFS_VAD_GATE_* */
    int32_t n_stretches;
    int32_t n_rejected;           /* stretches longer than max_run */
    int32_t longest_run;          /* the longest stretch's length, 0: none */
    int32_t reserved;             /* 0 */
    int64_t n_frames;
    int64_t n_active;             /* frames at or above t */
    int64_t n_kept;               /* of them, labelled speech */
} ffs_vad_gate;
#ifdef __cplusplus
static_assert(sizeof(ffs_vad_gate) == 48, "ffs_vad_gate is 48 bytes");
#else
_Static_assert(sizeof(ffs_vad_gate) == 48, "ffs_vad_gate is 48 bytes");
#endif

int64_t ffs_vad_steady_gate_workspace_bytes(int64_t n_frames);
int ffs_vad_steady_gate(const uint8_t* levels_dev, int64_t n_frames, const int32_t* threshold_dev, int threshold_host,
                        int dip_bins, int64_t max_run, float non_speech_label, float* labels_dev, uint8_t* bits_dev,
                        ffs_vad_gate* record_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* ---- centre-channel VAD: speech from stereo PCM by mid / side contrast (csrc/ffs_stereo_vad.h) -----------------------
 * Replaces: nothing in the reference (it asks ffmpeg for -ac 1, speech_transformers.py:551, and so discards the cue).
 * Dialogue is mixed to the centre, L ~ R; music, ambience, audiences and effects are mixed wide.  The mid signal L + R
 * holds the centre, the side signal L - R only what differs between the channels, so a frame whose mid level does not
 * stand min_contrast_bins above its side level is not dialogue, however loud, and speech over a wide bed still is.
 * The project's own rule: a numpy / integer model (tests/stereo_vad_model.py) is its only reference, and its shipped
 * default comes from SYNTHETIC data (profiles/centre_gate_calibration.json).
 *
 * ffs_vad_stereo_levels.  pcm_dev holds n_pairs interleaved (L, R) int16 pairs at any 2-byte aligned address; frame_len
 * >= 1 counts PAIRS per frame; n_frames = ceil(n_pairs / frame_len), the last frame may be short (n_f pairs).  In exact
 * 64-bit integers
 *   M_f = sum (L_i + R_i)^2,   S_f = sum (L_i - R_i)^2
 *   mid[f]  = #{k : (double)M_f >= edges[k] * (double)(4 n_f)}
 *   side[f] = #{k : (double)S_f >= edges[k] * (double)(4 n_f)}
 * edges and n_edges as for ffs_vad_levels.  The factor 4 (exact on both sides of the compare) makes a dual-mono file
 * (L == R) give mid equal to ffs_vad_levels of one channel byte for byte and side all zero.  Exactly n_frames bytes are
 * written to each output, each at any byte address, nothing behind them.  One pass over the PCM: 16-byte loads when
 * frame_len is a multiple of 4 and at most 512 pairs and pcm_dev is 16-byte aligned, a pair per lane otherwise (and for
 * the last frames of the buffer).  Stateless, no atomics, no allocation; can be called chunk by chunk like
 * ffs_vad_levels.  n_pairs == 0 is FFS_OK with nothing written.
 *
 * ffs_vad_centre_gate.  t is read ON THE DEVICE from threshold_dev when that is not NULL (a pick record's address works,
 * as for ffs_vad_level_labels; the value is taken as it stands), else it is threshold_host in [0, 256];
 * c = min_contrast_bins in [0, 255].
 *   out[f] = mid[f] if (int)mid[f] - (int)side[f] >= c, else 0          (does not depend on t)
 *   active(f) = mid[f] >= t;   kept(f) = active(f) and mid[f] - side[f] >= c
 * It follows: ffs_vad_level_labels(out, t) labels exactly the kept frames (for t >= 1), ffs_vad_steady_gate(out, t, ...)
 * sees a rejected frame as level 0, and for L == R and c <= t the labels are the mono path's byte for byte.
 * Record (one per call, 48 bytes, 8-byte aligned): the t and the c that were used, max_side the largest side level
 * (0 for no frames), the frames, the active and the kept frames, sum_contrast the signed sum of mid - side over the
 * active frames.  Flags:
 *   FFS_VAD_CENTRE_MONO          n_frames > 0 and max_side == 0: the file is dual mono, the gate decides nothing;
 *   FFS_VAD_CENTRE_ALL_REJECTED  n_active > 0 and n_kept == 0.
 * out_levels_dev may be NULL (the record alone) and may not overlap an input; n_frames == 0 writes the record alone.
 * Nothing is written behind out[n_frames - 1] or around the record.  The record is zeroed on the stream, a capped grid
 * adds each workgroup's integer sums into it with integer atomics (add, max: order-independent), one more wave writes
 * t, c, n_frames and the flags; no workgroup waits for another, nothing is allocated, nothing synchronises.
 * FFS_E_INVALID with a message that starts with the export's name, before any launch: a negative count, frame_len < 1,
 * n_edges outside [1, 255], threshold_host (without threshold_dev) or min_contrast_bins outside the ranges above, a null
 * pointer, PCM not 2-byte, edges or record not 8-byte, threshold_dev not 4-byte aligned, an output that overlaps an
 * input.  Stateless. */
#define FFS_VAD_CENTRE_MONO 1         /* no frame has a side level: dual mono */
#define FFS_VAD_CENTRE_ALL_REJECTED 2 /* active frames, none kept */

typedef struct ffs_vad_centre {
    int32_t threshold_bin;        /* the t that was used */
    int32_t flags;                /* FFS_VAD_CENTRE_* */
    int32_t min_contrast_bins;    /* the c that was used */
    int32_t max_side;             /* the largest side level, 0 for no frames */
    int64_t n_frames;
    int64_t n_active;             /* frames with mid >= t */
    int64_t n_kept;               /* of them, with mid - side >= c */
    int64_t sum_contrast;         /* signed sum of mid - side over the active frames */
} ffs_vad_centre;
#ifdef __cplusplus
static_assert(sizeof(ffs_vad_centre) == 48, "ffs_vad_centre is 48 bytes");
#else
_Static_assert(sizeof(ffs_vad_centre) == 48, "ffs_vad_centre is 48 bytes");
#endif

int ffs_vad_stereo_levels(const int16_t* pcm_dev, int64_t n_pairs, int frame_len, const double* edges_dev, int n_edges,
                          uint8_t* mid_levels_dev, uint8_t* side_levels_dev, void* hip_stream);
int ffs_vad_centre_gate(const uint8_t* mid_dev, const uint8_t* side_dev, int64_t n_frames, const int32_t* threshold_dev,
                        int threshold_host, int min_contrast_bins, uint8_t* out_levels_dev, ffs_vad_centre* record_dev,
                        void* hip_stream);

/* ---- progressive alignment: the quality report of a growing reference prefix (csrc/ffs_progressive.h) -----------
 * Replaces: nothing in the reference (its --multi-segment-sync, speech_transformers.py:760-903, samples eight minutes
 * and hopes they suffice).  Score counts are additive over the reference, so after every appended chunk of reference
 * samples the exact report of the prefix read so far costs one pass over the NEW samples.  Pinned against the numpy
 * model tests/progressive_model.py.
 *
 * A plan holds max_slots slots; a slot holds one file: a two-level reference prefix r[0, L) that grows by appends,
 * n_cand <= max_cand (<= 8) two-level candidate vectors s_c fixed at open, and the lag window d in [-W+1, W]
 * (W = max_offset_samples, n_lags = 2W <= max_lags <= 262144) fixed at open.  Subtitle sample i meets reference sample
 * i + d.  Score of candidate c at lag d at prefix length L: two_level_score of (n11, n1x, nx1) over the overlap
 * i in [max(0, -d), min(S_c, L - d)), exactly 0.0 where it is empty -- the scores of ffs_align_quality_batch on
 * (r[0, L), s_c), over this window whatever L is.
 *
 * ffs_prog_open (slot i of the call: slot[i]; its candidate c: entry i * max_cand + c of sub_ptr / sub_len / sub_lo /
 * sub_hi, the entries of c >= n_cand[i] are not read): the candidates (FFS_DTYPE_U1, device) are copied into the plan
 * on the stream, their prefix sums computed, curves and reference zeroed, L = 0.  Reopening an open slot is allowed and
 * leaves nothing of the old problem.
 * ffs_prog_append: bits [first_bit[i], first_bit[i] + n_new[i]) of the 32-bit words at chunk_dev[i] (device, 4-byte
 * aligned, first_bit in [0, 32): what ffs_vad_energy_bits wrote at a byte offset can be handed over in place) become
 * reference samples [L, L + n_new); n_new = 0 is allowed.  Only the words that hold those bits are loaded, no other
 * bit of them is interpreted.  Then, per slot of the call, cand_out_dev[i * max_cand + c] = the ffs_quality_result of
 * candidate c on the prefix (greedy top_k peaks at least exclusion_samples apart, largest lag on ties, two-pass moments,
 * FFS_QUALITY_FLAT, n_lags = 2W; zeros for c >= n_cand) and state_out_dev[i] = the slot's ffs_prog_state.
 * ffs_prog_reference: the plan's bits of the consumed prefix (device; valid until the slot is reopened or the plan
 * destroyed; bits at positions >= len are 0) and its length.  The call itself queues nothing and waits for nothing: a read
 * of the returned pointer must be ordered behind the stream of the slot's last ffs_prog_append (queue it on that stream,
 * or behind an event recorded there).  ffs_prog_close marks slots as not open.
 *
 * Everything is queued on hip_stream; host arrays may be freed on return.  The plan keeps L per slot on the host, so
 * every refusal (FFS_E_INVALID) happens before any launch, with state and outputs untouched: a null or misaligned
 * pointer, first_bit outside [0, 32), n_new < 0, L + n_new > max_ref_samples, a slot out of range, not open (append,
 * reference, close) or named twice in one call, n_cand outside [1, max_cand], a candidate length < 1 or >
 * max_sub_samples, W < 1 or 2W > max_lags, non-finite levels, top_k outside [1, 8], exclusion_samples < 1.
 * ffs_prog_plan_destroy waits for pending work.
 *
 * Workspace (ffs_prog_plan_workspace_bytes), with lpad = max_lags rounded up to 64 and words(x) = x / 32 + 2 rounded up
 * to 16:  max_slots * (8 * words(max_ref_samples) + max_cand * (8 * words(max_sub_samples) + 12 * lpad)) bytes, plus
 * the descriptors of one call (less than 256 bytes per slot and candidate, not counted). */
typedef struct ffs_prog_state {
    int64_t ref_len;    /* L after the append */
    int64_t offset;     /* peak 1 of the best candidate (samples) */
    double score;       /* its score */
    double mean, std;   /* of the best candidate's curve */
    double runner_up;   /* the best candidate's peak-2 score; NaN when it has none */
    double other_best;  /* the largest peak-1 score among the other candidates; NaN with one candidate */
    int32_t best_cand;  /* the largest peak-1 score, the smallest candidate index on ties */
    int32_t flags;      /* the best candidate's FFS_QUALITY_* flags */
} ffs_prog_state;
#ifdef __cplusplus
static_assert(sizeof(ffs_prog_state) == 64, "ffs_prog_state is 64 bytes");
#else
_Static_assert(sizeof(ffs_prog_state) == 64, "ffs_prog_state is 64 bytes");
#endif

typedef struct ffs_prog_plan ffs_prog_plan;
int ffs_prog_plan_create(int device, int max_slots, int max_cand, int64_t max_lags, int64_t max_ref_samples,
                         int64_t max_sub_samples, ffs_prog_plan** out);
int ffs_prog_plan_destroy(ffs_prog_plan* plan);
int64_t ffs_prog_plan_workspace_bytes(const ffs_prog_plan* plan);
int ffs_prog_open(ffs_prog_plan* plan, int n, const int32_t* slot, const int32_t* n_cand, const void* const* sub_ptr,
                  const int64_t* sub_len, const double* sub_lo, const double* sub_hi, const double* ref_lo,
                  const double* ref_hi, const int64_t* max_offset_samples, void* hip_stream);
int ffs_prog_append(ffs_prog_plan* plan, int n, const int32_t* slot, const void* const* chunk_dev, const int32_t* first_bit,
                    const int64_t* n_new, int top_k, int64_t exclusion_samples, ffs_quality_result* cand_out_dev,
                    ffs_prog_state* state_out_dev, void* hip_stream);
int ffs_prog_reference(ffs_prog_plan* plan, int slot, const uint32_t** bits_dev, int64_t* len);
int ffs_prog_close(ffs_prog_plan* plan, int n, const int32_t* slot);

/* ---- sampled alignment: masked scores for a reference read in segments (csrc/ffs_sampled.h) ----------------------
 * Replaces: the score behind the reference's --multi-segment-sync (MultiSegmentVideoSpeechTransformer,
 * speech_transformers.py:760-903), which places a few decoded windows in a vector that is zero everywhere else, so that
 * every cue on unread audio is charged as a mismatch.  Here unread frames contribute nothing.  Pinned against the numpy
 * model tests/sampled_model.py.
 *
 * A sampled slot of an ffs_prog_plan holds a reference of declared length T = ref_total (1 <= T <= max_ref_samples) of
 * which disjoint intervals [a, b) arrive in any order; K is their union (abutting intervals merge; at most
 * FFS_PROG_MAX_INTERVALS merged intervals).  Candidates, levels and the lag window d in [-W+1, W] are ffs_prog_open's.
 * Counts of candidate c at lag d over I(d) = { i : 0 <= i < S_c, i + d in K }: ov = |I|, n11 = sum_I s[i] r[i+d],
 * n1x = sum_I s[i], nx1 = sum_I r[i+d].  Score: exactly 0.0 where ov = 0, else two_level_score's expression on
 * (n11, n1x, nx1) with this ov in place of the overlap length -- what the reference aligner computes on a reference
 * vector that holds 0.5 in every unread frame (2 * 0.5 - 1 = 0).  The records for a given K do not depend on the order
 * or the cutting of the appends (all sums are integers), and for K = [0, L) they are ffs_prog_append's byte for byte.
 *
 * ffs_prog_open_sampled: ffs_prog_open plus ref_total[i]; K is empty.  A slot may be reopened as either kind.
 * ffs_prog_append_at: bits [first_bit[i], first_bit[i] + n_new[i]) of the words at chunk_dev[i] become reference samples
 * [position[i], position[i] + n_new[i]); then the candidates' ffs_quality_result records and the slot's ffs_prog_state
 * (ref_len = |K|), as ffs_prog_append writes them.  n_new = 0 re-reports.  The cost of an append does not depend on
 * what is already known, except that the slot's prefix popcounts are recomputed from position to T.
 * ffs_prog_known (host only; queues nothing): the merged intervals, ascending, as bounds_out[2k], bounds_out[2k + 1];
 * *n_out of them; FFS_E_INVALID when cap is too small.
 * ffs_prog_reference on a sampled slot: the bits (zero outside K) and len = T.
 * ffs_prog_plan_sampled_bytes: what sampled slots add to the plan, made by the first ffs_prog_open_sampled (0 before):
 * 12 * lpad bytes per slot and candidate for the ov, n1x, nx1 curves, the descriptors of one call, and the host's
 * interval tables (16 * FFS_PROG_MAX_INTERVALS bytes per slot).  ffs_prog_plan_workspace_bytes does not include it.
 *
 * Every refusal is FFS_E_INVALID before any launch, state and outputs untouched: everything ffs_prog_open /
 * ffs_prog_append refuse, T outside [1, max_ref_samples], position < 0 or position + n_new > T, an interval that
 * overlaps K, more than FFS_PROG_MAX_INTERVALS intervals after merging, ffs_prog_append on a sampled slot,
 * ffs_prog_append_at on a prefix slot. */
#define FFS_PROG_MAX_INTERVALS 256
int ffs_prog_open_sampled(ffs_prog_plan* plan, int n, const int32_t* slot, const int32_t* n_cand, const void* const* sub_ptr,
                          const int64_t* sub_len, const double* sub_lo, const double* sub_hi, const double* ref_lo,
                          const double* ref_hi, const int64_t* max_offset_samples, const int64_t* ref_total,
                          void* hip_stream);
int ffs_prog_append_at(ffs_prog_plan* plan, int n, const int32_t* slot, const void* const* chunk_dev, const int32_t* first_bit,
                       const int64_t* position, const int64_t* n_new, int top_k, int64_t exclusion_samples,
                       ffs_quality_result* cand_out_dev, ffs_prog_state* state_out_dev, void* hip_stream);
int ffs_prog_known(ffs_prog_plan* plan, int slot, int64_t* bounds_out, int cap, int* n_out);
int64_t ffs_prog_plan_sampled_bytes(const ffs_prog_plan* plan);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char* ffs_last_error(void);

/* Library/ABI version (major*10000 + minor*100 + patch). */
int ffs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FFSUBSYNC_AMD_H */
