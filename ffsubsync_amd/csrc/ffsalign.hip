// ffsalign.hip -- host side of libffsalign.so: plans, descriptor building, kernel dispatch and
// the extern "C" entry points declared in include/ffsubsync_amd.h.
//
// Written for gfx950 (MI355X) only: hipcc --offload-arch=gfx950.
#include <hip/hip_runtime.h>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <immintrin.h>
#define FFS_HOST_AVX2 1  // host pass only: the device pass parses host functions too, without the x86 headers
#else
#define FFS_HOST_AVX2 0
#endif
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/ffsubsync_amd.h"
#include "ffs_kernels.h"
#include "ffs_runs.h"
#include "ffs_split.h"
#include "ffs_quality.h"
#include "ffs_match.h"
#include "ffs_split_report.h"
#include "ffs_split_refine.h"
#include "ffs_drift_refine.h"
#include "ffs_split_range.h"
#include "ffs_cut_report.h"
#include "ffs_drift.h"
#include "ffs_drift_report.h"
#include "ffs_cue_report.h"
#include "ffs_cue_retime.h"
#include "ffs_drift_smooth.h"
#include "ffs_drift_range.h"
#include "ffs_drift_range_smooth.h"
#include "ffs_drift_range_report.h"
#include "ffs_sweep.h"
#include "ffs_surrogate.h"
#include "ffs_stability.h"
#include "ffs_progressive.h"
#include "ffs_sampled.h"
#include "ffs_adaptive_vad.h"
#include "ffs_vad_gate.h"
#include "ffs_stereo_vad.h"

using namespace ffsa;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(FFS_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// run `stmt` with a compile-time DT equal to the runtime element type (0 = bytes, 1 = float, 2 = bit-packed, 3 = double)
#define FFS_BY_DTYPE(dtype, stmt)              \
    do {                                       \
        if ((dtype) == FFS_DTYPE_U8) {         \
            constexpr int DT = 0;              \
            stmt;                              \
        } else if ((dtype) == FFS_DTYPE_F32) { \
            constexpr int DT = 1;              \
            stmt;                              \
        } else if ((dtype) == FFS_DTYPE_F64) { \
            constexpr int DT = 3;              \
            stmt;                              \
        } else {                               \
            constexpr int DT = 2;              \
            stmt;                              \
        }                                      \
    } while (0)

// the exact re-evaluation kernels: DT as above, or 4 when the reference and the candidates differ in element type
#define FFS_BY_RESCORE_DTYPE(mixed, dtype, stmt)  \
    do {                                          \
        if (mixed) {                              \
            constexpr int DT = 4;                 \
            stmt;                                 \
        } else if ((dtype) == FFS_DTYPE_U8) {     \
            constexpr int DT = 0;                 \
            stmt;                                 \
        } else if ((dtype) == FFS_DTYPE_F32) {    \
            constexpr int DT = 1;                 \
            stmt;                                 \
        } else if ((dtype) == FFS_DTYPE_F64) {    \
            constexpr int DT = 3;                 \
            stmt;                                 \
        } else {                                  \
            constexpr int DT = 2;                 \
            stmt;                                 \
        }                                         \
    } while (0)

constexpr int64_t kMinFftN = 4096;  // shorter problems go to the exact direct kernel
constexpr int64_t kMaxFftN = 1 << 24;
constexpr unsigned kPoolCapacity = 1u << 20;
// FFS_ALGO_AUTO: boundary coincidences per candidate, per point of the plan's transform length and packed transform slot
// the candidate occupies, above which the transforms take over.  Measured break-even (profiles/budget_probe.py, round 5):
// +-60 s window: ~20 per point of N = 3 * 2^18 (lists of 17 k x 20 k boundaries); no window: ~13 per point of N = 3 * 2^19
// (118 lag tiles per candidate cost as much as 6 M coincidences).  Twelve keeps the choice on the winning side in both.
constexpr long long kRunsBudgetPerPoint = 12;
// Plan-owned boundary lists (vectors that arrive as bits) start with room for this many entries each -- subtitle-like vectors
// have ~2 000 -- and the stride grows (x 4, up to RUNS_CAP) when a call meets a longer list: that same call is solved again
// with the longer stride (align_impl), and the plan keeps it.  A 256 KB stride for 16 KB lists cost 4 % of k_runs_extract
// (65 536 lists spread over 16 GB of address space).
constexpr int kRunsStride0 = 4096;
// calls of at most this many candidates upload their descriptors once and launch the extraction behind them (see late_extract)
constexpr size_t kSmallCallCands = 4096;
constexpr int kSegBlocks = 3;    // blocks per candidate in block-segmented mode (n_fft = 3 * block transform length)
constexpr int kCollectRows = 4;  // grid rows of the exhaustive last pass (each walks the flagged-candidate list)

int ilog2(int64_t x) {
    int p = 0;
    while ((int64_t(1) << p) < x) ++p;
    return p;
}

// column-tile width for a column transform of length L
int tile_cols(int L) {
    if (L % 3 == 0) {  // 3 * 2^k columns: 48, 96, 192, 384, 768
        const int c = 3072 / L;
        return c < 16 ? 16 : c;
    }
    if (L <= 16) return 256;
    if (L <= 128) return 4096 / L;
    if (L <= 1024) return 16;
    if (L == 2048) return 8;
    return 4;
}

size_t col_lds_bytes(int L) {
    size_t t = (L > 16) ? (size_t)L * tile_cols(L) * sizeof(cf) : 0;
    if (L % 3 == 0) t += (size_t)L * sizeof(cf);  // W_L^k for the radix-3 combine
    return t < 2048 ? 2048 : t;  // the byte / bit input staging of pass A needs up to 2 KB on its own
}
size_t row_lds_bytes(int L) {
    const int rows = 256 / (L / 16);
    return (size_t)rows * (L + L / 16) * sizeof(cf);
}

// stage tables of Shape<L>: stage 1 (Ns = 16) then stage 2 (Ns = 256).  A radix-16 stage stores the
// six powers e in {1,2,3,4,8,12} of w = exp(-2*pi*i*jm/(Ns*16)) as [6][Ns]; a smaller radix R stores
// w^r as [R][Ns].
std::vector<cf> make_stage_tables(int L) {
    const int LT = L / 16;
    const int R1 = LT >= 16 ? 16 : LT;
    const int R2 = L / (16 * R1);
    std::vector<cf> t;
    auto add = [&](int R, int Ns) {
        static const int pw16[6] = {1, 2, 3, 4, 8, 12};
        const int rows = (R == 16) ? 6 : R;
        for (int i = 0; i < rows; ++i)
            for (int jm = 0; jm < Ns; ++jm) {
                const int e = (R == 16) ? pw16[i] : i;
                const double a = -2.0 * M_PI * (double)e * (double)jm / ((double)Ns * (double)R);
                t.push_back(mk((float)cos(a), (float)sin(a)));
            }
    };
    if (R1 > 1) add(R1, 16);
    if (R2 > 1) add(R2, 256);
    if (t.empty()) t.push_back(mk(1.f, 0.f));
    return t;
}

// Transform lengths 3 * 2^k the kernels can run: N = N1 * N2 with N1 = 3 * 2^j in [48, 768] columns.
bool radix3_length(int64_t n) {
    if (n % 3) return false;
    const int64_t m = n / 3;
    return (m & (m - 1)) == 0 && n >= 48 * 256 && n <= 768 * 4096;
}

cf wn(int64_t N, int64_t p) {
    p %= N;
    const double a = -2.0 * M_PI * (double)p / (double)N;
    return mk((float)cos(a), (float)sin(a));
}

}  // namespace

struct ffs_plan {
    int device = 0;
    int64_t N = 0;
    int N1 = 0, N2 = 0, C = 0, log2C = 0;
    int log2CL = 0;  // tile layout T[x/CL][k1][x%CL]: CL = max(C, 64) columns (512-byte row chunks)
    int pairs_in_flight = 0, max_cand = 0, max_slots = 0;
    int pass_a_prefetch = 3;  // grid rows the input prefetch blocks of pass A run ahead, byte inputs (FFS_PASS_A_PREFETCH, 0 = off)
    int pass_a_prefetch_bits = 12;  // the same for bit-packed inputs, in rows of a 2^18-point transform (scaled by length)
    bool direct_only = false;
    // the five run-time knobs; none of them can change a result
    bool allow_pruned = true;       // FFS_DISABLE_PRUNED_PASS_C=1 forces the full last pass
    bool allow_half_last = true;    // FFS_DISABLE_HALF_LAST=1: store all rows of a single-candidate last slot
    int lab_flags = 0;              // lab build only (make lab): DBG_* section switches, timing only
    // device tables
    cf *tw1 = nullptr, *tw2 = nullptr;        // stage tables for N1 / N2
    cf *tbA = nullptr, *tsA = nullptr;        // pass A inter twiddles: [N1/16][N2], [16][N2]
    cf* tw1h = nullptr;                       // stage tables of the 256-row sub-transforms of a 512-row column
    cf *tbR = nullptr, *tsR = nullptr, *thR = nullptr;  // pass-A twiddles of the three-sub-transforms-per-thread columns (k_pass_a3)
    cf *tbM = nullptr, *tsM = nullptr;        // mid inter twiddles:    [N1][N2/16], [N1][16]
    cf* twn1 = nullptr;                       // W_N1^k, k < N1 (pruned pass C)
    cf* work = nullptr;                       // [pairs_in_flight][max_slots][N]
    BlockNom* bnom = nullptr;                 // [pairs_in_flight*n_packed*2][tiles]
    PoolEntry* pool_entries = nullptr;        // [kPoolCapacity] exhaustive fallback for flagged candidates
    int* xlist = nullptr;                     // [1 + pairs_in_flight*max_cand] flagged candidates of the sub-batch
    // Block-segmented mode (n_fft = 3*M, M = 2^k >= 2^16): a complete power-of-two plan of length M with
    // room for three blocks per pair; used when the lag window is narrow enough (ffs_align_batch)
    ffs_plan* seg = nullptr;
    bool allow_seg = true;                    // FFS_DISABLE_SEGMENTED=1
    // per-call descriptor storage (grown on demand)
    void* dev_desc = nullptr;
    size_t dev_desc_bytes = 0;
    void* host_desc = nullptr;                // pinned
    size_t host_desc_bytes = 0;
    hipEvent_t upload_done = nullptr;
    // Run-boundary calls that extract lists upload their descriptors on a COPY STREAM (one per device, shared by the plans)
    // into one of TWO device blocks (dev_desc / dev_desc2, alternating): the vector table of call k + 1 goes up while
    // call k's correlation runs, a large call's candidate descriptors while the extraction of their own call runs -- on
    // one stream the uploads sat between the kernels with the device idle (126 + 70 us of a 3.3 ms step of 8192 pairs,
    // ~20 us of a 111 us step of 128: profiles/large_step_timeline.py, small_step_timeline.py).
    void* dev_desc2 = nullptr;
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_ev = nullptr;                 // the vector table of the current call has arrived
    hipEvent_t half_done[2] = {nullptr, nullptr};  // the last call that used block h has finished
    bool half_used[2] = {false, false};
    int cur_half = 0;                             // the block the current (or most recent) call uses
    // The workspace, descriptor and nominee buffers are reused by every call: a call on another stream
    // than the previous one first waits for that one's last kernel (same-stream calls are ordered anyway).
    hipEvent_t last_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
    int64_t workspace_bytes = 0;
    bool radix3_off = false;                  // FFS_DISABLE_RADIX3=1 when the plan was created (ffs_plan_length)
    bool workspace_ready = false;             // every buffer of ensure_workspace is allocated (all or nothing)
    // Run-boundary path (ffs_runs.h): FFS_ALGO_AUTO sends every sub-batch of bit-packed two-level vectors whose boundary
    // lists are short enough through it (one event wait per call to read the list lengths), the others through the
    // transforms; FFS_ALGO_FFT never uses it; FFS_ALGO_RUNS ignores the coincidence budget (truncated lists still go
    // through the transforms).  Buffers grown on demand.
    int algo = FFS_ALGO_AUTO;
    int runs_split = 0;                 // FFS_RUNS_SPLIT: workgroups per pair in k_runs_corr (0: the rule at the launch site)
    long long runs_budget = -1;         // FFS_RUNS_BUDGET: boundary coincidences per candidate above which the transforms take over (-1: the rule in ffs_plan_create)
    int2* runs_e = nullptr;             // [vectors][runs_stride] lists of the vectors that arrive as bits: references and threshold planes as
                                        // (boundary position, ones in front of it), candidates as 4-byte positions only (RunsRef, COMPACT)
    int runs_stride = 4096;             // entries per plan-owned list (kRunsStride0; FFS_RUNS_STRIDE; grows up to RUNS_CAP)
    size_t runs_e_entries = 0;          // entries allocated behind runs_e
    int2* runs_n = nullptr;             // [vectors] (boundaries, ones)
    size_t runs_vecs = 0;               // vectors the two buffers above have room for
    unsigned* pack_buf = nullptr;       // bit-packed images of a call's FFS_DTYPE_U8 vectors / of list-only vectors that need the transforms
    size_t pack_bytes = 0;
    int* runs_flags = nullptr;          // [sub-batches] 1 = goes through the transforms, 2 = unusable list (k_runs_chunk_flags); then the
                                        // 8-byte boundary counter of the call
    int* runs_zero_flags = nullptr;     // [sub-batches] zeros: calls whose host-known list bounds rule the transforms out
    int* runs_flags_host = nullptr;     // pinned copy of runs_flags
    size_t runs_flags_n = 0;
    RunsBest* runs_best = nullptr;      // [candidates][tiles] (windows wider than one tile)
    size_t runs_best_n = 0;
    bool runs_prev_fft = false;         // the previous run-boundary call needed the transforms for some sub-batch
    unsigned* lvl_buf = nullptr;        // threshold planes of a call's multi-level (float) references
    size_t lvl_bytes = 0;
    hipEvent_t runs_ev = nullptr;
    int64_t runs_calls = 0, runs_fft_chunks = 0, runs_chunks = 0, runs_last_boundaries = 0;  // statistics (ffs_plan_runs_stats)
    // What the most recent ffs_align_batch* call launched for its transform sub-batches (ffs_plan_dispatch_report): every
    // launch function notes its choice here, on the plan whose kernels it starts (the sub-plan in block-segmented mode;
    // launch_transform_chunk copies that to the call's plan).
    mutable ffs_dispatch_report dispatch = {};
    // FFS_HOST_TIMING=1: host nanoseconds of the run-boundary calls by section, printed when the plan is destroyed
    bool host_timing = false;
    double ht_vec = 0, ht_cand = 0, ht_wait = 0, ht_decide = 0, ht_total = 0;
    // kernels whose dynamic-LDS limit has been raised on this plan's device (the attribute is per device)
    mutable std::vector<const void*> lds_configured;
    // optional per-kernel event timing
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;            // reusable events
    size_t ev_used = 0;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_spans;  // (kernel id, (start, stop))
};

namespace {

template <class T>
int upload(T** dst, const std::vector<T>& src, int64_t* total) {
    HIP_TRY(hipMalloc((void**)dst, src.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *total += (int64_t)(src.size() * sizeof(T));
    return FFS_OK;
}

int ensure_desc(ffs_plan* p, size_t bytes) {
    if (bytes <= p->dev_desc_bytes) return FFS_OK;
    if (p->upload_done) HIP_TRY(hipEventSynchronize(p->upload_done));
    if (p->dev_desc) HIP_TRY(hipFree(p->dev_desc));
    if (p->dev_desc2) HIP_TRY(hipFree(p->dev_desc2));  // (allocated again by ensure_copy, at the new size)
    p->dev_desc2 = nullptr;
    p->half_used[1] = false;
    if (p->host_desc) HIP_TRY(hipHostFree(p->host_desc));
    p->dev_desc = nullptr;
    p->host_desc = nullptr;
    p->dev_desc_bytes = p->host_desc_bytes = 0;
    const size_t cap = bytes + bytes / 2 + 4096;
    HIP_TRY(hipMalloc(&p->dev_desc, cap));
    HIP_TRY(hipHostMalloc(&p->host_desc, cap, hipHostMallocDefault));
    p->dev_desc_bytes = p->host_desc_bytes = cap;
    return FFS_OK;
}

// The copy stream: ONE per device for every plan of the process, created on first use (the calling thread's current device
// is `device`) and never destroyed -- a stream per plan made plan creation slow enough to stretch the GPU test suite from
// 40 s to 7.6 min (round 6, first attempt).  Plans only ever queue their own descriptor uploads on it, each behind an
// event of their own that has long completed; what they share is the order of those uploads.
hipStream_t shared_copy_stream(int device) {
    static std::mutex mu;
    static hipStream_t streams[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[device] && hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        streams[device] = nullptr;
    }
    return streams[device];
}
// Copy stream, its event and the second descriptor block (see ffs_plan::dev_desc2); false: this call uploads on its own stream.
bool ensure_copy(ffs_plan* p) {
    if (!p->copy_stream) {
        p->copy_stream = shared_copy_stream(p->device);
        if (!p->copy_stream) return false;
    }
    if (!p->copy_ev && hipEventCreateWithFlags(&p->copy_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        p->copy_ev = nullptr;
        return false;
    }
    if (!p->dev_desc2 && hipMalloc(&p->dev_desc2, p->dev_desc_bytes) != hipSuccess) {
        (void)hipGetLastError();
        p->dev_desc2 = nullptr;
        return false;
    }
    return true;
}

// Raise a kernel's dynamic-LDS limit once per plan (tiles above 64 KB need it).
int ensure_lds(const ffs_plan* p, const void* fn, size_t bytes) {
    for (const void* f : p->lds_configured)
        if (f == fn) return FFS_OK;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    p->lds_configured.push_back(fn);
    return FFS_OK;
}

// Transform workspace of a plan (and of its block-segmented sub-plan), allocated on first use.  All or nothing: a failed
// allocation frees what this call had obtained, so a later call tries again instead of launching on null buffers.
int ensure_workspace(ffs_plan* p) {
    if (p->direct_only || p->workspace_ready) return FFS_OK;
    const size_t work_bytes = (size_t)p->pairs_in_flight * p->max_slots * p->N * sizeof(cf);
    const size_t bn_bytes = (size_t)p->pairs_in_flight * (p->max_slots - 1) * 2 * (p->N2 / p->C) * sizeof(BlockNom);
    bool ok = hipMalloc((void**)&p->work, work_bytes) == hipSuccess;
    ok = ok && hipMalloc((void**)&p->bnom, bn_bytes) == hipSuccess;
    ok = ok && hipMalloc((void**)&p->xlist, (1 + (size_t)p->pairs_in_flight * p->max_cand) * sizeof(int)) == hipSuccess;
    ok = ok && hipMalloc((void**)&p->pool_entries, (size_t)kPoolCapacity * sizeof(PoolEntry)) == hipSuccess;
    int rc = FFS_OK;
    if (!ok) {
        (void)hipGetLastError();
        rc = fail(FFS_E_NOMEM, "transform workspace of %zu bytes could not be allocated", work_bytes + bn_bytes);
    } else if (p->seg) {
        rc = ensure_workspace(p->seg);
    }
    if (rc) {
        (void)hipFree(p->work);
        (void)hipFree(p->bnom);
        (void)hipFree(p->xlist);
        (void)hipFree(p->pool_entries);
        p->work = nullptr;
        p->bnom = nullptr;
        p->xlist = nullptr;
        p->pool_entries = nullptr;
        return rc;
    }
    p->workspace_ready = true;
    return FFS_OK;
}

// Buffers of the run-boundary path: boundary lists for `n_vec` vectors that arrive as bits (0: every vector of the call
// brings its own list), `n_best` tile records, per-sub-batch flags.  Counted in
// ffs_plan_workspace_bytes (the Python plan cache budgets HBM by it).
int ensure_runs(ffs_plan* p, size_t n_vec, size_t n_best, size_t n_chunks) {
    if (!p->runs_ev) HIP_TRY(hipEventCreateWithFlags(&p->runs_ev, hipEventDisableTiming));
    auto quiesce = [&]() -> int {
        if (p->has_last) HIP_TRY(hipEventSynchronize(p->last_done));  // the previous call may still be using them
        return FFS_OK;
    };
    int rc;
    // more vectors, or a longer stride than the lists were allocated for: then every vector the plan had room for gets the
    // longer list at once (a stream of calls meets its longest list in a small call as readily as in a large one)
    if (n_vec > p->runs_vecs || (n_vec && p->runs_vecs * (size_t)p->runs_stride > p->runs_e_entries)) {
        if ((rc = quiesce())) return rc;
        (void)hipFree(p->runs_e);
        (void)hipFree(p->runs_n);
        p->workspace_bytes -= (int64_t)(p->runs_e_entries * sizeof(int2) + p->runs_vecs * sizeof(int2));
        p->runs_e = nullptr;
        p->runs_n = nullptr;
        const size_t old_vecs = p->runs_vecs;  // (a longer stride alone keeps the room for as many vectors as before)
        p->runs_vecs = 0;
        p->runs_e_entries = 0;
        const size_t cap = (n_vec > old_vecs ? n_vec : old_vecs) + n_vec / 4 + 64;
        const size_t entries = cap * (size_t)p->runs_stride;
        if (hipMalloc((void**)&p->runs_e, entries * sizeof(int2)) != hipSuccess ||
            hipMalloc((void**)&p->runs_n, cap * sizeof(int2)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p->runs_e);
            p->runs_e = nullptr;
            return fail(FFS_E_NOMEM, "boundary lists for %zu vectors (%zu bytes) could not be allocated", cap, entries * sizeof(int2));
        }
        p->runs_vecs = cap;
        p->runs_e_entries = entries;
        p->workspace_bytes += (int64_t)(entries * sizeof(int2) + cap * sizeof(int2));
    }
    if (n_best > p->runs_best_n) {
        if ((rc = quiesce())) return rc;
        (void)hipFree(p->runs_best);
        p->workspace_bytes -= (int64_t)(p->runs_best_n * sizeof(RunsBest));
        p->runs_best = nullptr;
        p->runs_best_n = 0;
        HIP_TRY(hipMalloc((void**)&p->runs_best, n_best * sizeof(RunsBest)));
        p->runs_best_n = n_best;
        p->workspace_bytes += (int64_t)(n_best * sizeof(RunsBest));
    }
    if (n_chunks > p->runs_flags_n) {
        if ((rc = quiesce())) return rc;
        (void)hipFree(p->runs_flags);
        (void)hipFree(p->runs_zero_flags);
        if (p->runs_flags_host) (void)hipHostFree(p->runs_flags_host);
        p->runs_flags = p->runs_zero_flags = p->runs_flags_host = nullptr;
        p->runs_flags_n = 0;
        const size_t cap = n_chunks + 64;  // (two 8-byte statistics sit behind the flags, 8-byte aligned: boundaries, longest list)
        const size_t bytes = ((cap * sizeof(int) + 7) & ~(size_t)7) + 16;
        HIP_TRY(hipMalloc((void**)&p->runs_flags, bytes));
        HIP_TRY(hipMalloc((void**)&p->runs_zero_flags, bytes));
        HIP_TRY(hipMemset(p->runs_zero_flags, 0, bytes));
        HIP_TRY(hipHostMalloc((void**)&p->runs_flags_host, bytes, hipHostMallocDefault));
        p->runs_flags_n = cap;
    }
    return FFS_OK;
}

// Calls on one plan from different streams: order them (see ffs_plan::last_done).
int enter_stream(ffs_plan* p, hipStream_t st) {
    if (p->has_last && p->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, p->last_done, 0));
    return FFS_OK;
}
int leave_stream(ffs_plan* p, hipStream_t st) {
    // (every call, whichever stream uploaded its descriptors: a later call's copy-stream upload into this block waits for it)
    HIP_TRY(hipEventRecord(p->half_done[p->cur_half], st));
    p->half_used[p->cur_half] = true;
    HIP_TRY(hipEventRecord(p->last_done, st));
    p->last_stream = st;
    p->has_last = true;
    return FFS_OK;
}

// Entry points without a plan work on whatever device owns the caller's buffer -- and leave the thread's current
// device as they found it (a torch process would otherwise see its current device change under it).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    int enter(const void* dev_ptr) {
        hipPointerAttribute_t attr;
        if (dev_ptr && hipPointerGetAttributes(&attr, dev_ptr) == hipSuccess) {
            HIP_TRY(hipGetDevice(&prev));
            if (attr.device != prev) {
                HIP_TRY(hipSetDevice(attr.device));
                switched = true;
            }
        } else {
            (void)hipGetLastError();  // not a tracked allocation: stay on the caller's current device
        }
        return FFS_OK;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

hipEvent_t prof_event(ffs_plan* p) {
    if (p->ev_used == p->ev_pool.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        p->ev_pool.push_back(e);
    }
    return p->ev_pool[p->ev_used++];
}

// RAII span: records start now and stop at scope exit when profiling is on
struct ProfSpan {
    ffs_plan* p;
    hipStream_t st;
    int id;
    hipEvent_t a = nullptr, b = nullptr;
    ProfSpan(ffs_plan* p_, hipStream_t st_, int id_) : p(p_), st(st_), id(id_) {
        if (!p->profiling) return;
        a = prof_event(p);
        b = prof_event(p);
        if (a && b) (void)hipEventRecord(a, st);
    }
    ~ProfSpan() {
        if (a && b) {
            (void)hipEventRecord(b, st);
            p->ev_spans.push_back({id, {a, b}});
        }
    }
};

// ---- kernel dispatch -------------------------------------------------------------------------
// Bit-packed inputs: how many grid rows (transforms) the prefetch blocks of pass A run ahead -- about the time of
// twelve 2^18-point transforms (measured plateau: 9-14 rows there), but at least four rows (2^21-point transforms:
// pass A 17.3 us/pair at one row ahead, 15.8 at four, 15.9 at twelve), 0 = off.
int bit_prefetch_rows(const ffs_plan* p) {
    if (p->pass_a_prefetch_bits <= 0) return 0;
    const long long rows = ((long long)p->pass_a_prefetch_bits << 18) / (long long)p->N;
    return (int)(rows < 4 ? 4 : (rows > 255 ? 255 : rows));
}

#ifndef FFS_PAIR_MAX_XF
#define FFS_PAIR_MAX_XF 64  // A/B builds: largest transform group that takes the paired transform
#endif
// row_sel = first | count << 16: only transforms [first, first + count) of every group (0 = all of them; see k_pass_a)
template <int L, int C, int DT>
int launch_pass_a_inst(const ffs_plan* p, const XformDesc* descs, int n_xf, int xf_per_pair, int slots_per_pair,
                       int ref_half, hipStream_t st, int row_sel) {
    const size_t lds = col_lds_bytes(L);
    int rc_lds;
    const int nt = p->N2 / C;
    // byte inputs: one prefetch block per 128-column line group and grid row (see the kernel)
    const int groups = p->N2 / 128;
    // bit-packed inputs: eight prefetch blocks per grid row, one per XCD (see the kernel)
    const int ahead = DT == 2 ? bit_prefetch_rows(p) : p->pass_a_prefetch;
    const int pf = (DT == 0 && ahead > 0 && nt % 8 == 0 && groups % 8 == 0) ? groups
                   : (DT == 2 && ahead > 0 && nt % 8 == 0) ? 8 : 0;
    // bit-packed inputs, reference slot and last candidate slot both half slots (one real vector each): one paired
    // column transform per group instead of two, in the same launch as the group's other transforms
    constexpr bool CAN_PAIR = DT == 2 && L % 3 != 0;
    const bool paired = CAN_PAIR && !row_sel && (ref_half & HALF_REF) && (ref_half & HALF_LAST) && xf_per_pair >= 2 &&
                        xf_per_pair <= FFS_PAIR_MAX_XF && xf_per_pair == slots_per_pair;
    const int grid_rows = row_sel ? (n_xf / xf_per_pair) * (row_sel >> 16) : n_xf;
    const int flags = ref_half | STORE_8B | (p->lab_flags & (31 << 10));
    ffs_dispatch_report& rep = p->dispatch;
    (row_sel && (row_sel & 0xffff) == 0 ? rep.pass_a_ref_family : rep.pass_a_family) = FFS_DISPATCH_PASS_A;
    rep.pass_a_paired = !paired ? 0 : xf_per_pair == 2 ? 1 : 2;
    if constexpr (CAN_PAIR) {
        if (paired) {
            const size_t lds_p = lds > (size_t)L * C * sizeof(cf) ? lds : (size_t)L * C * sizeof(cf);  // the whole column tile
            const int groups_y = n_xf / xf_per_pair;
            if (xf_per_pair == 2) {
                if ((rc_lds = ensure_lds(p, (const void*)k_pass_a<L, C, DT, 1>, lds_p))) return rc_lds;
                hipLaunchKernelGGL((k_pass_a<L, C, DT, 1>), dim3(nt + pf, groups_y), dim3((L / 16) * C), lds_p, st, descs, p->work,
                                   p->N2, (long long)p->N, p->tw1, p->tbA, p->tsA, p->twn1, p->log2CL, xf_per_pair,
                                   slots_per_pair, nt, ahead, (unsigned*)p->bnom, flags, 0);
            } else {
                if ((rc_lds = ensure_lds(p, (const void*)k_pass_a<L, C, DT, 2>, lds_p))) return rc_lds;
                hipLaunchKernelGGL((k_pass_a<L, C, DT, 2>), dim3(nt + pf, groups_y * (xf_per_pair - 1)), dim3((L / 16) * C), lds_p,
                                   st, descs, p->work, p->N2, (long long)p->N, p->tw1, p->tbA, p->tsA, p->twn1, p->log2CL,
                                   xf_per_pair, slots_per_pair, nt, ahead, (unsigned*)p->bnom, flags, 0);
            }
            HIP_TRY(hipGetLastError());
            return FFS_OK;
        }
    }
    if ((rc_lds = ensure_lds(p, (const void*)k_pass_a<L, C, DT>, lds))) return rc_lds;
    hipLaunchKernelGGL((k_pass_a<L, C, DT>), dim3(nt + pf, grid_rows), dim3((L / 16) * C), lds, st, descs, p->work, p->N2,
                       (long long)p->N, p->tw1, p->tbA, p->tsA, p->twn1, p->log2CL, xf_per_pair, slots_per_pair, nt, ahead,
                       (unsigned*)p->bnom, flags, row_sel);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// columns of length 3*LI with three sub-transforms per thread (bit-packed inputs): tiles of C = 4096/LI columns
bool col3r_ok(const ffs_plan* p) { return p->tbR && (p->N1 == 192 || p->N1 == 384 || p->N1 == 768 || p->N1 == 512); }
int col3r_cols(const ffs_plan* p) { return p->N1 == 512 ? 16 : 4096 / (p->N1 / 3); }

template <int NS, int LI, int C>
int launch_pass_a3_inst(const ffs_plan* p, const XformDesc* descs, int n_xf, int xf_per_pair, int slots_per_pair,
                        int ref_half, hipStream_t st, int row_sel) {
    const size_t lds = (size_t)LI * C * sizeof(cf);
    int rc_lds;
    const int nt = p->N2 / C;
    const int ahead = nt % 8 == 0 ? bit_prefetch_rows(p) : 0;  // eight prefetch blocks per grid row, one per XCD
    const cf* tw = NS == 2 ? p->tw1h : p->tw1;
    // reference slot and last candidate slot both half slots (one real vector each): one paired column transform
    const bool paired = !row_sel && (ref_half & HALF_REF) && (ref_half & HALF_LAST) && xf_per_pair >= 2 &&
                        xf_per_pair <= FFS_PAIR_MAX_XF && xf_per_pair == slots_per_pair;
    const int flags = ref_half | (ahead << 16);
    const dim3 gx(nt + (ahead ? 8 : 0));
    const int groups_y = n_xf / xf_per_pair;
    ffs_dispatch_report& rep = p->dispatch;
    (row_sel && (row_sel & 0xffff) == 0 ? rep.pass_a_ref_family : rep.pass_a_family) = FFS_DISPATCH_PASS_A3;
    rep.pass_a_paired = !paired ? 0 : xf_per_pair == 2 ? 1 : 2;
#define FFS_A3_LAUNCH(PM, GY)                                                                                              \
    do {                                                                                                                   \
        if ((rc_lds = ensure_lds(p, (const void*)k_pass_a3<NS, LI, C, PM>, lds))) return rc_lds;                          \
        hipLaunchKernelGGL((k_pass_a3<NS, LI, C, PM>), dim3(gx.x, (GY)), dim3(256), lds, st, descs, p->work, p->N2,        \
                           (long long)p->N, tw, p->tbR, p->tsR, p->thR, p->twn1, p->log2CL, xf_per_pair, slots_per_pair,  \
                           nt, flags, PM == 0 ? row_sel : 0);                                                              \
    } while (0)
    if (!paired)
        FFS_A3_LAUNCH(0, row_sel ? groups_y * (row_sel >> 16) : n_xf);
    else if (xf_per_pair == 2)
        FFS_A3_LAUNCH(1, groups_y);
    else
        FFS_A3_LAUNCH(2, groups_y * (xf_per_pair - 1));
#undef FFS_A3_LAUNCH
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

template <int NS, int LI, int C>
int launch_pass_c3_inst(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed, int n_slots,
                        int n_pairs, int half_last, hipStream_t st) {
    const size_t lds = (size_t)LI * C * sizeof(cf);
    int rc_lds;
    const cf* tw = NS == 2 ? p->tw1h : p->tw1;
    const int tiles = p->N2 / C;
    const int plain = n_packed - (half_last ? 1 : 0);  // slots with two candidates (or all of them without HALF_LAST)
    p->dispatch.last_family = FFS_DISPATCH_LAST_C3;
    if (plain > 0) {
        if ((rc_lds = ensure_lds(p, (const void*)k_pass_c3<NS, LI, C, false>, lds))) return rc_lds;
        hipLaunchKernelGGL((k_pass_c3<NS, LI, C, false>), dim3(tiles, n_pairs * plain), dim3(256), lds, st, p->work, p->N2,
                           (long long)p->N, tw, cands, first_cand, n_cand, n_packed, n_slots, p->bnom, p->log2CL, p->twn1, plain);
    }
    if (half_last) {  // the single-candidate slot: two real output columns per complex column transform
        if ((rc_lds = ensure_lds(p, (const void*)k_pass_c3<NS, LI, C, true>, lds))) return rc_lds;
        hipLaunchKernelGGL((k_pass_c3<NS, LI, C, true>), dim3(tiles / 2, n_pairs), dim3(256), lds, st, p->work, p->N2,
                           (long long)p->N, tw, cands, first_cand, n_cand, n_packed, n_slots, p->bnom, p->log2CL, p->twn1, 1);
    }
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}
int launch_pass_c3(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed, int n_slots,
                   int n_pairs, int half_last, hipStream_t st) {
    switch (p->N1) {
        case 192: return launch_pass_c3_inst<3, 64, 64>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, half_last, st);
        case 384: return launch_pass_c3_inst<3, 128, 32>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, half_last, st);
        case 768: return launch_pass_c3_inst<3, 256, 16>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, half_last, st);
        case 512: return launch_pass_c3_inst<2, 256, 16>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, half_last, st);
    }
    return fail(FFS_E_INVALID, "unsupported column length %d", p->N1);
}

template <int DT>
int launch_pass_a(const ffs_plan* p, const XformDesc* descs, int n_xf, int xf_per_pair, int slots_per_pair, int ref_half,
                  hipStream_t st, int row_sel = 0) {
    if (DT == 2 && col3r_ok(p)) {
        switch (p->N1) {
            case 192: return launch_pass_a3_inst<3, 64, 64>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
            case 384: return launch_pass_a3_inst<3, 128, 32>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
            case 768: return launch_pass_a3_inst<3, 256, 16>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
            case 512: return launch_pass_a3_inst<2, 256, 16>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        }
    }
    switch (p->N1) {
        case 48: return launch_pass_a_inst<48, 64, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 96: return launch_pass_a_inst<96, 32, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 192: return launch_pass_a_inst<192, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 384: return launch_pass_a_inst<384, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 768: return launch_pass_a_inst<768, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 16: return launch_pass_a_inst<16, 256, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 32: return launch_pass_a_inst<32, 128, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 64: return launch_pass_a_inst<64, 64, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 128: return launch_pass_a_inst<128, 32, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 256: return launch_pass_a_inst<256, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 512: return launch_pass_a_inst<512, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 1024: return launch_pass_a_inst<1024, 16, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 2048: return launch_pass_a_inst<2048, 8, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
        case 4096: return launch_pass_a_inst<4096, 4, DT>(p, descs, n_xf, xf_per_pair, slots_per_pair, ref_half, st, row_sel);
    }
    return fail(FFS_E_INVALID, "unsupported column length %d", p->N1);
}

template <int L, bool SEP>
int launch_mid_inst(const ffs_plan* p, int n_pairs, int n_slots, int ref_half, hipStream_t st) {
    const size_t lds = row_lds_bytes(L);
    int rc_lds;
    if ((rc_lds = ensure_lds(p, (const void*)k_mid<L, SEP>, lds))) return rc_lds;
    constexpr int ROWS = 256 / (L / 16);
    dim3 grid(p->N1 / ROWS, n_pairs);
    p->dispatch.mid_family = FFS_DISPATCH_MID;
    hipLaunchKernelGGL((k_mid<L, SEP>), grid, dim3(256), lds, st, p->work, p->N1, p->log2CL, (long long)p->N, n_slots,
                       (float)(1.0 / (double)p->N), p->tw2, p->tbM, p->tsM, ref_half);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// the reference slot may hold only its rows 0..N1/2 (see k_mid) when one block handles one row
bool ref_half_ok(const ffs_plan* p) { return p->N2 == 4096 && (p->N2 / 16) >= (1 << p->log2CL) && p->N1 % 2 == 0; }

int launch_mid(const ffs_plan* p, int n_pairs, int n_slots, int ref_half, hipStream_t st) {
    const bool sep = (p->N2 / 16) >= (1 << p->log2CL);
    if (p->N2 == 4096 && sep) {  // one row per block: candidate rows requested one item ahead
        const size_t lds = row_lds_bytes(4096);
        int rc_lds;
        if ((rc_lds = ensure_lds(p, (const void*)k_mid<4096, true, true>, lds))) return rc_lds;
        p->dispatch.mid_family = FFS_DISPATCH_MID;
        hipLaunchKernelGGL((k_mid<4096, true, true>), dim3(p->N1, n_pairs), dim3(256), lds, st, p->work, p->N1, p->log2CL,
                           (long long)p->N, n_slots, (float)(1.0 / (double)p->N), p->tw2, p->tbM, p->tsM, ref_half);
        HIP_TRY(hipGetLastError());
        return FFS_OK;
    }
#define FFS_MID(L) \
    case L: return sep ? launch_mid_inst<L, true>(p, n_pairs, n_slots, ref_half, st) : launch_mid_inst<L, false>(p, n_pairs, n_slots, ref_half, st)
    switch (p->N2) {
        FFS_MID(256);
        FFS_MID(512);
        FFS_MID(1024);
        FFS_MID(2048);
        FFS_MID(4096);
    }
#undef FFS_MID
    return fail(FFS_E_INVALID, "unsupported row length %d", p->N2);
}

int launch_mid_seg(const ffs_plan* sp, int n_pairs, int n_slots, int n_blocks, int ref_half, hipStream_t st) {
    int rc_lds;
    const size_t lds = row_lds_bytes(4096);
    const size_t ldsp = row_lds_bytes(4096) + 4096 * sizeof(cf);  // + conj(R_k)/N parked next to the row buffer
    const float inv_n = (float)(1.0 / (double)sp->N);
    const int flags = ref_half | PAIR_ROWS;
    const int mid_lab = sp->lab_flags & (DBG_NO_FFT | DBG_HOT_MEM | DBG_NO_STORE);
    if (n_slots - 1 == 1) {  // one packed slot (every FFTAligner.fit): one accumulator row, three blocks per CU
        sp->dispatch.mid_family = FFS_DISPATCH_MID_SEG_ONE_1;
        if ((rc_lds = ensure_lds(sp, (const void*)k_mid_seg_one<4096, false, 1>, lds))) return rc_lds;
        hipLaunchKernelGGL((k_mid_seg_one<4096, false, 1>), dim3(sp->N1, n_pairs), dim3(256), lds, st, sp->work, sp->N1,
                           sp->log2CL, (long long)sp->N, n_slots, n_blocks, inv_n, sp->tw2, sp->tbM, sp->tsM, flags | mid_lab);
    } else if (n_slots - 1 <= 4) {  // single sweep: all (<= 4) candidate slots accumulate at once
        sp->dispatch.mid_family = FFS_DISPATCH_MID_SEG_ONE_4;
        if ((rc_lds = ensure_lds(sp, (const void*)k_mid_seg_one<4096, true>, ldsp))) return rc_lds;
        hipLaunchKernelGGL((k_mid_seg_one<4096, true>), dim3(sp->N1, n_pairs), dim3(256), ldsp, st, sp->work, sp->N1,
                           sp->log2CL, (long long)sp->N, n_slots, n_blocks, inv_n, sp->tw2, sp->tbM, sp->tsM, flags | mid_lab);
    } else {  // nine or more candidates: two slots per sweep
        sp->dispatch.mid_family = FFS_DISPATCH_MID_SEG_PIPE;
        if ((rc_lds = ensure_lds(sp, (const void*)k_mid_seg_pipe<4096>, ldsp))) return rc_lds;
        hipLaunchKernelGGL((k_mid_seg_pipe<4096>), dim3(sp->N1, n_pairs), dim3(256), ldsp, st, sp->work, sp->N1, sp->log2CL,
                           (long long)sp->N, n_slots, n_blocks, inv_n, sp->tw2, sp->tbM, sp->tsM, flags);
    }
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

struct PoolArgs {
    const NomList* noms;
    PoolHeader* header;
    PoolEntry* entries;
    PoolBest* best;
    int shares;  // sub-batches of the call that share the pool (each flagged candidate's quota is divided by it)
    int half_last = 0;  // HALF_LAST layout of the last candidate slot (see ffs_kernels.h)
};

template <int L, int C, int MODE>
int launch_pass_c_inst(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed, int n_slots,
                       int n_pairs, float* out_a, float* out_b, const PoolArgs& pa, hipStream_t st) {
    const size_t lds = col_lds_bytes(L);
    int rc_lds;
    if ((rc_lds = ensure_lds(p, (const void*)k_pass_c<L, C, MODE>, lds))) return rc_lds;
    dim3 grid(p->N2 / C, MODE == 2 ? kCollectRows : n_pairs * n_packed);
    if (MODE == 0) p->dispatch.last_family = FFS_DISPATCH_LAST_FULL;
    if (MODE == 2) p->dispatch.sweep_family = FFS_DISPATCH_LAST_FULL;
    hipLaunchKernelGGL((k_pass_c<L, C, MODE>), grid, dim3((L / 16) * C), lds, st, p->work, p->N2, (long long)p->N, p->tw1,
                       cands, first_cand, n_cand, n_packed, n_slots, p->bnom, out_a, out_b, pa.noms, pa.header, pa.entries, p->log2CL,
                       p->twn1, p->xlist, pa.best, pa.shares, pa.half_last);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

template <int MODE>
int launch_pass_c(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed, int n_slots,
                  int n_pairs, float* out_a, float* out_b, const PoolArgs& pa, hipStream_t st) {
#define FFS_PC(L, C) \
    case L: return launch_pass_c_inst<L, C, MODE>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, out_a, out_b, pa, st)
    switch (p->N1) {
        FFS_PC(48, 64);
        FFS_PC(96, 32);
        FFS_PC(192, 16);
        FFS_PC(384, 16);
        FFS_PC(768, 16);
        FFS_PC(16, 256);
        FFS_PC(32, 128);
        FFS_PC(64, 64);
        FFS_PC(128, 32);
        FFS_PC(256, 16);
        FFS_PC(512, 16);
        FFS_PC(1024, 16);
        FFS_PC(2048, 8);
        FFS_PC(4096, 4);
    }
#undef FFS_PC
    return fail(FFS_E_INVALID, "unsupported column length %d", p->N1);
}

size_t pruned_lds_bytes(int L) {
    const int C = tile_cols(L), LT = L / 16;
    return 1024 + (size_t)L * sizeof(cf) + (size_t)MAXBINS * LT * C * sizeof(cf);
}

template <int L, int C, bool EXH>
int launch_pass_c_pruned_inst(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed,
                              int n_slots, int n_pairs, const BinList& bins, const PoolArgs& pa, hipStream_t st, int seg,
                              int seg_shift) {
    const size_t lds = pruned_lds_bytes(L);
    int rc_lds;
    if ((rc_lds = ensure_lds(p, (const void*)k_pass_c_pruned<L, C, EXH>, lds))) return rc_lds;
    dim3 grid(p->N2 / C, EXH ? kCollectRows : n_pairs * n_packed);
    (EXH ? p->dispatch.sweep_family : p->dispatch.last_family) = FFS_DISPATCH_LAST_PRUNED;
    hipLaunchKernelGGL((k_pass_c_pruned<L, C, EXH>), grid, dim3((L / 16) * C), lds, st, p->work, p->N2, (long long)p->N,
                       p->twn1, cands, first_cand, n_cand, n_packed, n_slots, p->bnom, bins, pa.noms, pa.header, pa.entries, p->log2CL,
                       p->xlist, seg, seg_shift, pa.best, pa.shares, pa.half_last);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

template <bool EXH>
int launch_pass_c_pruned(const ffs_plan* p, const CandDesc* cands, int first_cand, int n_cand, int n_packed, int n_slots,
                         int n_pairs, const BinList& bins, const PoolArgs& pa, hipStream_t st, int seg = 0, int seg_shift = 0) {
#define FFS_PCP(L, C) \
    case L: return launch_pass_c_pruned_inst<L, C, EXH>(p, cands, first_cand, n_cand, n_packed, n_slots, n_pairs, bins, pa, st, seg, seg_shift)
    switch (p->N1) {
        FFS_PCP(48, 64);
        FFS_PCP(96, 32);
        FFS_PCP(192, 16);
        FFS_PCP(384, 16);
        FFS_PCP(768, 16);
        FFS_PCP(16, 256);
        FFS_PCP(32, 128);
        FFS_PCP(64, 64);
        FFS_PCP(128, 32);
        FFS_PCP(256, 16);
        FFS_PCP(512, 16);
        FFS_PCP(1024, 16);
        FFS_PCP(2048, 8);
        FFS_PCP(4096, 4);
    }
#undef FFS_PCP
    return fail(FFS_E_INVALID, "unsupported column length %d", p->N1);
}

// Output bins m2 = m / N2 of the last pass that the lag window [d_lo, d_hi] of a candidate touches
// (m = d for d >= 0, m = d + N for d < 0), as signed offsets in (-N1/2, N1/2].
void add_bins(const ffs_plan* p, const CandDesc& cd, std::vector<int>* bins, bool* overflow) {
    if (cd.flags & CAND_NO_LAGS) return;
    auto add_range = [&](int64_t m_lo, int64_t m_hi) {
        for (int64_t m2 = m_lo / p->N2; m2 <= m_hi / p->N2; ++m2) {
            int b = (int)m2;
            if (b > p->N1 / 2) b -= p->N1;
            bool seen = false;
            for (int x : *bins) seen |= (x == b);
            if (!seen) {
                if ((int)bins->size() >= MAXBINS) {
                    *overflow = true;
                    return;
                }
                bins->push_back(b);
            }
        }
    };
    if (cd.d_hi >= 0) add_range(cd.d_lo > 0 ? cd.d_lo : 0, cd.d_hi);
    if (!*overflow && cd.d_lo < 0) add_range(p->N + cd.d_lo, p->N + (cd.d_hi < -1 ? cd.d_hi : -1));
}

// Python slice semantics of  x[:stop] = v  /  x[start:] = v  on a length-n array
int64_t py_clamp(int64_t i, int64_t n) {
    if (i < 0) i += n;
    if (i < 0) i = 0;
    if (i > n) i = n;
    return i;
}

double mapped(double x) { return 2.0 * x - 1.0; }  // aligners.py:55-57

struct VecView {
    const void* ptr;
    int64_t len;
    double lo, hi;
    int64_t lead = 0;  // positions [0, lead) of the transform input are zero padding (see XformDesc)
    int64_t off = 0;   // bit-packed vectors: bit index of sample 0 relative to ptr (see XformDesc)
};

// The reference's lag window for (R, S): allowed k in [kA, kB) of its length-n_ref convolve array
// (aligners.py:31-43), returned as inclusive lags [d_lo, d_hi] (d = n_ref-1-S-k); false if empty.
bool lag_window(int64_t R, int64_t S, int64_t n_ref, int64_t max_off, int64_t* d_lo, int64_t* d_hi) {
    int64_t kA = 0, kB = n_ref;
    if (max_off >= 0) {
        kA = py_clamp(n_ref - 1 - max_off - S, n_ref);
        kB = py_clamp(n_ref - 1 + max_off - S, n_ref);
    }
    if (kA >= kB) return false;
    *d_hi = n_ref - 1 - S - kA;
    *d_lo = n_ref - S - kB;
    return true;
}

// What the transform pipeline has to evaluate of that window: only lags with a non-empty overlap,
// d in (-S, R).  Every other lag of the window has c(d) = 0 exactly and is represented by the single
// virtual nominee (0, d_zero) -- d_zero = the largest such lag, i.e. the first such k (see CAND_HAS_ZERO
// in ffs_kernels.h).  Returns false when the reference's window is empty (everything -inf);
// *d_lo > *d_hi when the window holds only zero-overlap lags.
bool overlap_window(int64_t R, int64_t S, int64_t n_ref, int64_t max_off, int64_t* d_lo, int64_t* d_hi, bool* has_zero,
                    int64_t* d_zero) {
    int64_t wl = 0, wh = -1;
    *has_zero = false;
    *d_zero = 0;
    if (!lag_window(R, S, n_ref, max_off, &wl, &wh)) return false;
    if (wh >= R) {
        *has_zero = true;
        *d_zero = wh;
    } else if (wl <= -S) {
        *has_zero = true;
        *d_zero = -S;
    }
    *d_lo = wl > -S + 1 ? wl : -S + 1;
    *d_hi = wh < R - 1 ? wh : R - 1;
    return true;
}

// Samples that can meet the other vector at some lag of the window: s[i] is multiplied by r[i+d], which
// is zero padding unless i + d < R, so only i < R - d_lo of the candidate and j < S + d_hi of the
// reference ever contribute.  The transforms read just these prefixes.
void effective_lengths(int64_t R, int64_t S, int64_t d_lo, int64_t d_hi, int64_t* s_eff, int64_t* r_eff) {
    int64_t se = R - d_lo < S ? R - d_lo : S;
    int64_t re = S + d_hi < R ? S + d_hi : R;
    *s_eff = se < 1 ? 1 : se;
    *r_eff = re < 1 ? 1 : re;
}

int64_t next_pow2(int64_t x) {
    int64_t n = 2;
    while (n < x) n <<= 1;
    return n;
}

// Transform length a (R, S) pair needs under its lag window [d_lo, d_hi] (ffs_plan_length without the window arithmetic
// the caller has already done, and without reading the environment).
int64_t plan_length_core(int64_t R, int64_t S, int64_t n_ref, int64_t d_lo, int64_t d_hi, bool radix3_off) {
    int64_t s_eff, r_eff;
    effective_lengths(R, S, d_lo, d_hi, &s_eff, &r_eff);
    int64_t need = s_eff + d_hi + 1;
    if (r_eff - d_lo + 1 > need) need = r_eff - d_lo + 1;
    if (s_eff > need) need = s_eff;
    if (r_eff > need) need = r_eff;
    int64_t n = next_pow2(need);
    if (!radix3_off && n / 4 * 3 >= need && radix3_length(n / 4 * 3)) n = n / 4 * 3;
    return n < n_ref ? n : n_ref;
}

// Fill the candidate descriptor for (ref, sub); returns a negative code on error -- including FFS_E_TOO_LONG when the
// plan's transform length cannot hold the pair, on EVERY path (the run-boundary kernels would not need the transform,
// but whether a call is accepted must not depend on how dense its vectors are).  The fp32 tie margin, which only the
// transform path needs, is added by finish_cand_for_transforms.
int fill_cand(const ffs_plan* p, const VecView& ref, const VecView& sub, int64_t max_off, CandDesc* cd, int ref_dt, int cand_dt) {
    const int64_t R = ref.len, S = sub.len;
    if (R <= 0 || S <= 0)
        return fail(FFS_E_EMPTY, "cannot align empty speech data (reference length=%lld, subtitle length=%lld)",
                    (long long)R, (long long)S);
    const int64_t n_ref = ffs_fft_length(R, S);
    memset(cd, 0, sizeof *cd);
    cd->s = sub.ptr;
    cd->r = ref.ptr;
    cd->S = (int32_t)S;
    cd->R = (int32_t)R;
    cd->n_ref = (int32_t)n_ref;
    int64_t d_lo = 0, d_hi = -1, d_zero = 0;
    bool has_zero = false;
    if (!overlap_window(R, S, n_ref, max_off, &d_lo, &d_hi, &has_zero, &d_zero) || d_lo > d_hi) {
        cd->flags = CAND_NO_LAGS;
        cd->d_lo = 0;
        cd->d_hi = -1;
    } else {
        cd->d_lo = (int32_t)d_lo;
        cd->d_hi = (int32_t)d_hi;
        if (!p->direct_only) {
            const int64_t n_need = plan_length_core(R, S, n_ref, d_lo, d_hi, p->radix3_off);
            if (n_need > p->N)
                return fail(FFS_E_TOO_LONG, "R=%lld S=%lld needs transform length %lld > plan length %lld", (long long)R,
                            (long long)S, (long long)n_need, (long long)p->N);
        }
    }
    if (has_zero) {
        cd->flags |= CAND_HAS_ZERO;
        cd->d_zero = (int32_t)d_zero;
    }
    cd->flags |= (cand_dt << CAND_DTS_SHIFT) | (ref_dt << CAND_DTR_SHIFT);
    cd->s0 = mapped(sub.lo);
    cd->s1 = mapped(sub.hi);
    cd->r0 = mapped(ref.lo);
    cd->r1 = mapped(ref.hi);
    return FFS_OK;
}

int finish_cand_for_transforms(const ffs_plan* p, int64_t max_off, CandDesc* cd) {
    (void)max_off;
    const int64_t R = cd->R, S = cd->S;
    const double as = fmax(fabs(cd->s0), fabs(cd->s1)), ar = fmax(fabs(cd->r0), fabs(cd->r1));
    const double lg = (double)ilog2(p->N > 2 ? p->N : 2);
    // measured max fp32 error of the pipeline: ~0.02 (activity density 0.5) to ~0.2 (density 0.2) of
    // eps*log2(N)*sqrt(S*R)*|s||r| for N = 2^12..2^24; lags within 1.0x of it are nominated, and the
    // kernels widen this to 24 ulp of the maximum for DC-heavy signals (eff_margin)
    cd->margin = (float)(1.0 * 5.9604645e-08 * lg * sqrt((double)S * (double)R) * as * ar);
    return FFS_OK;
}

void fill_xform(XformDesc* x, const VecView* a, const VecView* b, const void* safe = nullptr) {
    memset(x, 0, sizeof *x);
    x->a = a->ptr;
    x->len_a = (int32_t)a->len;
    x->lead_a = (int32_t)a->lead;
    x->off_a = (int32_t)a->off;
    x->a0 = (float)mapped(a->lo);
    x->a1 = (float)mapped(a->hi);
    x->b = safe ? safe : a->ptr;  // absent second candidate: any valid address with length 0 (reads are clamped)
    if (b) {
        x->b = b->ptr;
        x->len_b = (int32_t)b->len;
        x->lead_b = (int32_t)b->lead;
        x->off_b = (int32_t)b->off;
        x->b0 = (float)mapped(b->lo);
        x->b1 = (float)mapped(b->hi);
    }
}

}  // namespace

extern "C" {

const char* ffs_last_error(void) { return g_err.c_str(); }
int ffs_version(void) { return 400; }

int64_t ffs_fft_length(int64_t ref_len, int64_t sub_len) {
    if (ref_len <= 0 || sub_len <= 0) return 0;
    // Between powers of two the reference's float expression (below) and the integer ceil(log2) agree -- log2 of
    // 2^k +- 1 differs from k by more than 1e-7 relative up to 2^24, a thousand times the rounding error of the quotient --
    // so only exact powers of two (where log(x)/log(2) can land a hair above the integer) take the float path.
    const int64_t x = ref_len + sub_len;
    if ((x & (x - 1)) != 0 && x < (int64_t(1) << 40)) return int64_t(1) << (64 - __builtin_clzll((unsigned long long)x));
    // aligners.py:67-68: int(2 ** math.ceil(math.log(R + S, 2))) -- math.log(x, 2) is
    // log(x)/log(2) in doubles, which is not exact at every power of two; keep the same quirk.
    const double bits = log((double)(ref_len + sub_len)) / log(2.0);
    return (int64_t)pow(2.0, ceil(bits));
}

int64_t ffs_plan_length(int64_t ref_len, int64_t sub_len, int64_t max_offset_samples) {
    const int64_t n_ref = ffs_fft_length(ref_len, sub_len);
    if (n_ref == 0) return n_ref;
    int64_t d_lo, d_hi, d_zero;
    bool has_zero;
    if (!overlap_window(ref_len, sub_len, n_ref, max_offset_samples, &d_lo, &d_hi, &has_zero, &d_zero) || d_lo > d_hi)
        return 2;  // nothing to evaluate
    // lags d in [d_lo, d_hi] of a length-n circular correlation equal the linear ones iff no product
    // wraps: S' + d_hi <= n and R' - d_lo <= n for the prefixes (S', R') that reach the window at all
    int64_t s_eff, r_eff;
    effective_lengths(ref_len, sub_len, d_lo, d_hi, &s_eff, &r_eff);
    int64_t need = s_eff + d_hi + 1;
    if (r_eff - d_lo + 1 > need) need = r_eff - d_lo + 1;
    if (s_eff > need) need = s_eff;
    if (r_eff > need) need = r_eff;
    int64_t n = next_pow2(need);
    // three quarters of that is enough for many inputs (a 2 h pair at 100 Hz needs 726 001 points:
    // 3 * 2^18 = 786 432 instead of 2^20), and the column passes handle one factor of three
    const char* e = getenv("FFS_DISABLE_RADIX3");  // (read per call: only the transform path asks for plan lengths)
    if (!(e && e[0] == '1') && n / 4 * 3 >= need && radix3_length(n / 4 * 3)) n = n / 4 * 3;
    return n < n_ref ? n : n_ref;
}

int ffs_plan_create(int device, int64_t n_fft, int pairs_in_flight, int max_cand, ffs_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "out is null");
    *out = nullptr;
    const bool r3 = radix3_length(n_fft);
    if (n_fft < 2 || n_fft > kMaxFftN || ((n_fft & (n_fft - 1)) && !r3))
        return fail(FFS_E_INVALID, "n_fft must be a power of two in [2, 2^24] or 3*2^k in [12288, 3145728], got %lld",
                    (long long)n_fft);
    if (pairs_in_flight < 1 || max_cand < 1) return fail(FFS_E_INVALID, "pairs_in_flight and max_cand must be >= 1");
    HIP_TRY(hipSetDevice(device));
    ffs_plan* p = new ffs_plan();
    struct Guard {  // destroy the half-built plan on any early return
        ffs_plan* p;
        ~Guard() {
            if (p) ffs_plan_destroy(p);
        }
    } guard{p};
    p->device = device;
    {
        const char* e3 = getenv("FFS_DISABLE_RADIX3");
        p->radix3_off = e3 && e3[0] == '1';
    }
    p->N = n_fft;
    p->pairs_in_flight = pairs_in_flight;
    p->max_cand = max_cand;
    p->max_slots = 1 + (max_cand + 1) / 2;
    HIP_TRY(hipEventCreateWithFlags(&p->upload_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->last_done, hipEventDisableTiming));
    for (int h = 0; h < 2; ++h) HIP_TRY(hipEventCreateWithFlags(&p->half_done[h], hipEventDisableTiming));
    {
        // Run-time knobs: five, all listed in INTEGRATION.md section 6, each selecting between code paths that
        // return identical records (every pairing has an "identical records" GPU test).
        auto on = [](const char* name) {
            const char* e = getenv(name);
            return e && e[0] == '1';
        };
        p->allow_pruned = !on("FFS_DISABLE_PRUNED_PASS_C");
        p->allow_seg = !on("FFS_DISABLE_SEGMENTED");
        p->allow_half_last = !on("FFS_DISABLE_HALF_LAST");
        if (const char* ea = getenv("FFS_ALGORITHM")) {  // auto (default) | fft | runs
            if (!strcmp(ea, "fft")) p->algo = FFS_ALGO_FFT;
            else if (!strcmp(ea, "runs")) p->algo = FFS_ALGO_RUNS;
        }
        // Measured break-even (profiles/r04_runs_experiments.json, `boundary_density` / `windowless` in the bench line):
        // k_runs_corr spends 1.2-1.6e-4 us*CU per boundary coincidence, the transform pipeline 6-9e-4 us*CU per point of
        // the plan length and packed transform slot -> eight coincidences per transform point and slot; a candidate's
        // share of the slots is (n_cand + 1) / (2 n_cand) (two candidates per complex transform + the reference's half
        // slot): 3.6 M for seven candidates on the window-shortened 2 h plan, 7.2 M on the windowless one.  Either path is
        // within ~10 % of the other around the threshold.  FFS_RUNS_BUDGET=<coincidences> overrides it.
        p->runs_budget = -1;
        if (const char* eb = getenv("FFS_RUNS_BUDGET")) p->runs_budget = atoll(eb);
        if (const char* es = getenv("FFS_RUNS_SPLIT")) p->runs_split = atoi(es);
        p->runs_stride = kRunsStride0;
        if (const char* es = getenv("FFS_RUNS_STRIDE")) {
            const int v = atoi(es);
            p->runs_stride = v < 64 ? 64 : (v > RUNS_CAP ? RUNS_CAP : v);
        }
        if (const char* et = getenv("FFS_HOST_TIMING")) p->host_timing = et[0] == '1';
        const char* e3 = getenv("FFS_PASS_A_PREFETCH");
        if (e3) p->pass_a_prefetch = p->pass_a_prefetch_bits = atoi(e3);
#ifdef FFS_LAB
        // section experiments of the lab build (timing only: these switches produce WRONG RESULTS)
        const char* e20 = getenv("FFS_PASS_A_DEBUG");
        if (e20) p->lab_flags |= (atoi(e20) & 31) << 10;
        const char* e15 = getenv("FFS_MID_DEBUG");
        if (e15) p->lab_flags |= ((atoi(e15) & 1) ? DBG_NO_FFT : 0) | ((atoi(e15) & 2) ? DBG_HOT_MEM : 0) | ((atoi(e15) & 4) ? DBG_NO_STORE : 0);
#endif
    }
    if (n_fft < kMinFftN) {
        p->direct_only = true;
        guard.p = nullptr;
        *out = p;
        return FFS_OK;
    }
    if (r3) {
        p->N2 = n_fft >= 48 * 4096 ? 4096 : (int)(n_fft / 48);
        p->N1 = (int)(n_fft / p->N2);
    } else {
        const int lg = ilog2(n_fft);
        const int lg2 = lg - 4 < 12 ? lg - 4 : 12;
        p->N2 = 1 << lg2;
        p->N1 = (int)(n_fft >> lg2);
    }
    p->C = tile_cols(p->N1);
    p->log2C = ilog2(p->C);
    p->log2CL = p->log2C < 6 ? 6 : p->log2C;
    if ((1 << p->log2CL) > p->N2) p->log2CL = ilog2(p->N2);
#ifdef FFS_LAB
    if (const char* ecl = getenv("FFS_LOG2CL")) {  // wider row chunks (timing experiments of the lab build)
        const int v = atoi(ecl);
        if (v >= p->log2C && (1 << v) <= p->N2 / 16) p->log2CL = v;
    }
#endif
    const int64_t N = n_fft;
    const int N1 = p->N1, N2 = p->N2, LT1 = N1 / 16, LT2 = N2 / 16;
    int rc;
    const int LI1 = r3 ? N1 / 3 : N1;  // power-of-two part of the column length
    if ((rc = upload(&p->tw1, make_stage_tables(LI1), &p->workspace_bytes))) return rc;
    if ((rc = upload(&p->tw2, make_stage_tables(N2), &p->workspace_bytes))) return rc;
    if (N1 == 512 && (rc = upload(&p->tw1h, make_stage_tables(256), &p->workspace_bytes))) return rc;  // sub-transforms of k_pass_a3/c3<2, 256>
    {
        // Power-of-two columns: thread u holds the outputs k1 = u + LT1*q.  3*2^k columns (k_pass_a's
        // radix-3 branch): store thread rg = r*KG + kg holds k1 = kg + LI*r + KG*j, KG = 2*(LI/16).
        const int KG = 2 * (LI1 / 16);
        const int nb = r3 ? 3 * KG : LT1, ostep = r3 ? KG : LT1;
        std::vector<cf> tb((size_t)nb * N2), ts((size_t)16 * N2);
        for (int u = 0; u < nb; ++u) {
            const int ob = r3 ? (u % KG) + LI1 * (u / KG) : u;
            for (int n2 = 0; n2 < N2; ++n2) tb[(size_t)u * N2 + n2] = wn(N, (int64_t)n2 * ob);
        }
        for (int q = 0; q < 16; ++q)
            for (int n2 = 0; n2 < N2; ++n2) ts[(size_t)q * N2 + n2] = wn(N, (int64_t)n2 * ostep * q);
        if ((rc = upload(&p->tbA, tb, &p->workspace_bytes))) return rc;
        if ((rc = upload(&p->tsA, ts, &p->workspace_bytes))) return rc;
    }
    {
        std::vector<cf> tb((size_t)N1 * LT2), ts((size_t)N1 * 16);
        for (int k1 = 0; k1 < N1; ++k1) {
            for (int u = 0; u < LT2; ++u) tb[(size_t)k1 * LT2 + u] = wn(N, (int64_t)k1 * u);
            for (int q = 0; q < 16; ++q) ts[(size_t)k1 * 16 + q] = wn(N, (int64_t)k1 * LT2 * q);
        }
        if ((rc = upload(&p->tbM, tb, &p->workspace_bytes))) return rc;
        if ((rc = upload(&p->tsM, ts, &p->workspace_bytes))) return rc;
    }
    if ((r3 && LI1 >= 64) || N1 == 512) {  // k_pass_a3: k1 = u + LTI*q + LI*r (three sub-transforms; two for N1 = 512)
        const int LIr = r3 ? LI1 : 256;
        const int LTI = LIr / 16;
        std::vector<cf> tb((size_t)LTI * N2), ts((size_t)4 * N2), th((size_t)2 * N2);
        for (int n2 = 0; n2 < N2; ++n2) {
            for (int u = 0; u < LTI; ++u) tb[(size_t)u * N2 + n2] = wn(N, (int64_t)n2 * u);
            for (int i = 0; i < 4; ++i) ts[(size_t)i * N2 + n2] = wn(N, (int64_t)n2 * LTI * (1 << i));
            for (int r = 1; r <= 2; ++r) th[(size_t)(r - 1) * N2 + n2] = wn(N, (int64_t)n2 * LIr * r);
        }
        if ((rc = upload(&p->tbR, tb, &p->workspace_bytes))) return rc;
        if ((rc = upload(&p->tsR, ts, &p->workspace_bytes))) return rc;
        if ((rc = upload(&p->thR, th, &p->workspace_bytes))) return rc;
    }
    {
        std::vector<cf> t((size_t)N1);
        for (int k = 0; k < N1; ++k) t[k] = wn(N1, k);
        if ((rc = upload(&p->twn1, t, &p->workspace_bytes))) return rc;
    }
    // The transform workspace ([pairs_in_flight][max_slots][N] complex fp32 -- 15 GiB for 512 seven-ratio 2 h pairs --,
    // block-nominee records, the overflow pool) is allocated by the first call that runs the transforms
    // (ensure_workspace): calls served by the run-boundary path never touch it.  workspace_bytes counts it from the start.
    p->workspace_bytes += (int64_t)((size_t)pairs_in_flight * p->max_slots * N * sizeof(cf));
    p->workspace_bytes += (int64_t)((size_t)pairs_in_flight * (p->max_slots - 1) * 2 * (N2 / p->C) * sizeof(BlockNom));
    p->workspace_bytes += (int64_t)kPoolCapacity * sizeof(PoolEntry);
    if (r3 && p->allow_seg && p->N2 == 4096 && n_fft / 3 >= 65536) {
        if ((rc = ffs_plan_create(device, n_fft / 3, pairs_in_flight * kSegBlocks, max_cand, &p->seg))) return rc;
        p->workspace_bytes += p->seg->workspace_bytes;
    }
    guard.p = nullptr;
    *out = p;
    return FFS_OK;
}

int ffs_plan_destroy(ffs_plan* p) {
    if (!p) return FFS_OK;
    if (p->host_timing && p->runs_calls)
        fprintf(stderr, "[ffs host timing] %lld run-boundary calls: total %.1f us/call = vectors+extract launch %.1f, candidate "
                "descriptors %.1f, wait for list lengths %.1f, decision+rest %.1f\n", (long long)p->runs_calls,
                p->ht_total / p->runs_calls / 1e3, p->ht_vec / p->runs_calls / 1e3, p->ht_cand / p->runs_calls / 1e3,
                p->ht_wait / p->runs_calls / 1e3, p->ht_decide / p->runs_calls / 1e3);
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->tw1);
    (void)hipFree(p->tw2);
    (void)hipFree(p->tbA);
    (void)hipFree(p->tsA);
    (void)hipFree(p->tw1h);
    (void)hipFree(p->tbR);
    (void)hipFree(p->tsR);
    (void)hipFree(p->thR);
    (void)hipFree(p->tbM);
    (void)hipFree(p->tsM);
    (void)hipFree(p->twn1);
    (void)hipFree(p->work);
    (void)hipFree(p->bnom);
    (void)hipFree(p->pool_entries);
    (void)hipFree(p->xlist);
    if (p->seg) (void)ffs_plan_destroy(p->seg);
    (void)hipFree(p->runs_e);
    (void)hipFree(p->runs_n);
    (void)hipFree(p->runs_best);
    (void)hipFree(p->runs_flags);
    (void)hipFree(p->runs_zero_flags);
    (void)hipFree(p->pack_buf);
    (void)hipFree(p->lvl_buf);
    if (p->runs_flags_host) (void)hipHostFree(p->runs_flags_host);
    if (p->runs_ev) (void)hipEventDestroy(p->runs_ev);
    if (p->upload_done) (void)hipEventSynchronize(p->upload_done);  // (the shared copy stream may still be reading the pinned block)
    if (p->copy_ev) (void)hipEventDestroy(p->copy_ev);
    for (int h = 0; h < 2; ++h)
        if (p->half_done[h]) (void)hipEventDestroy(p->half_done[h]);
    (void)hipFree(p->dev_desc);
    (void)hipFree(p->dev_desc2);
    if (p->host_desc) (void)hipHostFree(p->host_desc);
    if (p->upload_done) (void)hipEventDestroy(p->upload_done);
    if (p->last_done) (void)hipEventDestroy(p->last_done);
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    delete p;
    return FFS_OK;
}

int64_t ffs_plan_workspace_bytes(const ffs_plan* p) { return p ? p->workspace_bytes : 0; }

}  // extern "C"

// ---- the main solve (ffs_align_batch*) -----------------------------------------------------------------------------
namespace {

// One call as the entry points hand it over.  `dtype` = the candidates' element type, `ref_dt` = the references';
// vec_bound (may be null): FFS_DTYPE_RUNS vectors only -- a host-known upper bound of the list's length (0: unknown).
struct AlignArgs {
    int n_pairs, n_cand, ref_dt, dtype;
    const void* const* vec_ptr;
    const int64_t* vec_len;
    const double *vec_lo, *vec_hi;
    const int32_t* vec_bound;
    int64_t max_offset_samples, filter_max_offset;
    ffs_cand_result* cand_out_dev;
    ffs_pair_result* pair_out_dev;
    void* hip_stream;
};

bool runs_able(int dt) { return dt == FFS_DTYPE_U1 || dt == FFS_DTYPE_RUNS; }
int as_bits(int dt) { return dt == FFS_DTYPE_RUNS ? FFS_DTYPE_U1 : dt; }  // list-only vectors reach the transforms as bits
size_t esz_of(int dt) { return dt == FFS_DTYPE_U8 ? 1 : (dt == FFS_DTYPE_F32 ? 4 : (dt == FFS_DTYPE_F64 ? 8 : 0)); }
double now_ns() {
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One contract for every path, checked before anything is queued: no empty vector (aligners.py:58-66), no null or
// misaligned pointer, no vector of 2^30 samples or more (positions are 32-bit; 0x3fffffff is the run-boundary kernels'
// "beyond everything").  The plan-length check (FFS_E_TOO_LONG whichever path would have served the pair) is part of
// fill_cand, which every path runs for every candidate.
int check_align_args(const ffs_plan* p, const AlignArgs& a) {
    auto known = [](int dt) {
        return dt == FFS_DTYPE_U8 || dt == FFS_DTYPE_F32 || dt == FFS_DTYPE_U1 || dt == FFS_DTYPE_F64 || dt == FFS_DTYPE_RUNS;
    };
    auto amask_of = [](int dt) -> uintptr_t { return dt == FFS_DTYPE_U8 ? 0 : (dt == FFS_DTYPE_F64 || dt == FFS_DTYPE_RUNS ? 7 : 3); };
    if (!p) return fail(FFS_E_INVALID, "plan is null");
    if (a.n_pairs < 0 || a.n_cand < 1 || a.n_cand > p->max_cand)
        return fail(FFS_E_INVALID, "n_cand=%d outside [1, plan max_cand=%d]", a.n_cand, p->max_cand);
    if (!known(a.dtype) || !known(a.ref_dt)) return fail(FFS_E_INVALID, "unknown dtype %d / %d", a.ref_dt, a.dtype);
    if (!a.vec_ptr || !a.vec_len || !a.vec_lo || !a.vec_hi || !a.cand_out_dev || !a.pair_out_dev)
        return fail(FFS_E_INVALID, "null argument");
    const int stride = 1 + a.n_cand;
    for (int pi = 0; pi < a.n_pairs; ++pi) {
        const size_t b = (size_t)pi * stride;
        for (int v = 0; v < stride; ++v) {
            const int dt = v ? a.dtype : a.ref_dt;
            if (a.vec_len[b] <= 0 || a.vec_len[b + v] <= 0)
                return fail(FFS_E_EMPTY, "cannot align empty speech data (reference length=%lld, subtitle length=%lld)",
                            (long long)a.vec_len[b], (long long)a.vec_len[b + (v ? v : 1)]);
            if (!a.vec_ptr[b + v]) return fail(FFS_E_INVALID, "null device pointer for pair %d", pi);
            if ((uintptr_t)a.vec_ptr[b + v] & amask_of(dt))
                return fail(FFS_E_INVALID, "float / bit-packed vectors and boundary lists must be aligned to their element (pair %d)", pi);
            if (a.vec_len[b + v] >= (int64_t(1) << 30))
                return fail(FFS_E_TOO_LONG, "vector of %lld samples (pair %d): at most 2^30 - 1", (long long)a.vec_len[b + v], pi);
        }
    }
    return FFS_OK;
}

// Byte offsets of n bit images packed one behind the other, each starting on a 64-byte line: image i holds `planes`
// planes of len[i * step] bits when want(i), nothing otherwise.  (*off)[n] = the bytes of them all; returns the longest
// wanted length (at least 1).
template <class Pred>
int64_t bit_image_offsets(const int64_t* len, size_t n, size_t step, int planes, Pred want, std::vector<size_t>* off) {
    off->assign(n + 1, 0);
    int64_t len_max = 1;
    for (size_t i = 0; i < n; ++i) {
        const int64_t l = len[i * step];
        (*off)[i + 1] = (*off)[i] + (want(i) ? ((planes * ((size_t)(l + 31) / 32) * 4 + 63) & ~(size_t)63) : 0);
        if (want(i) && l > len_max) len_max = l;
    }
    return len_max;
}

// A plan-owned device buffer that only ever grows (pack_buf, lvl_buf): the previous call may still be reading the old one.
template <class T>
int grow_device_buf(ffs_plan* p, T** buf, size_t* bytes, size_t need) {
    if (need <= *bytes) return FFS_OK;
    if (p->has_last) HIP_TRY(hipEventSynchronize(p->last_done));
    (void)hipFree(*buf);
    *buf = nullptr;
    *bytes = 0;
    HIP_TRY(hipMalloc((void**)buf, need + need / 4));
    *bytes = need + need / 4;
    return FFS_OK;
}

// 0/1 BYTES (the north star's literal input format): one pass packs every vector of the call to bits (bit = byte != 0,
// exactly the two-level reading the byte kernels apply), then the call continues as FFS_DTYPE_U1 -- run-boundary path
// where the lists are short, transforms on an eighth of the input bytes otherwise.  Identical records
// (tests/test_gpu_headline.py::test_byte_inputs_give_the_same_records; FFS_ALGO_FFT keeps the byte kernels).
// Rewrites `a` to read the packed images (`packed` owns its pointer table).  A stream entry of its own: the solve enters again.
int pack_byte_vectors(ffs_plan* p, AlignArgs* a, std::vector<const void*>* packed) {
    hipStream_t st = (hipStream_t)a->hip_stream;
    const size_t n_vec = (size_t)a->n_pairs * (size_t)(1 + a->n_cand);
    std::vector<size_t> off;
    const int64_t len_max = bit_image_offsets(a->vec_len, n_vec, 1, 1, [](size_t) { return true; }, &off);
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if ((rc = enter_stream(p, st))) return rc;
    if ((rc = grow_device_buf(p, &p->pack_buf, &p->pack_bytes, off[n_vec]))) return rc;
    if ((rc = ensure_desc(p, n_vec * sizeof(PackVec) + 4096))) return rc;
    HIP_TRY(hipEventSynchronize(p->upload_done));
    p->cur_half = 0;
    PackVec* hp = (PackVec*)p->host_desc;
    packed->resize(n_vec);
    for (size_t i = 0; i < n_vec; ++i) {
        unsigned* dst = (unsigned*)((char*)p->pack_buf + off[i]);
        hp[i] = PackVec{(const unsigned char*)a->vec_ptr[i], dst, (int32_t)a->vec_len[i], 0};
        (*packed)[i] = dst;
    }
    HIP_TRY(hipMemcpyAsync(p->dev_desc, hp, n_vec * sizeof(PackVec), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->upload_done, st));
    const int chunks_per_vec = (int)(((len_max + 31) / 32 + 255) / 256);
    hipLaunchKernelGGL(k_pack_bytes_batch, dim3((unsigned)(n_vec * chunks_per_vec)), dim3(256), 0, st, (const PackVec*)p->dev_desc,
                       chunks_per_vec);
    HIP_TRY(hipGetLastError());
    if ((rc = leave_stream(p, st))) return rc;
    a->ref_dt = a->dtype = FFS_DTYPE_U1;
    a->vec_ptr = packed->data();
    a->vec_bound = nullptr;
    return FFS_OK;
}

// Expands the call's list-only vectors (role `ref`/`cand` of type FFS_DTYPE_RUNS) to bits in the plan's pack buffer;
// `out` = the call's pointer table with those vectors replaced.  Queued on `st`, inside the caller's stream entry.
int expand_list_vectors(ffs_plan* p, const AlignArgs& a, hipStream_t st, std::vector<const void*>* out) {
    const size_t stride = 1 + (size_t)a.n_cand, n_vec = (size_t)a.n_pairs * stride;
    auto is_list = [&](size_t i) { return ((i % stride) ? a.dtype : a.ref_dt) == FFS_DTYPE_RUNS; };
    std::vector<size_t> off;
    const int64_t len_max = bit_image_offsets(a.vec_len, n_vec, 1, 1, is_list, &off);
    int rc;
    if ((rc = grow_device_buf(p, &p->pack_buf, &p->pack_bytes, off[n_vec]))) return rc;
    ExpandVec* d_ev = nullptr;
    std::vector<ExpandVec> hev(n_vec);
    out->assign(a.vec_ptr, a.vec_ptr + n_vec);
    for (size_t i = 0; i < n_vec; ++i) {
        unsigned* dst = is_list(i) ? (unsigned*)((char*)p->pack_buf + off[i]) : nullptr;
        hev[i] = ExpandVec{(const int2*)((const char*)a.vec_ptr[i] + 16), (const int2*)a.vec_ptr[i], dst, (int32_t)a.vec_len[i], 0};
        if (dst) (*out)[i] = dst;
    }
    // (rare path; the table is followed by one int the kernel raises when a block's header does not fit the block)
    const size_t tab = n_vec * sizeof(ExpandVec);
    int bad_list = 0;
    HIP_TRY(hipMallocAsync((void**)&d_ev, tab + sizeof(int), st));
    hipError_t he = hipMemcpyAsync(d_ev, hev.data(), tab, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemsetAsync((char*)d_ev + tab, 0, sizeof(int), st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess) {
        const int chunks_per_vec = (int)(((len_max + 31) / 32 + 255) / 256);
        hipLaunchKernelGGL(k_runs_expand, dim3((unsigned)(n_vec * chunks_per_vec)), dim3(256), 0, st, (const ExpandVec*)d_ev, chunks_per_vec,
                           (int*)((char*)d_ev + tab));
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(&bad_list, (char*)d_ev + tab, sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    const hipError_t hf = hipFreeAsync(d_ev, st);  // (on every path: an error above must not leak the table)
    HIP_TRY(he);
    HIP_TRY(hf);
    if (bad_list)
        return fail(FFS_E_INVALID, "a boundary list of the call is truncated (more entries than its block holds) or was made for "
                    "another vector length: nothing can solve it -- pass the vector as bits");
    return FFS_OK;
}

// Boundary lists where only the transforms (or the direct kernel of short plans) may run: the call continues on bits.
// A stream entry of its own, like pack_byte_vectors.
int lists_to_bits(ffs_plan* p, AlignArgs* a, std::vector<const void*>* bits_ptr) {
    hipStream_t st = (hipStream_t)a->hip_stream;
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if ((rc = enter_stream(p, st))) return rc;
    if ((rc = expand_list_vectors(p, *a, st, bits_ptr))) return rc;
    if ((rc = leave_stream(p, st))) return rc;
    a->ref_dt = as_bits(a->ref_dt);
    a->dtype = as_bits(a->dtype);
    a->vec_ptr = bits_ptr->data();
    a->vec_bound = nullptr;
    return FFS_OK;
}

// The descriptor block of one solve, the same in the pinned host block and in either device block:
// [PoolHeader][CandDesc n_cands][RunsRef n_rr][multi-level tables][XformDesc n_xf][NomList n_cands][RescoreAcc n_cands*KNOM]
// [PoolBest n_cands].  Everything up to the transform descriptors is written by the host and uploaded; the rest lives on
// the device only.
struct DescLayout {
    size_t n_pairs = 0, n_cands = 0, n_rr = 0;
    size_t o_pool = 0;   // PoolHeader (uploaded: count = 0, capacity)
    size_t o_cand = 64;
    size_t o_rv = 0;     // RunsRef[n_rr] when runs_ok
    // multi-level tables behind it: LevelInfo | sample pointers | plane pointers | lengths | plane words, one per pair
    size_t o_li = 0, o_mp = 0, o_mq = 0, o_ml = 0, o_mw = 0;
    size_t o_xf = 0, o_nom = 0, o_acc = 0, o_pbest = 0, total = 0;

    DescLayout() = default;
    DescLayout(size_t n_pairs_, size_t n_cand, size_t n_rr_, bool ml_on, bool runs_ok, size_t n_xf_alloc)
        : n_pairs(n_pairs_), n_cands(n_pairs_ * n_cand), n_rr(n_rr_) {
        const size_t ml_pairs = ml_on ? n_pairs : 0;
        o_rv = o_cand + n_cands * sizeof(CandDesc);
        o_li = (o_rv + (runs_ok ? n_rr * sizeof(RunsRef) : 0) + 63) & ~(size_t)63;
        o_mp = o_li + ml_pairs * sizeof(LevelInfo);
        o_mq = o_mp + ml_pairs * 8;
        o_ml = o_mq + ml_pairs * 8;
        o_mw = o_ml + ml_pairs * 4;
        o_xf = (o_mw + ml_pairs * 4 + 63) & ~(size_t)63;
        o_nom = (o_xf + n_xf_alloc * sizeof(XformDesc) + 255) & ~(size_t)255;
        o_acc = o_nom + n_cands * sizeof(NomList);
        o_pbest = o_acc + n_cands * KNOM * sizeof(RescoreAcc);  // zeroed together with acc
        total = o_pbest + n_cands * sizeof(PoolBest);
    }
    PoolHeader* pool(char* b) const { return (PoolHeader*)(b + o_pool); }
    CandDesc* cands(char* b) const { return (CandDesc*)(b + o_cand); }
    RunsRef* runs_refs(char* b) const { return (RunsRef*)(b + o_rv); }
    LevelInfo* level_info(char* b) const { return (LevelInfo*)(b + o_li); }
    const void** level_samples(char* b) const { return (const void**)(b + o_mp); }
    unsigned** level_planes(char* b) const { return (unsigned**)(b + o_mq); }
    int32_t* level_lens(char* b) const { return (int32_t*)(b + o_ml); }
    int32_t* level_words(char* b) const { return (int32_t*)(b + o_mw); }
    XformDesc* xforms(char* b) const { return (XformDesc*)(b + o_xf); }
    NomList* nominees(char* b) const { return (NomList*)(b + o_nom); }
    RescoreAcc* acc(char* b) const { return (RescoreAcc*)(b + o_acc); }
    PoolBest* pool_best(char* b) const { return (PoolBest*)(b + o_pbest); }
    // the byte ranges that go up (offset, bytes)
    size_t table_at() const { return o_rv; }
    size_t table_bytes(size_t n_refs) const { return n_refs * sizeof(RunsRef); }  // the first n_refs of the vector table
    size_t level_tables_bytes() const { return o_xf - o_rv; }                      // the vector table and the multi-level tables
    size_t head_bytes(size_t n_refs) const { return o_rv + n_refs * sizeof(RunsRef); }  // from 0: header, candidates (+ table)
    size_t transform_bytes(size_t n_xf) const { return o_xf + n_xf * sizeof(XformDesc); }  // from 0: all the host writes
    size_t refresh_at() const { return o_cand; }
    size_t refresh_bytes(size_t n_xf) const { return transform_bytes(n_xf) - o_cand; }  // candidates .. transform descriptors
    size_t acc_bytes(size_t n) const { return n * KNOM * sizeof(RescoreAcc); }
    size_t acc_and_best_bytes() const { return acc_bytes(n_cands) + n_cands * sizeof(PoolBest); }
};

// Leaves the plan's bookkeeping consistent on every exit of a solve once work has been queued: an error return after a
// kernel launch must still record the call's last event (the next call on another stream waits for it), and one after a
// copy from the pinned block must leave upload_done behind that copy (the next call waits for it before it writes the block).
struct StreamLeave {
    ffs_plan* p;
    hipStream_t st;
    bool armed = false;
    bool upload_open = false;  // a copy from the pinned block is queued on upload_st with no upload_done behind it yet
    hipStream_t upload_st = nullptr;
    ~StreamLeave() {
        if (upload_open) (void)hipEventRecord(p->upload_done, upload_st);
        if (armed) (void)leave_stream(p, st);
    }
};

// One solve of at most 65 536 run-boundary vectors: the call's state, with its phases as member functions in the order
// solve_call() runs them.
struct AlignCall {
    ffs_plan* const p;
    const AlignArgs& a;
    const hipStream_t st;
    StreamLeave leave;
    // shape
    const int n_pairs, n_cand, stride, n_packed, n_slots, n_chunks;
    const size_t n_vec, n_cands;
    size_t n_rr = 0;       // RunsRef entries: every vector, then three threshold planes per pair of a multi-level call
    size_t flag_bytes = 0;  // sub-batch flags + two 8-byte statistics behind them (boundaries of the call, its longest plan-owned list)
    // decided once
    bool lists_in, ml, runs_ok, need_extract, ml_on = false, mixed, use_copy = false, dense_stream = false;
    int t_dtype, t_ref_dt;  // the types the transform kernels see (list-only vectors are expanded to bits before they run)
    int hflags = 0;
    long long budget = 0;
    DescLayout L;
    char *hb = nullptr, *db = nullptr;  // the pinned block, the device block of this call
    CandDesc* hc = nullptr;
    const CandDesc* dc = nullptr;
    const RunsRef* d_rv = nullptr;
    const XformDesc* dx = nullptr;
    NomList* dn = nullptr;
    RescoreAcc* da = nullptr;
    PoolBest* dpb = nullptr;
    PoolArgs pa{};
    CandResult* cres;
    PairResult* pres;
    // changes during the call
    bool late_extract = false;   // small calls: table and extraction go behind the candidate descriptors (upload_descriptors)
    bool probe_first = false;    // a density probe stands in for the extraction so far
    bool flags_cleared = false;  // the extraction kernel's first workgroup has cleared the flags (a memset otherwise)
    bool copy_entered = false;   // the copy stream already waits for the last call that used this device block
    bool proven = false, xf_built = false, retry = false;
    int tiles_max = 1;
    int64_t lvl_len_max = 1;
    const void* const* xptr;  // the vectors as the transform path reads them (list-only vectors: their expansion)
    std::vector<const void*> expanded;
    BinList bins;
    bool pruned = false, seg = false;
    int seg_blocks = 0;
    int64_t seg_lo = 0;
    size_t n_xf;
    std::vector<char> chunk_fft;
    bool any_fft = false;
    double ht0 = 0, ht1 = 0, ht2 = 0, ht3 = 0;  // FFS_HOST_TIMING marks

    AlignCall(ffs_plan* p_, const AlignArgs& a_)
        : p(p_), a(a_), st((hipStream_t)a_.hip_stream), leave{p_, (hipStream_t)a_.hip_stream},
          n_pairs(a_.n_pairs), n_cand(a_.n_cand), stride(1 + a_.n_cand), n_packed((a_.n_cand + 1) / 2), n_slots(1 + (a_.n_cand + 1) / 2),
          n_chunks((a_.n_pairs + p_->pairs_in_flight - 1) / p_->pairs_in_flight), n_vec((size_t)a_.n_pairs * (1 + a_.n_cand)),
          n_cands((size_t)a_.n_pairs * a_.n_cand), cres((CandResult*)a_.cand_out_dev), pres((PairResult*)a_.pair_out_dev),
          xptr(a_.vec_ptr), n_xf((size_t)a_.n_pairs * (1 + (a_.n_cand + 1) / 2)) {
        memset(&bins, 0, sizeof bins);
        const bool may_run = p->algo != FFS_ALGO_FFT && !p->direct_only;
        lists_in = a.dtype == FFS_DTYPE_RUNS || a.ref_dt == FFS_DTYPE_RUNS;
        // Run-boundary path: two-level vectors on both sides, as bits (FFS_DTYPE_U1: their lists are extracted here) or as
        // boundary lists (FFS_DTYPE_RUNS); everything else, and every sub-batch whose lists turn out too long, goes through
        // the transforms.  Multi-level float references (the `weighted` fused VAD's four levels,
        // speech_transformers.py:290-293) against two-level candidates: the reference's threshold planes are made on the
        // device (k_levels_*), their lists extracted, and the run-boundary kernel adds the levels up (ffs_runs.h, LevelInfo).
        ml = may_run && (a.ref_dt == FFS_DTYPE_F64 || a.ref_dt == FFS_DTYPE_F32) && runs_able(a.dtype);
        runs_ok = may_run && runs_able(a.dtype) && (runs_able(a.ref_dt) || ml);
        need_extract = runs_ok && (ml || a.dtype == FFS_DTYPE_U1 || a.ref_dt == FFS_DTYPE_U1);
        n_rr = n_vec + (ml ? 3 * (size_t)n_pairs : 0);
        flag_bytes = (((size_t)n_chunks * sizeof(int) + 7) & ~(size_t)7) + 16;
        // `mixed` when the two roles differ in type: the first pass runs once per role (row_sel) and the exact
        // re-evaluation goes through the type-generic instantiations (DT 4)
        t_dtype = as_bits(a.dtype), t_ref_dt = as_bits(a.ref_dt);
        mixed = t_ref_dt != t_dtype;
        hflags = p->direct_only ? 0 : half_flags_of(p, ref_half_ok(p));
        budget = p->algo == FFS_ALGO_RUNS ? INT64_MAX / 4
                 : p->runs_budget >= 0    ? p->runs_budget
                                          : kRunsBudgetPerPoint * (long long)p->N * (n_cand + 1) / (2 * n_cand);
    }
    // odd candidate count: the last packed transform carries one real candidate -> half of its rows suffice
    // (needs the one-row-per-block mid kernels, like ref_half; the plan that runs the kernels decides)
    int half_flags_of(const ffs_plan* q, bool rh) const {
        const bool hl = (n_cand % 2 == 1) && q->allow_half_last && ref_half_ok(q) && q->N1 >= 4;
        return (rh ? HALF_REF : 0) | (hl ? HALF_LAST : 0);
    }
    void mark(double* t) const {
        if (p->host_timing) *t = now_ns();
    }
    VecView view(const void* const* ptrs, size_t i) const { return VecView{ptrs[i], a.vec_len[i], a.vec_lo[i], a.vec_hi[i]}; }

    // The ONE place that copies from the pinned block: [off, off + bytes) goes up on the call's stream, or on the copy
    // stream behind the last call that used this device block (the call's stream then waits for the copy).  upload_done
    // is recorded behind the copy -- except behind the vector table that goes ahead of the descriptors (`table_ahead`: they
    // follow on the same stream and record it; should the call fail before that, `leave` does).
    int upload(size_t off, size_t bytes, bool on_copy, bool table_ahead = false) {
        const hipStream_t us = on_copy ? p->copy_stream : st;
        if (on_copy && !copy_entered) {
            if (p->half_used[p->cur_half]) HIP_TRY(hipStreamWaitEvent(us, p->half_done[p->cur_half], 0));
            copy_entered = true;
        }
        HIP_TRY(hipMemcpyAsync(db + off, hb + off, bytes, hipMemcpyHostToDevice, us));
        leave.armed = true;
        leave.upload_open = true;
        leave.upload_st = us;
        const hipEvent_t ev = table_ahead ? p->copy_ev : p->upload_done;
        if (!table_ahead || on_copy) HIP_TRY(hipEventRecord(ev, us));
        if (on_copy) HIP_TRY(hipStreamWaitEvent(st, ev, 0));
        if (!table_ahead) leave.upload_open = false;
        return FFS_OK;
    }
    void launch_extraction(size_t n_refs, bool clear_flags, bool plain_lists) {
        ProfSpan span(p, st, FFS_K_RUNS_EXTRACT);
        if (plain_lists)  // the call's own vectors: candidates' lists compact (see RunsRef)
            runs_extract_launch(d_rv, n_refs, false, st, clear_flags ? p->runs_flags : nullptr, clear_flags ? (int)(flag_bytes / sizeof(int)) : 0,
                                stride, (int)n_vec);
        else  // (full lists: see runs_corr_body, p_sh)
            runs_extract_launch(d_rv, n_refs, false, st, p->runs_flags, (int)(flag_bytes / sizeof(int)));
        flags_cleared = flags_cleared || clear_flags;
    }

    // ---- phases, in the order of solve_call ------------------------------------------------------------------------
    // The run-boundary buffers come first: without them (out of memory) an AUTO call on bits still has the transforms.
    int prepare() {
        int rc;
        if (runs_ok && (rc = ensure_runs(p, need_extract ? n_rr : 0, 0, (size_t)n_chunks))) {
            if (lists_in || p->algo != FFS_ALGO_AUTO) return rc;
            runs_ok = false;  // FFS_ALGO_AUTO: "only the time differs" -- the transforms need no list buffers
        }
        ml_on = runs_ok && ml;
        L = DescLayout((size_t)n_pairs, (size_t)n_cand, n_rr, ml_on, runs_ok,
                       p->seg ? (size_t)n_pairs * kSegBlocks * n_slots : n_xf);  // block-segmented mode needs more
        if ((rc = ensure_desc(p, L.total))) return rc;
        HIP_TRY(hipEventSynchronize(p->upload_done));  // previous call's upload has left the pinned buffer
        hb = (char*)p->host_desc;
        memset(L.pool(hb), 0, 64);
        L.pool(hb)->capacity = kPoolCapacity;
        // a stream of dense calls (the previous one needed the transforms): probe before extracting, upload on the call's stream
        dense_stream = p->algo == FFS_ALGO_AUTO && p->runs_prev_fft && !lists_in;
        use_copy = runs_ok && need_extract && !ml_on && !dense_stream && ensure_copy(p);
        p->cur_half = use_copy ? 1 - p->cur_half : 0;
        db = (char*)(p->cur_half ? p->dev_desc2 : p->dev_desc);
        hc = L.cands(hb);
        dc = L.cands(db);
        d_rv = L.runs_refs(db);
        dx = L.xforms(db);
        dn = L.nominees(db);
        da = L.acc(db);
        dpb = L.pool_best(db);
        pa = PoolArgs{dn, L.pool(db), nullptr, dpb, n_chunks};  // .entries: once the transform workspace exists
        pa.half_last = (hflags & HALF_LAST) ? 1 : 0;
        chunk_fft.assign((size_t)n_chunks, runs_ok ? 0 : 1);
        any_fft = !runs_ok;
        return FFS_OK;
    }
    // Run-boundary path, step 1: what the kernels need of every vector.
    int fill_runs_table() {
        RunsRef* hrv = L.runs_refs(hb);
        for (size_t i = 0; i < n_vec; ++i) {
            const int dt = (i % stride) ? a.dtype : a.ref_dt;
            if (dt == FFS_DTYPE_RUNS)  // caller-owned block: 16-byte header (n, ones, len, capacity), then the entries
                hrv[i] = RunsRef{(const int2*)((const char*)a.vec_ptr[i] + 16), (const int2*)a.vec_ptr[i], nullptr, (int32_t)a.vec_len[i], 0};
            else if (dt == FFS_DTYPE_U1)
                hrv[i] = RunsRef{p->runs_e + i * (size_t)p->runs_stride, p->runs_n + i, (const unsigned*)a.vec_ptr[i], (int32_t)a.vec_len[i], p->runs_stride};
            else  // a multi-level reference: its threshold planes follow the vectors
                hrv[i] = RunsRef{nullptr, p->runs_n + i, nullptr, (int32_t)a.vec_len[i], p->runs_stride};
        }
        if (!ml_on) return FFS_OK;
        // three threshold planes per reference, in the plan's plane buffer: their lists are extracted like the vectors'
        std::vector<size_t> poff;
        lvl_len_max = bit_image_offsets(a.vec_len, (size_t)n_pairs, (size_t)stride, 3, [](size_t) { return true; }, &poff);
        int rc;
        if ((rc = grow_device_buf(p, &p->lvl_buf, &p->lvl_bytes, poff[n_pairs]))) return rc;
        for (int pi = 0; pi < n_pairs; ++pi) {
            const size_t b = (size_t)pi * stride;
            const int32_t pw = (int32_t)((a.vec_len[b] + 31) / 32);
            unsigned* planes = (unsigned*)((char*)p->lvl_buf + poff[pi]);
            L.level_samples(hb)[pi] = a.vec_ptr[b];
            L.level_planes(hb)[pi] = planes;
            L.level_lens(hb)[pi] = (int32_t)a.vec_len[b];
            L.level_words(hb)[pi] = pw;
            for (int k = 0; k < 3; ++k) {
                const size_t r = n_vec + 3 * (size_t)pi + k;
                hrv[r] = RunsRef{p->runs_e + r * (size_t)p->runs_stride, p->runs_n + r, planes + (size_t)k * pw, (int32_t)a.vec_len[b], p->runs_stride};
            }
        }
        return FFS_OK;
    }
    template <class T>
    void launch_levels() {
        const unsigned chunks = (unsigned)((lvl_len_max + 16383) / 16384);
        LevelInfo* d_li = L.level_info(db);
        hipLaunchKernelGGL((k_levels_sample<T>), dim3((unsigned)n_pairs), dim3(256), 0, st, (const T* const*)L.level_samples(db),
                           (const int*)L.level_lens(db), d_li);
        hipLaunchKernelGGL((k_levels_bits<T>), dim3(chunks, (unsigned)n_pairs), dim3(256), 0, st, (const T* const*)L.level_samples(db),
                           (const int*)L.level_lens(db), d_li, (unsigned* const*)L.level_planes(db), (const int*)L.level_words(db));
    }
    // The lists of vectors that arrive as bits are extracted first -- the launch needs only the vector table, so the
    // candidate descriptors are built while the device reads the vectors.  Small calls: ONE upload (vector table + candidate
    // descriptors) and the extraction behind it, instead of the table, the extraction and then the candidates -- the host
    // takes longer to build ~1000 descriptors than the device to extract 1000 lists, so the early launch only moved a 20 us
    // hole behind the extraction and cost one more stream operation (profiles/small_step_timeline.py).
    int start_extraction_early() {
        int rc;
        if (ml_on) {
            if ((rc = upload(L.table_at(), L.level_tables_bytes(), false, true))) return rc;
            {
                ProfSpan lspan(p, st, FFS_K_LEVELS);
                if (a.ref_dt == FFS_DTYPE_F64) launch_levels<double>();
                else launch_levels<float>();
            }
            HIP_TRY(hipGetLastError());
            launch_extraction(n_rr, true, false);
            HIP_TRY(hipGetLastError());
        } else if (need_extract && n_cands <= kSmallCallCands && !dense_stream) {
            late_extract = true;
        } else if (need_extract) {
            if ((rc = upload(L.table_at(), L.table_bytes(n_vec), use_copy, true))) return rc;
            // A stream of dense calls: sample the vectors first -- when the estimate puts every sub-batch far over budget
            // the lists are never extracted (probe_dense_stream, once the candidate descriptors exist); otherwise the
            // extraction is launched then.
            probe_first = dense_stream;
            if (probe_first)
                hipLaunchKernelGGL(k_runs_probe, dim3((unsigned)((n_vec + 3) / 4)), dim3(256), 0, st, d_rv, (int)n_vec);
            else
                launch_extraction(n_vec, true, true);
            HIP_TRY(hipGetLastError());
        }
        return FFS_OK;
    }
    int fill_all_cands(const void* const* ptrs) {
        for (int pi = 0; pi < n_pairs; ++pi) {
            const size_t b = (size_t)pi * stride;
            const VecView ref = view(ptrs, b);
            for (int j = 0; j < n_cand; ++j) {
                CandDesc& cd = hc[(size_t)pi * n_cand + j];
                int rc;
                if ((rc = fill_cand(p, ref, view(ptrs, b + 1 + j), a.max_offset_samples, &cd, t_ref_dt, t_dtype))) return rc;
                if (runs_ok && !(cd.flags & CAND_NO_LAGS)) {
                    const int t = (cd.d_hi - cd.d_lo + RUNS_T) / RUNS_T;
                    if (t > tiles_max) tiles_max = t;
                }
            }
        }
        return FFS_OK;
    }
    // ---- descriptors of the transform path (built only when some sub-batch needs it) -------------------------
    int build_xforms() {
        int rc;
        xf_built = true;
        XformDesc* hx = L.xforms(hb);
        for (size_t i = 0; i < n_cands; ++i)
            if ((rc = finish_cand_for_transforms(p, a.max_offset_samples, &hc[i]))) return rc;
        std::vector<VecView> views((size_t)n_pairs * stride);  // per pair: reference, candidates (reachable prefixes)
        for (int pi = 0; pi < n_pairs; ++pi) {
            const size_t b = (size_t)pi * stride;
            VecView* v = &views[b];
            v[0] = view(xptr, b);
            int64_t ref_used = 1;
            for (int j = 0; j < n_cand; ++j) {
                v[1 + j] = view(xptr, b + 1 + j);
                const CandDesc& cd = hc[(size_t)pi * n_cand + j];
                // the transforms only read the prefixes that can reach the lag window (the exact re-evaluation
                // keeps working on the whole vectors through the candidate descriptor)
                int64_t s_eff, r_eff;
                effective_lengths(v[0].len, v[1 + j].len, cd.d_lo, cd.d_hi, &s_eff, &r_eff);
                if (!(cd.flags & CAND_NO_LAGS)) {
                    v[1 + j].len = s_eff;
                    if (r_eff > ref_used) ref_used = r_eff;
                }
            }
            v[0].len = ref_used;
            fill_xform(&hx[(size_t)pi * n_slots], &v[0], nullptr);
            for (int k = 0; k < n_packed; ++k)
                fill_xform(&hx[(size_t)pi * n_slots + 1 + k], &v[1 + 2 * k], (2 * k + 1 < n_cand) ? &v[2 + 2 * k] : nullptr);
        }
        // last-pass bins reachable by any lag window of this call (pruned pass C when there are few)
        std::vector<int> bin_set;
        bool bins_overflow = p->direct_only;
        for (size_t i = 0; i < n_cands && !bins_overflow; ++i) add_bins(p, hc[i], &bin_set, &bins_overflow);
        bins.n = (int)bin_set.size();
        for (int i = 0; i < bins.n; ++i) bins.b[i] = bin_set[i];
        pruned = p->allow_pruned && !bins_overflow && bins.n > 0 && bins.n * 2 <= p->N1;
        if (p->seg && p->allow_seg && p->allow_pruned && !p->direct_only && a.max_offset_samples >= 0 && p->seg->N2 == 4096 &&
            ref_half_ok(p->seg))
            build_seg_xforms(views);
        return FFS_OK;
    }
    // Block-segmented mode (see k_mid_seg): every candidate is cut into n_blocks <= 3 blocks of B samples,
    // block k is correlated with the reference stretch [kB + D_lo, kB + D_lo + M) by a length-M transform
    // (lag d at output index d - D_lo, nothing wraps), the blocks' spectrum products are added in the
    // mid pass.  [D_lo, D_hi] = union of the call's lag windows.  Taken when the window is narrow enough.
    void build_seg_xforms(const std::vector<VecView>& views) {
        const ffs_plan* sp = p->seg;
        int64_t d_lo = INT64_MAX, d_hi = INT64_MIN, s_max = 1;
        for (size_t i = 0; i < n_cands; ++i) {
            if (hc[i].flags & CAND_NO_LAGS) continue;
            if (hc[i].d_lo < d_lo) d_lo = hc[i].d_lo;
            if (hc[i].d_hi > d_hi) d_hi = hc[i].d_hi;
            const int64_t sl = views[(i / n_cand) * stride + 1 + i % n_cand].len;
            if (sl > s_max) s_max = sl;
        }
        if (d_lo > d_hi) return;
        const int64_t W = d_hi - d_lo + 1, B = sp->N - (W - 1);
        const int64_t nb = (W - 1) / sp->N2 + 1;
        if (!(B >= 1 && nb <= MAXBINS && nb * 2 <= sp->N1 && (s_max + B - 1) / B <= kSegBlocks)) return;
        seg = true;
        seg_blocks = (int)((s_max + B - 1) / B);
        seg_lo = d_lo;
        // byte / float vectors move the pointer to the block's first sample, bit-packed ones the bit offset
        const size_t esz = esz_of(t_dtype), esz_r = esz_of(t_ref_dt);
        XformDesc* hx = L.xforms(hb);
        n_xf = (size_t)n_pairs * seg_blocks * n_slots;
        std::vector<VecView> sb(n_cand);
        for (int pi = 0; pi < n_pairs; ++pi) {
            const VecView& ref = views[(size_t)pi * stride];
            for (int k = 0; k < seg_blocks; ++k) {
                XformDesc* x = &hx[((size_t)pi * seg_blocks + k) * n_slots];
                VecView rb = ref;  // positions [lead, len) of the block input = ref[start + n]
                const int64_t start = (int64_t)k * B + d_lo;
                rb.lead = start < 0 ? -start : 0;
                rb.len = ref.len - start < sp->N ? ref.len - start : sp->N;
                if (rb.len <= rb.lead) {
                    rb.len = rb.lead = 0;  // nothing of the reference in this stretch
                } else {
                    rb.ptr = (const char*)ref.ptr + start * (int64_t)esz_r;  // may point in front of the vector (lead)
                    if (!esz_r) rb.off = ref.off + start;
                }
                fill_xform(x, &rb, nullptr, ref.ptr);
                for (int j = 0; j < n_cand; ++j) {
                    sb[j] = views[(size_t)pi * stride + 1 + j];
                    const int64_t left = sb[j].len - (int64_t)k * B;
                    sb[j].len = left <= 0 ? 0 : (left < B ? left : B);
                    if (sb[j].len > 0) {
                        sb[j].ptr = (const char*)sb[j].ptr + (int64_t)k * B * (int64_t)esz;
                        if (!esz) sb[j].off += (int64_t)k * B;
                    }
                }
                for (int kk = 0; kk < n_packed; ++kk)
                    fill_xform(x + 1 + kk, &sb[2 * kk], (2 * kk + 1 < n_cand) ? &sb[2 * kk + 1] : nullptr, ref.ptr);
            }
        }
        memset(&bins, 0, sizeof bins);
        bins.n = (int)nb;
        for (int i = 0; i < bins.n; ++i) bins.b[i] = i;
        pruned = true;
    }
    // One upload when the transforms run anyway (the whole block); with the run-boundary path [header, candidates], plus
    // the vector table when no extraction was launched ahead of it -- small calls launch theirs here, behind the upload.
    // On the copy stream (use_copy) the block passes the previous call's kernels / goes up beside this call's extraction.
    int upload_descriptors() {
        int rc;
        const bool with_table = !need_extract || late_extract;
        if ((rc = upload(0, runs_ok ? L.head_bytes(with_table ? n_rr : 0) : L.transform_bytes(n_xf), use_copy))) return rc;
        if (late_extract) {
            launch_extraction(n_vec, true, true);
            HIP_TRY(hipGetLastError());
        }
        return FFS_OK;
    }
    int run_direct() {
        FFS_BY_RESCORE_DTYPE(mixed, t_dtype, hipLaunchKernelGGL((k_direct<DT>), dim3((unsigned)n_cands), dim3(256), 0, st, dc, cres));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_finalize_pairs, dim3((n_pairs + 255) / 256), dim3(256), 0, st, cres, pres, n_pairs, n_cand,
                           (long long)a.filter_max_offset);
        HIP_TRY(hipGetLastError());
        return FFS_OK;
    }

    // ---- run-boundary path: exact correlation of every candidate whose lists are short enough, candidate and pair
    // records written by the kernel itself; which sub-batches need the transforms instead is decided on the device
    // (k_runs_chunk_flags) and read back as one int per sub-batch -- after everything else of the call is queued
    unsigned long long* d_stats() const { return (unsigned long long*)((char*)p->runs_flags + flag_bytes - 16); }  // [boundaries, longest list]
    void launch_chunk_flags(int from_estimates) {
        hipLaunchKernelGGL(k_runs_chunk_flags, dim3((unsigned)n_chunks, runs_flag_split((long long)p->pairs_in_flight * n_cand)), dim3(256), 0, st,
                           dc, n_pairs, n_cand, p->pairs_in_flight, d_rv, budget, p->runs_flags, d_stats(), from_estimates);
    }
    int read_flags_async() {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(p->runs_flags_host, p->runs_flags, flag_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(p->runs_ev, st));
        return FFS_OK;
    }
    int run_boundary_path() {
        int rc;
        if ((rc = ensure_runs(p, need_extract ? n_rr : 0, tiles_max > 1 ? n_cands * (size_t)tiles_max : 0, (size_t)n_chunks))) return rc;
        proven = bounds_prove_budget();
        bool skip_runs = false;  // the probe says every sub-batch is dense: transforms only, nothing extracted
        if (probe_first && (rc = probe_dense_stream(&skip_runs))) return rc;
        if (skip_runs) return transforms_only();
        if ((rc = launch_flags_and_corr())) return rc;
        mark(&ht2);
        p->runs_calls += 1;
        p->runs_chunks += n_chunks;
        p->runs_last_boundaries = -1;  // (not known on the host when nothing was copied back)
        return proven ? FFS_OK : read_back_and_decide();
    }
    // Lists that arrive with host-known length bounds (the rasteriser's: two entries per subtitle) settle the question on
    // the host: within budget even at the bounds -> no flags kernel, no copy back, no wait.  A bound of RUNS_CAP or more
    // (16-bit histogram cells, as in k_runs_chunk_flags) proves nothing: the device decides.
    bool bounds_prove_budget() const {
        if (need_extract || !a.vec_bound) return false;
        for (int pi = 0; pi < n_pairs; ++pi) {
            const size_t bq = (size_t)pi * stride;
            if (a.vec_bound[bq] <= 0) return false;
            for (int j = 0; j < n_cand; ++j) {
                const CandDesc& cd = hc[(size_t)pi * n_cand + j];
                if (a.vec_bound[bq + 1 + j] <= 0 ||
                    (!(cd.flags & CAND_NO_LAGS) &&
                     runs_over_budget(a.vec_bound[bq + 1 + j], a.vec_bound[bq], RUNS_CAP, RUNS_CAP, (long long)cd.d_hi - cd.d_lo + 1, cd.R, budget)))
                    return false;
            }
        }
        return true;
    }
    // Flags from the ESTIMATED counts against the budget (the estimate's sampling error is a few per cent of a count whose
    // square enters: a sub-batch within that of the break-even costs the same either way).  *skip_runs: every sub-batch is dense.
    int probe_dense_stream(bool* skip_runs) {
        int rc;
        HIP_TRY(hipMemsetAsync(p->runs_flags, 0, flag_bytes, st));
        launch_chunk_flags(1);
        if ((rc = read_flags_async())) return rc;
        if ((rc = build_xforms())) return rc;  // (while the probe runs: needed in either case of a dense stream)
        HIP_TRY(hipEventSynchronize(p->runs_ev));
        *skip_runs = true;
        for (int ch = 0; ch < n_chunks; ++ch) *skip_runs = *skip_runs && p->runs_flags_host[ch] == 1;
        if (!*skip_runs) launch_extraction(n_vec, false, true);  // not (any more) a dense stream: the usual order from here on
        HIP_TRY(hipGetLastError());
        return FFS_OK;
    }
    int transforms_only() {
        int rc;
        for (int ch = 0; ch < n_chunks; ++ch) chunk_fft[ch] = 1;
        any_fft = true;
        p->runs_calls += 1;
        p->runs_chunks += n_chunks;
        p->runs_fft_chunks += n_chunks;
        p->runs_last_boundaries = -1;
        if ((rc = upload(L.refresh_at(), L.refresh_bytes(n_xf), false))) return rc;
        return clear_accumulators();
    }
    int launch_flags_and_corr() {
        const int* d_flags = proven ? p->runs_zero_flags : p->runs_flags;
        int rc;
        if (!proven) {
            // (flags + the statistics behind them: cleared by the extraction kernel of this call unless a probe has
            // written estimates into them since, or no extraction ran)
            if (!flags_cleared || probe_first) HIP_TRY(hipMemsetAsync(p->runs_flags, 0, flag_bytes, st));
            if (ml_on)
                hipLaunchKernelGGL(k_runs_chunk_flags_ml, dim3((unsigned)n_chunks), dim3(256), 0, st, dc, n_pairs, n_cand, p->pairs_in_flight,
                                   d_rv, (const LevelInfo*)L.level_info(db), (int)n_vec, budget, p->runs_flags, d_stats());
            else
                launch_chunk_flags(0);
            if ((rc = read_flags_async())) return rc;
        }
        {
            ProfSpan span(p, st, FFS_K_RUNS_CORR);
            if (ml_on) {
                hipLaunchKernelGGL(k_runs_corr_ml, dim3((unsigned)n_cands, (unsigned)tiles_max), dim3(RUNS_THREADS), 0, st, dc, n_cand, d_rv,
                                   cres, p->runs_best, tiles_max, d_flags, p->pairs_in_flight, (const LevelInfo*)L.level_info(db), (int)n_vec);
            } else {
                // One workgroup per candidate.  The kernel can also walk several candidates of a pair in one workgroup
                // (FFS_RUNS_SPLIT = workgroups per pair; the reference's list is then staged once for them), measured in
                // round 6: 7 x fewer stagings, but the 7 x longer workgroups leave the chip idle longer at the end of a
                // launch -- 0.248 against 0.238 us per pair at 4096 pairs (profiles/r06_runs_experiments.json).
                int split = n_cand;
                if (p->runs_split > 0) split = p->runs_split < n_cand ? p->runs_split : n_cand;
                hipLaunchKernelGGL(k_runs_corr, dim3((unsigned)((size_t)n_pairs * split), (unsigned)tiles_max), dim3(RUNS_THREADS), 0, st, dc,
                                   n_cand, d_rv, cres, p->runs_best, tiles_max, d_flags, p->pairs_in_flight, split);
            }
            if (tiles_max > 1)
                hipLaunchKernelGGL(k_runs_pick, dim3((unsigned)((n_cands + 255) / 256)), dim3(256), 0, st, dc, (int)n_cands, n_cand,
                                   p->runs_best, tiles_max, cres, d_flags, p->pairs_in_flight);
        }
        // (pairs of sub-batches that go through the transforms are finished again behind those)
        hipLaunchKernelGGL(k_finalize_pairs, dim3((n_pairs + 255) / 256), dim3(256), 0, st, cres, pres, n_pairs, n_cand,
                           (long long)a.filter_max_offset);
        HIP_TRY(hipGetLastError());
        return FFS_OK;
    }
    int read_back_and_decide() {
        int rc;
        // a stream of dense calls: the transform descriptors are built while the device extracts and decides
        // (unless a probe has built them already)
        if (!xf_built && p->runs_prev_fft && !lists_in && (rc = build_xforms())) return rc;
        HIP_TRY(hipEventSynchronize(p->runs_ev));  // k_runs_corr keeps the device busy meanwhile
        mark(&ht3);
        bool bad = false;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int f = p->runs_flags_host[ch];
            if (f == 2) bad = true;
            if (f) chunk_fft[ch] = 1, any_fft = true;
        }
        memcpy(&p->runs_last_boundaries, (char*)p->runs_flags_host + flag_bytes - 16, 8);
        // A plan-owned list filled its slot: the call is solved again with four times the room (at most twice from the
        // default: 4096 -> 16 384 -> 32 768 entries; what the first attempt wrote is overwritten in stream order), and the
        // plan keeps the longer stride.  Which path solves what therefore does not depend on the stride.
        long long longest = 0;
        memcpy(&longest, (char*)p->runs_flags_host + flag_bytes - 8, 8);
        if (need_extract && longest >= p->runs_stride && p->runs_stride < RUNS_CAP) {
            p->runs_stride = p->runs_stride * 4 < RUNS_CAP ? p->runs_stride * 4 : RUNS_CAP;
            p->runs_calls -= 1;
            p->runs_chunks -= n_chunks;
            retry = true;
            return FFS_OK;
        }
        if (bad)
            return fail(FFS_E_INVALID, "a boundary list of the call is truncated (more entries than its block holds): "
                        "nothing can solve it -- pass the vector as bits");
        p->runs_prev_fft = any_fft;
        return any_fft ? upload_for_fallback() : FFS_OK;
    }
    // Some sub-batches go through the transforms after all: complete and upload what those need.
    int upload_for_fallback() {
        int rc;
        for (int ch = 0; ch < n_chunks; ++ch) p->runs_fft_chunks += chunk_fft[ch];
        if (lists_in) {  // the transforms read bits: expand the list-only vectors, point the descriptors at them
            if ((rc = expand_list_vectors(p, a, st, &expanded))) return rc;
            xptr = expanded.data();
            const int tm = tiles_max;
            if ((rc = fill_all_cands(xptr))) return rc;
            tiles_max = tm;
        }
        if (!xf_built && (rc = build_xforms())) return rc;  // also completes the candidate descriptors (tie margins)
        if ((rc = upload(L.refresh_at(), L.refresh_bytes(n_xf), false))) return rc;
        for (int ch = 0; ch < n_chunks; ++ch) {  // clean accumulators for the sub-batches that are solved again
            if (!chunk_fft[ch]) continue;
            const size_t c0 = (size_t)ch * p->pairs_in_flight * n_cand;
            const size_t c1 = c0 + (size_t)p->pairs_in_flight * n_cand < n_cands ? c0 + (size_t)p->pairs_in_flight * n_cand : n_cands;
            HIP_TRY(hipMemsetAsync(da + c0 * KNOM, 0, L.acc_bytes(c1 - c0), st));
            HIP_TRY(hipMemsetAsync(dpb + c0, 0, (c1 - c0) * sizeof(PoolBest), st));
        }
        return FFS_OK;
    }
    int clear_accumulators() {
        HIP_TRY(hipMemsetAsync(da, 0, L.acc_and_best_bytes(), st));
        return FFS_OK;
    }

    // ---- transform path ----------------------------------------------------------------------------------------------
    // The pipeline of one sub-batch on plan `q`: the call's plan, or in block-segmented mode its length-M sub-plan (3x
    // shorter transforms, the blocks' spectrum products are added in the mid pass, last pass over one third of the data).
    // `slot_map`: see slot_stride()/cand_slot() in ffs_kernels.h.
    int launch_transform_chunk(ffs_plan* q, int flags, int slot_map, int seg_shift, int p0) {
        int rc = FFS_OK;
        const int blocks = seg ? seg_blocks : 1;
        const int np = (n_pairs - p0) < p->pairs_in_flight ? (n_pairs - p0) : p->pairs_in_flight;
        const int first_cand = p0 * n_cand, nx = np * blocks * n_slots;
        const int sel_ref = 0 | (1 << 16), sel_cand = 1 | ((n_slots - 1) << 16);  // row_sel of the two first-pass launches when mixed
        const XformDesc* dxs = dx + (size_t)p0 * blocks * n_slots;
        const bool full3 = !pruned && col3r_ok(q);  // full last pass over radix-3 columns: k_pass_c3's (wider) tiles
        PoolArgs qa = pa;
        qa.half_last = (flags & HALF_LAST) ? 1 : 0;
        const int done = p->dispatch.transform_sub_batches;  // (q may be p)
        q->dispatch = ffs_dispatch_report{};
        {
            ProfSpan span(p, st, FFS_K_PASS_A);
            if (mixed) {  // the reference slot of every group in its own type, then the candidate slots in theirs
                FFS_BY_DTYPE(t_ref_dt, rc = launch_pass_a<DT>(q, dxs, nx, n_slots, n_slots, flags, st, sel_ref));
                if (!rc) FFS_BY_DTYPE(t_dtype, rc = launch_pass_a<DT>(q, dxs, nx, n_slots, n_slots, flags, st, sel_cand));
            } else {
                FFS_BY_DTYPE(t_dtype, rc = launch_pass_a<DT>(q, dxs, nx, n_slots, n_slots, flags, st));
            }
        }
        if (rc) return rc;
        {
            ProfSpan span(p, st, FFS_K_MID);
            rc = seg ? launch_mid_seg(q, np, n_slots, seg_blocks, flags, st) : launch_mid(q, np, n_slots, flags, st);
        }
        if (rc) return rc;
        {
            ProfSpan span(p, st, FFS_K_PASS_C);
            rc = pruned  ? launch_pass_c_pruned<false>(q, dc, first_cand, n_cand, n_packed, slot_map, np, bins, qa, st, seg ? 1 : 0, seg_shift)
                 : full3 ? launch_pass_c3(q, dc, first_cand, n_cand, n_packed, slot_map, np, qa.half_last, st)
                         : launch_pass_c<0>(q, dc, first_cand, n_cand, n_packed, slot_map, np, nullptr, nullptr, qa, st);
        }
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(q->xlist, 0, sizeof(int), st));
        {
            ProfSpan span(p, st, FFS_K_NOMINEES);
            hipLaunchKernelGGL(k_nominees, dim3(np * n_cand), dim3(64), 0, st, q->bnom, full3 ? q->N2 / col3r_cols(q) : q->N2 / q->C, n_cand,
                               n_packed, dc, dn, first_cand, q->xlist);
        }
        HIP_TRY(hipGetLastError());
        // candidates whose nominee lists overflowed (listed by k_nominees): sweep their transforms again,
        // exhaustively; with an empty list the few blocks of this launch exit at once
        rc = pruned ? launch_pass_c_pruned<true>(q, dc, first_cand, n_cand, n_packed, slot_map, np, bins, qa, st, seg ? 1 : 0, seg_shift)
                    : launch_pass_c<2>(q, dc, first_cand, n_cand, n_packed, slot_map, np, nullptr, nullptr, qa, st);
        if (rc) return rc;
        {
            ProfSpan span(p, st, FFS_K_RESCORE);
            FFS_BY_RESCORE_DTYPE(mixed, t_dtype, hipLaunchKernelGGL((k_rescore<DT>), dim3(DT == 2 ? 4 : RSEG, np * n_cand), dim3(256), 0, st,
                                                                  dc, dn, da, first_cand));
        }
        HIP_TRY(hipGetLastError());
        p->dispatch = q->dispatch;
        p->dispatch.transform_sub_batches = done + 1;
        p->dispatch.transform_length = (int32_t)q->N;
        p->dispatch.n1 = q->N1;
        p->dispatch.n2 = q->N2;
        p->dispatch.seg_blocks = seg ? seg_blocks : 0;
        p->dispatch.half_flags = flags & (HALF_REF | HALF_LAST);
        return FFS_OK;
    }
    int run_transform_chunks() {
        if (!any_fft) return FFS_OK;
        int rc;
        if ((rc = ensure_workspace(p))) return rc;
        pa.entries = p->pool_entries;
        const int sflags = seg ? half_flags_of(p->seg, true) : 0;
        for (int p0 = 0; p0 < n_pairs; p0 += p->pairs_in_flight) {
            if (!chunk_fft[p0 / p->pairs_in_flight]) continue;
            rc = seg ? launch_transform_chunk(p->seg, sflags, seg_blocks * n_slots, (int)seg_lo, p0)
                     : launch_transform_chunk(p, hflags, n_slots, 0, p0);
            if (rc) return rc;
        }
        FFS_BY_RESCORE_DTYPE(mixed, t_dtype, hipLaunchKernelGGL((k_pool_rescore<DT>), dim3(2048), dim3(256), 0, st, dc, pa.header, pa.entries, dpb));
        hipLaunchKernelGGL(k_pool_pick, dim3(256), dim3(256), 0, st, pa.header, pa.entries, dpb);
        return FFS_OK;
    }
    // candidate and pair records of everything the transforms solved (the run-boundary kernels wrote their own)
    void finalize_range(size_t c0, size_t c1, int p0, int p1) {
        hipLaunchKernelGGL(k_finalize_cands, dim3((unsigned)((c1 - c0 + 255) / 256)), dim3(256), 0, st, dc + c0, dn + c0, da + c0 * KNOM,
                           cres + c0, (int)(c1 - c0), mixed ? 4 : t_dtype, pa.header, dpb + c0);
        hipLaunchKernelGGL(k_finalize_pairs, dim3((unsigned)((p1 - p0 + 255) / 256)), dim3(256), 0, st, cres + (size_t)p0 * n_cand, pres + p0,
                           p1 - p0, n_cand, (long long)a.filter_max_offset);
    }
    int finalize_transformed() {
        if (!runs_ok) finalize_range(0, n_cands, 0, n_pairs);
        for (int ch = 0; runs_ok && ch < n_chunks; ++ch) {
            if (!chunk_fft[ch]) continue;
            const int p0 = ch * p->pairs_in_flight, p1 = (p0 + p->pairs_in_flight) < n_pairs ? (p0 + p->pairs_in_flight) : n_pairs;
            finalize_range((size_t)p0 * n_cand, (size_t)p1 * n_cand, p0, p1);
        }
        HIP_TRY(hipGetLastError());
        return FFS_OK;
    }
    // the ONE leave_stream of a solve that reaches its end (`leave` covers the error returns)
    int finish() {
        leave.armed = false;
        const int rc = leave_stream(p, st);
        if (p->host_timing && runs_ok && !retry) {
            const double ht4 = now_ns();
            p->ht_vec += ht1 - ht0, p->ht_cand += ht2 - ht1, p->ht_wait += ht3 - ht2, p->ht_decide += ht4 - ht3, p->ht_total += ht4 - ht0;
        }
        return rc;
    }
};

// One solve, as the order of events.  *retry: a plan-owned list filled its slot -- the plan's stride has grown, solve again.
int solve_call(ffs_plan* p, const AlignArgs& a, bool* retry) {
    static_assert(sizeof(CandResult) == sizeof(ffs_cand_result), "ABI struct mismatch");
    static_assert(sizeof(PairResult) == sizeof(ffs_pair_result), "ABI struct mismatch");
    *retry = false;
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    p->dispatch = ffs_dispatch_report{};
    AlignCall c(p, a);
    if ((rc = enter_stream(p, c.st))) return rc;  // left by c.finish(), or by c.leave on an error return
    c.ht0 = c.ht1 = c.ht2 = c.ht3 = p->host_timing ? now_ns() : 0.0;
    if ((rc = c.prepare())) return rc;
    if (c.runs_ok) {
        if ((rc = c.fill_runs_table())) return rc;
        if ((rc = c.start_extraction_early())) return rc;
    }
    c.mark(&c.ht1);
    if ((rc = c.fill_all_cands(a.vec_ptr))) return rc;
    if (!c.runs_ok && (rc = c.build_xforms())) return rc;
    if ((rc = c.upload_descriptors())) return rc;
    if (p->direct_only) {
        if ((rc = c.run_direct())) return rc;
        return c.finish();
    }
    if ((rc = c.runs_ok ? c.run_boundary_path() : c.clear_accumulators())) return rc;
    if (c.retry) {
        *retry = true;
        return c.finish();
    }
    if ((rc = c.run_transform_chunks())) return rc;
    if ((rc = c.finalize_transformed())) return rc;
    return c.finish();
}

// The driver of every ffs_align_batch* call: check once, bring the inputs into a form the solve takes, split, solve.
int align_impl(ffs_plan* p, const AlignArgs& in) {
    int rc;
    if ((rc = check_align_args(p, in))) return rc;
    if (in.n_pairs == 0) return FFS_OK;
    AlignArgs a = in;
    std::vector<const void*> bits_ptr;  // the rewritten pointer table, when the inputs are rewritten
    const bool may_run = p->algo != FFS_ALGO_FFT && !p->direct_only;
    const bool lists_in = a.dtype == FFS_DTYPE_RUNS || a.ref_dt == FFS_DTYPE_RUNS;
    // (a multi-level float reference against two-level candidates takes the run-boundary path too: candidates that are
    // lists stay the caller's lists there -- k_runs_corr_ml reads their edge windows from the list -- and are expanded
    // only for a sub-batch that needs the transforms after all)
    const bool ml_split = (a.ref_dt == FFS_DTYPE_F64 || a.ref_dt == FFS_DTYPE_F32) && runs_able(a.dtype);
    if (may_run && a.dtype == FFS_DTYPE_U8 && a.ref_dt == FFS_DTYPE_U8)
        rc = pack_byte_vectors(p, &a, &bits_ptr);
    else if (lists_in && !(may_run && runs_able(a.dtype) && (runs_able(a.ref_dt) || ml_split)))
        rc = lists_to_bits(p, &a, &bits_ptr);
    if (rc) return rc;
    // The plan-owned boundary lists take 256 KiB per vector: a call with more than 65 536 vectors of bit-packed
    // two-level samples is solved as consecutive sub-calls (results land where one call would put them).
    // (a multi-level float reference brings three threshold planes of its own)
    const int64_t stride = 1 + a.n_cand;
    const int64_t per_pair = stride + (ml_split ? 3 : 0);
    const int64_t max_pairs = (int64_t(1) << 16) / per_pair > 0 ? (int64_t(1) << 16) / per_pair : 1;
    const bool split = may_run && runs_able(a.dtype) && (runs_able(a.ref_dt) || ml_split) && a.n_pairs > max_pairs;
    const int64_t step = split ? max_pairs : a.n_pairs;
    for (int64_t p0 = 0; p0 < a.n_pairs; p0 += step) {
        AlignArgs s = a;
        s.n_pairs = (int)((a.n_pairs - p0) < step ? (a.n_pairs - p0) : step);
        s.vec_ptr += p0 * stride, s.vec_len += p0 * stride, s.vec_lo += p0 * stride, s.vec_hi += p0 * stride;
        if (s.vec_bound) s.vec_bound += p0 * stride;
        s.cand_out_dev += p0 * a.n_cand, s.pair_out_dev += p0;
        // (solve_call asks again only while the stride can still grow: RUNS_CAP bounds the loop, two retries from the default)
        bool again = true;
        while (again)
            if ((rc = solve_call(p, s, &again))) return rc;
    }
    return FFS_OK;
}

}  // namespace

extern "C" {

int ffs_align_batch(ffs_plan* p, int n_pairs, int n_cand, int dtype, const void* const* vec_ptr,
                    const int64_t* vec_len, const double* vec_lo, const double* vec_hi, int64_t max_offset_samples,
                    int64_t filter_max_offset, ffs_cand_result* cand_out_dev, ffs_pair_result* pair_out_dev,
                    void* hip_stream) {
    return align_impl(p, AlignArgs{n_pairs, n_cand, dtype, dtype, vec_ptr, vec_len, vec_lo, vec_hi, nullptr, max_offset_samples,
                                   filter_max_offset, cand_out_dev, pair_out_dev, hip_stream});
}

int ffs_align_batch_runs(ffs_plan* p, int n_pairs, int n_cand, const int32_t* vec_dtype, const void* const* vec_ptr,
                         const int64_t* vec_len, const double* vec_lo, const double* vec_hi, const int32_t* vec_max_boundaries,
                         int64_t max_offset_samples, int64_t filter_max_offset, ffs_cand_result* cand_out_dev,
                         ffs_pair_result* pair_out_dev, void* hip_stream) {
    if (!vec_dtype) return fail(FFS_E_INVALID, "null argument");
    if (n_pairs <= 0 || n_cand < 1) return n_pairs == 0 ? FFS_OK : fail(FFS_E_INVALID, "bad n_pairs / n_cand");
    // one type per ROLE: every reference of the call shares vec_dtype[0], every candidate vec_dtype[1]
    const int ref_dt = vec_dtype[0], cand_dt = vec_dtype[1];
    const size_t stride = 1 + (size_t)n_cand;
    for (size_t i = 0; i < (size_t)n_pairs * stride; ++i)
        if (vec_dtype[i] != (i % stride == 0 ? ref_dt : cand_dt))
            return fail(FFS_E_INVALID, "vector %zu has element type %d: within one call all references must share one type "
                        "and all candidates one type (split the call)", i, (int)vec_dtype[i]);
    return align_impl(p, AlignArgs{n_pairs, n_cand, ref_dt, cand_dt, vec_ptr, vec_len, vec_lo, vec_hi, vec_max_boundaries,
                                   max_offset_samples, filter_max_offset, cand_out_dev, pair_out_dev, hip_stream});
}

int ffs_align_batch_typed(ffs_plan* p, int n_pairs, int n_cand, const int32_t* vec_dtype, const void* const* vec_ptr,
                          const int64_t* vec_len, const double* vec_lo, const double* vec_hi, int64_t max_offset_samples,
                          int64_t filter_max_offset, ffs_cand_result* cand_out_dev, ffs_pair_result* pair_out_dev,
                          void* hip_stream) {
    return ffs_align_batch_runs(p, n_pairs, n_cand, vec_dtype, vec_ptr, vec_len, vec_lo, vec_hi, nullptr, max_offset_samples,
                                filter_max_offset, cand_out_dev, pair_out_dev, hip_stream);
}

int64_t ffs_runs_list_bytes(int64_t cap) { return cap < 0 ? 0 : 16 + 8 * cap; }

int ffs_runs_from_bits(const uint32_t* bits_dev, int64_t len, void* list_dev, int64_t cap, void* hip_stream) {
    if (!bits_dev || !list_dev) return fail(FFS_E_INVALID, "null argument");
    if (len <= 0 || len >= (int64_t(1) << 30)) return fail(len <= 0 ? FFS_E_EMPTY : FFS_E_TOO_LONG, "vector of %lld samples", (long long)len);
    if (cap < 1 || cap >= (int64_t(1) << 28)) return fail(FFS_E_INVALID, "list capacity %lld outside [1, 2^28)", (long long)cap);
    if (((uintptr_t)bits_dev & 3) || ((uintptr_t)list_dev & 7)) return fail(FFS_E_INVALID, "misaligned pointer");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(list_dev))) return rc_dev;
    hipLaunchKernelGGL(k_runs_extract_one, dim3(1), dim3(1024), 0, st, (const unsigned*)bits_dev, (int)len,
                       (int2*)((char*)list_dev + 16), (int2*)list_dev, (int)cap);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_runs_to_bits(const void* list_dev, int64_t len, uint32_t* bits_out_dev, void* hip_stream) {
    if (!list_dev || !bits_out_dev) return fail(FFS_E_INVALID, "null argument");
    if (len <= 0 || len >= (int64_t(1) << 30)) return fail(len <= 0 ? FFS_E_EMPTY : FFS_E_TOO_LONG, "vector of %lld samples", (long long)len);
    if (((uintptr_t)bits_out_dev & 3) || ((uintptr_t)list_dev & 7)) return fail(FFS_E_INVALID, "misaligned pointer");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(list_dev))) return rc_dev;
    ExpandVec ev{(const int2*)((const char*)list_dev + 16), (const int2*)list_dev, (unsigned*)bits_out_dev, (int32_t)len, 0};
    ExpandVec* d_ev = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d_ev, sizeof ev, st));
    {
        hipError_t hu = hipMemcpyAsync(d_ev, &ev, sizeof ev, hipMemcpyHostToDevice, st);
        if (hu == hipSuccess) hu = hipStreamSynchronize(st);  // (ev is a stack temporary)
        if (hu != hipSuccess) {
            (void)hipFreeAsync(d_ev, st);
            HIP_TRY(hu);
        }
    }
    const int chunks = (int)(((len + 31) / 32 + 255) / 256);
    // (asynchronous: a block whose header does not fit it is never followed past its capacity -- the bits are then garbage)
    hipLaunchKernelGGL(k_runs_expand, dim3((unsigned)chunks), dim3(256), 0, st, (const ExpandVec*)d_ev, chunks, (int*)nullptr);
    const hipError_t he = hipGetLastError();
    const hipError_t hf = hipFreeAsync(d_ev, st);
    HIP_TRY(he);
    HIP_TRY(hf);
    return FFS_OK;
}

int ffs_correlate_full(ffs_plan* p, int dtype, const void* ref_dev, int64_t ref_len, double ref_lo, double ref_hi,
                       const void* a_dev, int64_t a_len, double a_lo, double a_hi, const void* b_dev, int64_t b_len,
                       double b_lo, double b_hi, float* out_a_dev, float* out_b_dev, void* hip_stream) {
    if (!p || p->direct_only) return fail(FFS_E_INVALID, "plan has no FFT path (n_fft < %lld)", (long long)kMinFftN);
    if (dtype != FFS_DTYPE_U8 && dtype != FFS_DTYPE_F32 && dtype != FFS_DTYPE_U1 && dtype != FFS_DTYPE_F64)
        return fail(FFS_E_INVALID, "unknown dtype %d", dtype);
    if (!ref_dev || !a_dev || ref_len <= 0 || a_len <= 0) return fail(FFS_E_EMPTY, "empty reference or candidate");
    if (ref_len > p->N || a_len > p->N || (b_dev && b_len > p->N)) return fail(FFS_E_TOO_LONG, "vector longer than n_fft");
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if ((rc = enter_stream(p, st))) return rc;
    if ((rc = ensure_workspace(p))) return rc;
    if ((rc = ensure_desc(p, 4096))) return rc;
    HIP_TRY(hipEventSynchronize(p->upload_done));
    p->cur_half = 0;
    XformDesc* hx = (XformDesc*)p->host_desc;
    VecView r{ref_dev, ref_len, ref_lo, ref_hi}, a{a_dev, a_len, a_lo, a_hi}, b{b_dev, b_len, b_lo, b_hi};
    fill_xform(&hx[0], &r, nullptr);
    fill_xform(&hx[1], &a, b_dev ? &b : nullptr);
    HIP_TRY(hipMemcpyAsync(p->dev_desc, hx, 2 * sizeof(XformDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(p->upload_done, st));
    const XformDesc* dx = (const XformDesc*)p->dev_desc;
    FFS_BY_DTYPE(dtype, rc = launch_pass_a<DT>(p, dx, 2, 2, 2, ref_half_ok(p) ? HALF_REF : 0, st));
    if (rc) return rc;
    if ((rc = launch_mid(p, 1, 2, ref_half_ok(p) ? HALF_REF : 0, st))) return rc;
    const PoolArgs none{nullptr, nullptr, nullptr, nullptr, 1};
    if ((rc = launch_pass_c<1>(p, nullptr, 0, 2, 1, 2, 1, out_a_dev, out_b_dev, none, st))) return rc;
    return leave_stream(p, st);
}

int64_t ffs_raster_length(const int64_t* end_us, int64_t n_subs, double ratio, double sample_rate) {
    double max_time = 0.0;  // speech_transformers.py:958-960
    for (int64_t i = 0; i < n_subs; ++i) {
        const double e = scaled_seconds(end_us[i], ratio);
        if (e > max_time) max_time = e;
    }
    return (int64_t)(max_time * sample_rate) + 2;       // :962
}

int ffs_raster_lengths(const int64_t* track_end_us_max, const double* ratio, int64_t n_vec, double sample_rate, int64_t* len_out) {
    if (n_vec < 0 || (n_vec > 0 && (!track_end_us_max || !ratio || !len_out))) return fail(FFS_E_INVALID, "bad argument");
    // the scaling is monotone (division, multiplication and the microsecond rounding all are), so a track's largest
    // scaled end is the scaled largest end
    for (int64_t v = 0; v < n_vec; ++v) len_out[v] = ffs_raster_length(&track_end_us_max[v], 1, ratio[v], sample_rate);
    return FFS_OK;
}

int64_t ffs_raster_intervals(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs,
                             double ratio, double sample_rate, double start_seconds, int64_t out_len, int32_t* iv_out) {
    int64_t n = 0;
    for (int64_t i = 0; i < n_subs; ++i) {
        if (is_metadata && is_metadata[i]) continue;    // speech_transformers.py:966-967
        long long a, b;
        if (raster_interval(start_us[i], end_us[i], ratio, sample_rate, start_seconds, out_len, &a, &b)) {
            iv_out[2 * n] = (int32_t)a;
            iv_out[2 * n + 1] = (int32_t)b;
            ++n;
        }
    }
    return n;
}

static int rasterize_impl(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs,
                          double ratio, double sample_rate, double start_seconds, void* out_dev, int64_t out_len,
                          bool bits, void* hip_stream) {
    if (n_subs < 0 || out_len < 0 || (n_subs > 0 && (!start_us || !end_us))) return fail(FFS_E_INVALID, "bad argument");
    if (out_len > 0 && !out_dev) return fail(FFS_E_INVALID, "null output");
    if (out_len >= (int64_t(1) << 31)) return fail(FFS_E_TOO_LONG, "raster longer than 2^31 samples");
    if (bits && ((uintptr_t)out_dev & 3)) return fail(FFS_E_INVALID, "bit-packed output must be 4-byte aligned");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(out_dev))) return rc_dev;
    if (out_len > 0) HIP_TRY(hipMemsetAsync(out_dev, 0, bits ? (size_t)((out_len + 31) / 32) * 4 : (size_t)out_len, st));
    // The interval list is a host temporary that an asynchronous copy reads later: park it in a
    // per-thread keep-alive list that is only emptied after a stream synchronisation, so that a run
    // of calls (seven ratios per file) costs one sync per 64 calls instead of one each.
    thread_local std::vector<std::vector<int32_t>> keep_alive;
    thread_local hipStream_t keep_stream = nullptr;
    if (keep_alive.size() >= 64 || (!keep_alive.empty() && keep_stream != st)) {
        HIP_TRY(hipStreamSynchronize(keep_stream));
        keep_alive.clear();
    }
    keep_stream = st;
    keep_alive.emplace_back((size_t)(2 * n_subs + 2));
    std::vector<int32_t>& iv = keep_alive.back();
    const int64_t n_iv = ffs_raster_intervals(start_us, end_us, is_metadata, n_subs, ratio, sample_rate, start_seconds,
                                              out_len, iv.data());
    if (n_iv == 0) {
        keep_alive.pop_back();
        return FFS_OK;
    }
    int2* d_iv = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d_iv, (size_t)n_iv * sizeof(int2), st));
    HIP_TRY(hipMemcpyAsync(d_iv, iv.data(), (size_t)n_iv * sizeof(int2), hipMemcpyHostToDevice, st));
    const int blocks = (int)((n_iv + 3) / 4);
    if (bits)
        hipLaunchKernelGGL(k_fill_intervals_bits, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, st, d_iv, (int)n_iv,
                           (unsigned*)out_dev);
    else
        hipLaunchKernelGGL(k_fill_intervals, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, st, d_iv, (int)n_iv,
                           (unsigned char*)out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipFreeAsync(d_iv, st));
    return FFS_OK;
}

int ffs_rasterize_subtitles(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs,
                            double ratio, double sample_rate, double start_seconds, uint8_t* out_dev, int64_t out_len,
                            void* hip_stream) {
    return rasterize_impl(start_us, end_us, is_metadata, n_subs, ratio, sample_rate, start_seconds, out_dev, out_len, false,
                          hip_stream);
}

int ffs_rasterize_subtitles_bits(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs,
                                 double ratio, double sample_rate, double start_seconds, uint32_t* out_dev,
                                 int64_t out_len, void* hip_stream) {
    return rasterize_impl(start_us, end_us, is_metadata, n_subs, ratio, sample_rate, start_seconds, out_dev, out_len, true,
                          hip_stream);
}

namespace {
// Pinned host staging for tables that an asynchronous copy reads after the entry point has returned.
struct PinnedStage {
    void* host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    int device = -1;
    bool pending = false;
};
int stage_acquire(size_t bytes, PinnedStage** out) {
    thread_local PinnedStage stages[2];
    thread_local int next = 0;
    PinnedStage& sg = stages[next];
    next ^= 1;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (sg.pending) {
        (void)hipEventSynchronize(sg.done);  // the copy that read this buffer (two calls ago) has completed
        sg.pending = false;
    }
    if (sg.done && sg.device != dev) {  // events belong to a device
        (void)hipEventDestroy(sg.done);
        sg.done = nullptr;
    }
    if (!sg.done) {
        HIP_TRY(hipEventCreateWithFlags(&sg.done, hipEventDisableTiming));
        sg.device = dev;
    }
    if (sg.cap < bytes) {
        if (sg.host) (void)hipHostFree(sg.host);
        sg.host = nullptr;
        sg.cap = 0;
        const size_t cap = bytes + bytes / 2 + 4096;
        HIP_TRY(hipHostMalloc(&sg.host, cap, hipHostMallocDefault));
        sg.cap = cap;
    }
    *out = &sg;
    return FFS_OK;
}
}  // namespace

int ffs_rasterize_batch_bits(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs_total,
                             const int64_t* vec_sub_first, const int64_t* vec_sub_count, const double* vec_ratio,
                             const int64_t* vec_out_word, const int64_t* vec_len, int64_t n_vec, double sample_rate,
                             double start_seconds, uint32_t* out_dev, int64_t out_words, void* hip_stream) {
    if (n_vec < 0 || n_subs_total < 0 || out_words < 0) return fail(FFS_E_INVALID, "bad argument");
    if (n_vec > 0 && (!vec_sub_first || !vec_sub_count || !vec_ratio || !vec_out_word || !vec_len))
        return fail(FFS_E_INVALID, "null vector table");
    if (n_subs_total > 0 && (!start_us || !end_us)) return fail(FFS_E_INVALID, "null subtitle arrays");
    if (out_words > 0 && (!out_dev || ((uintptr_t)out_dev & 3))) return fail(FFS_E_INVALID, "null or misaligned output");
    if (n_vec >= (int64_t(1) << 31)) return fail(FFS_E_INVALID, "too many vectors");
    std::vector<RasterVec> vecs((size_t)n_vec);
    int64_t longest = 0;
    for (int64_t v = 0; v < n_vec; ++v) {
        if (vec_sub_first[v] < 0 || vec_sub_count[v] < 0 || vec_sub_first[v] + vec_sub_count[v] > n_subs_total)
            return fail(FFS_E_INVALID, "vector %lld: subtitle range outside the arrays", (long long)v);
        if (vec_len[v] < 0 || vec_len[v] >= (int64_t(1) << 31)) return fail(FFS_E_TOO_LONG, "raster longer than 2^31 samples");
        if (vec_sub_count[v] >= (int64_t(1) << 31)) return fail(FFS_E_INVALID, "vector %lld: too many subtitles", (long long)v);
        if (vec_out_word[v] < 0 || vec_out_word[v] + (vec_len[v] + 31) / 32 > out_words)
            return fail(FFS_E_INVALID, "vector %lld: output range outside the buffer", (long long)v);
        vecs[(size_t)v] = RasterVec{(long long)vec_sub_first[v], (long long)vec_out_word[v], vec_ratio[v], (int)vec_sub_count[v],
                                    (int)vec_len[v]};
        if (vec_sub_count[v] > longest) longest = vec_sub_count[v];
    }
    if (out_words == 0) return FFS_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(out_dev))) return rc_dev;
    HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)out_words * 4, st));
    if (n_vec == 0 || longest == 0) return FFS_OK;
    // one staging allocation: start | end | vector table | metadata flags.  The tables are the caller's (and this
    // function's) pageable memory and must have been read before we return: they are copied into a pinned per-thread
    // staging buffer (two of them, alternating; a buffer is reused once the copy that read it has completed -- an event,
    // not a synchronisation of the caller's stream, which may hold a pipelined VAD sweep or the previous solve) and go
    // to the device in ONE asynchronous copy.
    const size_t nsub = (size_t)n_subs_total, off_end = nsub * 8, off_vec = 2 * nsub * 8;
    const size_t off_meta = off_vec + (size_t)n_vec * sizeof(RasterVec), total = off_meta + (is_metadata ? nsub : 0);
    PinnedStage* stage = nullptr;
    int rc = stage_acquire(total, &stage);
    if (rc) return rc;
    char* hs = (char*)stage->host;
    memcpy(hs, start_us, nsub * 8);
    memcpy(hs + off_end, end_us, nsub * 8);
    memcpy(hs + off_vec, vecs.data(), (size_t)n_vec * sizeof(RasterVec));
    if (is_metadata) memcpy(hs + off_meta, is_metadata, nsub);
    char* d = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d, total, st));
    if (hipMemcpyAsync(d, hs, total, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(FFS_E_HIP, "copying the subtitle tables failed");
    if (rc == FFS_OK && hipEventRecord(stage->done, st) == hipSuccess) stage->pending = true;
    if (rc == FFS_OK) {
        const unsigned bx = (unsigned)((longest + 255) / 256);
        hipLaunchKernelGGL(k_rasterize_batch, dim3(bx < 64 ? bx : 64, (unsigned)(n_vec < 65535 ? n_vec : 65535)), dim3(256), 0, st,
                           (const long long*)d, (const long long*)(d + off_end),
                           is_metadata ? (const unsigned char*)(d + off_meta) : nullptr, (const RasterVec*)(d + off_vec),
                           (int)n_vec, sample_rate, start_seconds, out_dev);
        if (hipGetLastError() != hipSuccess) rc = fail(FFS_E_HIP, "k_rasterize_batch launch failed");
    }
    (void)hipFreeAsync(d, st);
    return rc;
}

int ffs_rasterize_batch_runs(const int64_t* start_us, const int64_t* end_us, const uint8_t* is_metadata, int64_t n_subs_total,
                             const int64_t* vec_sub_first, const int64_t* vec_sub_count, const double* vec_ratio,
                             const int64_t* vec_out_off, const int64_t* vec_cap, const int64_t* vec_len, int64_t n_vec,
                             double sample_rate, double start_seconds, void* out_dev, int64_t out_bytes, void* hip_stream) {
    if (n_vec < 0 || n_subs_total < 0 || out_bytes < 0) return fail(FFS_E_INVALID, "bad argument");
    if (n_vec > 0 && (!vec_sub_first || !vec_sub_count || !vec_ratio || !vec_out_off || !vec_cap || !vec_len))
        return fail(FFS_E_INVALID, "null vector table");
    if (n_subs_total > 0 && (!start_us || !end_us)) return fail(FFS_E_INVALID, "null subtitle arrays");
    if (n_vec > 0 && (!out_dev || ((uintptr_t)out_dev & 7))) return fail(FFS_E_INVALID, "null or misaligned output");
    if (n_vec >= (int64_t(1) << 31)) return fail(FFS_E_INVALID, "too many vectors");
    if (start_seconds > 0.0)
        return fail(FFS_E_INVALID, "start_seconds > 0 can make start samples negative (Python slices wrap them around): "
                    "use ffs_rasterize_batch_bits");
    if (n_vec == 0) return FFS_OK;
    // DEVICE-resident subtitle tables (the same tracks rasterised again and again: the steps of a golden-section search, a
    // subtitle file against many references): nothing of them is copied, only the vector table travels.  They must be
    // sorted by start time already (the host cannot look).
    bool tables_on_device = false;
    if (n_subs_total > 0) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, start_us) == hipSuccess && attr.type == hipMemoryTypeDevice) {
            tables_on_device = true;
            hipPointerAttribute_t a2;
            if (hipPointerGetAttributes(&a2, end_us) != hipSuccess || a2.type != hipMemoryTypeDevice)
                return fail(FFS_E_INVALID, "start_us is device memory, end_us is not: the subtitle tables must live on one side");
            if (is_metadata && (hipPointerGetAttributes(&a2, is_metadata) != hipSuccess || a2.type != hipMemoryTypeDevice))
                return fail(FFS_E_INVALID, "start_us is device memory, is_metadata is not: the subtitle tables must live on one side");
        } else {
            (void)hipGetLastError();
        }
    }
    // Tracks must reach the kernel sorted by start time.  Unsorted ones (rare) are sorted into extra rows behind the
    // caller's; vectors naming the same unsorted range share one copy.
    std::vector<int64_t> xs, xe;
    std::vector<uint8_t> xm;
    std::vector<RasterRunsVec> vecs((size_t)n_vec);
    int64_t last_first = -1, last_count = -1, last_new_first = -1;
    for (int64_t v = 0; v < n_vec; ++v) {
        const int64_t f = vec_sub_first[v], c = vec_sub_count[v];
        if (f < 0 || c < 0 || f + c > n_subs_total) return fail(FFS_E_INVALID, "vector %lld: subtitle range outside the arrays", (long long)v);
        if (c >= (int64_t(1) << 27)) return fail(FFS_E_INVALID, "vector %lld: too many subtitles", (long long)v);
        if (vec_len[v] < 0 || vec_len[v] >= (int64_t(1) << 30)) return fail(FFS_E_TOO_LONG, "raster longer than 2^30 - 1 samples");
        if (vec_cap[v] < 2 * c + 1 || vec_cap[v] >= (int64_t(1) << 28))
            return fail(FFS_E_INVALID, "vector %lld: list capacity %lld below 2 * %lld subtitles + 1", (long long)v, (long long)vec_cap[v], (long long)c);
        if (vec_out_off[v] < 0 || (vec_out_off[v] & 7) || vec_out_off[v] + ffs_runs_list_bytes(vec_cap[v]) > out_bytes)
            return fail(FFS_E_INVALID, "vector %lld: list block outside the buffer or misaligned", (long long)v);
        int64_t first = f;
        if (tables_on_device) {
            // sorted by contract
        } else if (f == last_first && c == last_count) {
            first = last_new_first;
        } else {
            // (branch-free per block of 64: the compiler vectorises the comparison; an early exit per element does not)
            bool sorted = true;
            for (int64_t i0 = f + 1; i0 < f + c && sorted; i0 += 64) {
                const int64_t i1 = i0 + 64 < f + c ? i0 + 64 : f + c;
                int ok = 1;
                for (int64_t i = i0; i < i1; ++i) ok &= (int)(start_us[i - 1] <= start_us[i]);
                sorted = ok != 0;
            }
            if (!sorted) {
                std::vector<int64_t> idx((size_t)c);
                for (int64_t i = 0; i < c; ++i) idx[(size_t)i] = f + i;
                std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return start_us[x] < start_us[y]; });
                first = n_subs_total + (int64_t)xs.size();
                for (int64_t i : idx) {
                    xs.push_back(start_us[i]);
                    xe.push_back(end_us[i]);
                    xm.push_back(is_metadata ? is_metadata[i] : 0);
                }
            }
            last_first = f, last_count = c, last_new_first = first;
        }
        vecs[(size_t)v] = RasterRunsVec{(long long)first, (long long)vec_out_off[v], vec_ratio[v], (int32_t)c, (int32_t)vec_len[v],
                                        (int32_t)vec_cap[v], 0};
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(out_dev))) return rc_dev;
    // one staging allocation: start | end | vector table | metadata flags (see ffs_rasterize_batch_bits); with
    // device-resident tables only the vector table.  PINNED host tables (hipHostMalloc / hipHostRegister: the caller keeps
    // them alive and unchanged until the stream has passed this call) are copied to the device straight from where they
    // lie -- no staging copy on the host.
    bool tables_pinned = false;
    if (!tables_on_device && n_subs_total > 0 && xs.empty()) {
        hipPointerAttribute_t a0, a1, a2;
        tables_pinned = hipPointerGetAttributes(&a0, start_us) == hipSuccess && a0.type == hipMemoryTypeHost &&
                        hipPointerGetAttributes(&a1, end_us) == hipSuccess && a1.type == hipMemoryTypeHost &&
                        (!is_metadata || (hipPointerGetAttributes(&a2, is_metadata) == hipSuccess && a2.type == hipMemoryTypeHost));
        (void)hipGetLastError();
    }
    const bool stage_subs = !tables_on_device && !tables_pinned;
    const size_t nsub = tables_on_device ? 0 : (size_t)n_subs_total + xs.size(), off_end = nsub * 8, off_vec = 2 * nsub * 8;
    const bool with_meta = is_metadata != nullptr;
    const size_t off_meta = off_vec + (size_t)n_vec * sizeof(RasterRunsVec), total = off_meta + (with_meta && !tables_on_device ? nsub : 0);
    PinnedStage* stage = nullptr;
    int rc = stage_acquire(stage_subs ? total : (size_t)n_vec * sizeof(RasterRunsVec), &stage);
    if (rc) return rc;
    char* hs = (char*)stage->host;
    const size_t n0 = tables_on_device ? 0 : (size_t)n_subs_total;
    if (stage_subs) {
        if (n0) {
            memcpy(hs, start_us, n0 * 8);
            memcpy(hs + off_end, end_us, n0 * 8);
        }
        if (!xs.empty()) {
            memcpy(hs + n0 * 8, xs.data(), xs.size() * 8);
            memcpy(hs + off_end + n0 * 8, xe.data(), xe.size() * 8);
        }
        memcpy(hs + off_vec, vecs.data(), (size_t)n_vec * sizeof(RasterRunsVec));
        if (with_meta) {
            if (n0) memcpy(hs + off_meta, is_metadata, n0);
            if (!xm.empty()) memcpy(hs + off_meta + n0, xm.data(), xm.size());
        }
    } else {
        memcpy(hs, vecs.data(), (size_t)n_vec * sizeof(RasterRunsVec));
    }
    char* d = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d, total, st));
    if (stage_subs) {
        if (hipMemcpyAsync(d, hs, total, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(FFS_E_HIP, "copying the subtitle tables failed");
    } else {
        bool ok = hipMemcpyAsync(d + off_vec, hs, (size_t)n_vec * sizeof(RasterRunsVec), hipMemcpyHostToDevice, st) == hipSuccess;
        if (tables_pinned) {
            ok = ok && hipMemcpyAsync(d, start_us, n0 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d + off_end, end_us, n0 * 8, hipMemcpyHostToDevice, st) == hipSuccess;
            if (with_meta) ok = ok && hipMemcpyAsync(d + off_meta, is_metadata, n0, hipMemcpyHostToDevice, st) == hipSuccess;
        }
        if (!ok) rc = fail(FFS_E_HIP, "copying the subtitle tables failed");
    }
    if (rc == FFS_OK && hipEventRecord(stage->done, st) == hipSuccess) stage->pending = true;
    if (rc == FFS_OK) {
        const long long* d_start = tables_on_device ? (const long long*)start_us : (const long long*)d;
        const long long* d_end = tables_on_device ? (const long long*)end_us : (const long long*)(d + off_end);
        const unsigned char* d_meta = !with_meta ? nullptr : tables_on_device ? (const unsigned char*)is_metadata : (const unsigned char*)(d + off_meta);
        hipLaunchKernelGGL(k_rasterize_runs, dim3((unsigned)n_vec), dim3(256), 0, st, d_start, d_end, d_meta,
                           (const RasterRunsVec*)(d + off_vec), sample_rate, start_seconds, (char*)out_dev);
        if (hipGetLastError() != hipSuccess) rc = fail(FFS_E_HIP, "k_rasterize_runs launch failed");
    }
    (void)hipFreeAsync(d, st);
    return rc;
}

int ffs_runs_from_bits_batch(const uint32_t* const* bits_dev, const int64_t* len, void* const* list_dev, const int64_t* cap,
                             int64_t n_vec, void* hip_stream) {
    if (n_vec < 0 || (n_vec > 0 && (!bits_dev || !len || !list_dev || !cap))) return fail(FFS_E_INVALID, "bad argument");
    if (n_vec == 0) return FFS_OK;
    if (n_vec >= (int64_t(1) << 31)) return fail(FFS_E_INVALID, "too many vectors");
    for (int64_t v = 0; v < n_vec; ++v) {
        if (!bits_dev[v] || !list_dev[v]) return fail(FFS_E_INVALID, "vector %lld: null pointer", (long long)v);
        if (len[v] <= 0 || len[v] >= (int64_t(1) << 30))
            return fail(len[v] <= 0 ? FFS_E_EMPTY : FFS_E_TOO_LONG, "vector %lld of %lld samples", (long long)v, (long long)len[v]);
        if (cap[v] < 1 || cap[v] >= (int64_t(1) << 28)) return fail(FFS_E_INVALID, "vector %lld: list capacity %lld outside [1, 2^28)", (long long)v, (long long)cap[v]);
        if (((uintptr_t)bits_dev[v] & 3) || ((uintptr_t)list_dev[v] & 7)) return fail(FFS_E_INVALID, "vector %lld: misaligned pointer", (long long)v);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(list_dev[0]))) return rc_dev;
    PinnedStage* stage = nullptr;
    int rc = stage_acquire((size_t)n_vec * sizeof(RunsRef), &stage);
    if (rc) return rc;
    RunsRef* hr = (RunsRef*)stage->host;
    for (int64_t v = 0; v < n_vec; ++v)
        hr[v] = RunsRef{(const int2*)((const char*)list_dev[v] + 16), (const int2*)list_dev[v], (const unsigned*)bits_dev[v], (int32_t)len[v],
                        (int32_t)cap[v]};
    RunsRef* d = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d, (size_t)n_vec * sizeof(RunsRef), st));
    if (hipMemcpyAsync(d, hr, (size_t)n_vec * sizeof(RunsRef), hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(FFS_E_HIP, "copying the vector table failed");
    if (rc == FFS_OK && hipEventRecord(stage->done, st) == hipSuccess) stage->pending = true;
    if (rc == FFS_OK) {
        runs_extract_launch((const RunsRef*)d, (size_t)n_vec, true, st);
        if (hipGetLastError() != hipSuccess) rc = fail(FFS_E_HIP, "k_runs_extract_lists launch failed");
    }
    (void)hipFreeAsync(d, st);
    return rc;
}

// Host-only.  One activity vector as the reference hands it over (float64): are its samples two-level, and if so
// which levels, and the samples as bits -- ONE pass over the array instead of numpy's five temporaries.  The AVX2
// bodies are chosen at run time (the library is built without -march).
namespace {
struct MinMax {
    double lo, hi;
    bool nan;
};
// bits of up to 32 samples: bit k = (x[k] == hi); *ok is cleared when a sample equals neither level
uint32_t word_scalar(const double* x, int cnt, double lo, double hi, bool* ok) {
    uint32_t bits = 0, good = 1;
    for (int k = 0; k < cnt; ++k) {
        const uint32_t is_hi = x[k] == hi;
        good &= is_hi | (uint32_t)(x[k] == lo);
        bits |= is_hi << k;
    }
    if (!good) *ok = false;
    return bits;
}
#if FFS_HOST_AVX2
__attribute__((target("avx2"))) bool pack_avx2(const double* x, int64_t n_full_words, double lo, double hi, uint32_t* words) {
    const __m256d vlo = _mm256_set1_pd(lo), vhi = _mm256_set1_pd(hi);
    int all_ok = 0xf;
    for (int64_t w = 0; w < n_full_words; ++w) {
        const double* p = x + 32 * w;
        uint32_t bits = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const __m256d v = _mm256_loadu_pd(p + 4 * g);
            const __m256d eh = _mm256_cmp_pd(v, vhi, _CMP_EQ_OQ), el = _mm256_cmp_pd(v, vlo, _CMP_EQ_OQ);
            bits |= (uint32_t)_mm256_movemask_pd(eh) << (4 * g);
            all_ok &= _mm256_movemask_pd(_mm256_or_pd(eh, el));
        }
        words[w] = bits;
    }
    return all_ok == 0xf;
}
#endif
}  // namespace

int ffs_two_level_pack(const double* x, int64_t n, double* lo_out, double* hi_out, uint32_t* words) {
    if (n <= 0 || !x || !lo_out || !hi_out || !words) return fail(FFS_E_INVALID, "bad argument");
#if FFS_HOST_AVX2
    static const bool avx2 = __builtin_cpu_supports("avx2");
#else
    const bool avx2 = false;
#endif
    (void)avx2;
    // ONE pass over the samples (round 6; before: a min/max pass, then the packing pass -- 2 x 5.8 MB per 2 h vector, and
    // the drop-in's host time is this memory traffic): the first two distinct values are the candidate levels, the packing
    // pass itself verifies that every sample equals one of them.
    MinMax m{x[0], x[0], false};
    {
        int64_t i = 1;
        while (i < n && x[i] == x[0]) ++i;  // (a constant vector: this IS the one pass)
        if (i < n) {
            m.lo = x[i] < x[0] ? x[i] : x[0];
            m.hi = x[i] < x[0] ? x[0] : x[i];
        }
        m.nan = !(x[0] == x[0]) || (i < n && !(x[i] == x[i]));
    }
    *lo_out = m.lo;
    *hi_out = m.hi;
    if (m.nan || !std::isfinite(m.lo) || !std::isfinite(m.hi)) return 0;
    const int64_t n_words = (n + 31) / 32, n_full = n / 32;
    (void)n_full;
    if (m.hi == m.lo) {
        memset(words, 0, (size_t)n_words * 4);
        return 1;
    }
    bool ok = true;
    int64_t w = 0;
#if FFS_HOST_AVX2
    if (avx2) {
        ok = pack_avx2(x, n_full, m.lo, m.hi, words);
        w = n_full;
    }
#endif
    for (; ok && w < n_words; ++w) {
        const int64_t i0 = w * 32;
        words[w] = word_scalar(x + i0, (int)(n - i0 < 32 ? n - i0 : 32), m.lo, m.hi, &ok);
    }
    return ok ? 1 : 0;
}

int ffs_pack_bits(const void* src_dev, int src_dtype, int64_t n, double threshold, uint32_t* dst_dev, void* hip_stream) {
    if (n < 0 || (src_dtype != FFS_DTYPE_U8 && src_dtype != FFS_DTYPE_F32)) return fail(FFS_E_INVALID, "bad argument");
    if (n == 0) return FFS_OK;
    if (!src_dev || !dst_dev || ((uintptr_t)dst_dev & 3)) return fail(FFS_E_INVALID, "null or misaligned buffer");
    DeviceGuard guard;
    int rc;
    if ((rc = guard.enter(dst_dev))) return rc;
    const long long n_words = (n + 31) / 32;
    long long blocks = (n_words + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    // the kernel compares floats: for a float x, x > threshold <=> x > (the largest float not above the threshold)
    float thr = (float)threshold;
    if ((double)thr > threshold) thr = nextafterf(thr, -INFINITY);
    if (src_dtype == FFS_DTYPE_U8)
        hipLaunchKernelGGL((k_pack_bits<0>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, src_dev, (long long)n,
                           thr, dst_dev, n_words);
    else
        hipLaunchKernelGGL((k_pack_bits<1>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, src_dev, (long long)n,
                           thr, dst_dev, n_words);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_scatter_segments(const float* seg_labels_dev, const int64_t* seg_src_off, const int64_t* seg_dst_start,
                         const int64_t* seg_len, int n_segments, float* out_dev, int64_t out_len, void* hip_stream) {
    if (n_segments < 0 || out_len < 0 || (n_segments > 0 && (!seg_src_off || !seg_dst_start || !seg_len)))
        return fail(FFS_E_INVALID, "bad argument");
    if (out_len == 0) return FFS_OK;
    if (!out_dev) return fail(FFS_E_INVALID, "null device pointer");
    if (!seg_labels_dev)  // fine as long as no window holds a label (a detector that returned nothing)
        for (int i = 0; i < n_segments; ++i)
            if (seg_len[i] > 0) return fail(FFS_E_INVALID, "null device pointer");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc;
    if ((rc = guard.enter(out_dev))) return rc;
    HIP_TRY(hipMemsetAsync(out_dev, 0, (size_t)out_len * sizeof(float), st));
    for (int s0 = 0; s0 < n_segments; s0 += SCATTER_MAX) {
        ScatterSegs segs;
        memset(&segs, 0, sizeof segs);
        long long longest = 0;
        for (int i = s0; i < n_segments && i < s0 + SCATTER_MAX; ++i) {
            if (seg_len[i] < 0 || seg_src_off[i] < 0) return fail(FFS_E_INVALID, "negative segment length / source offset");
            // Python slice assignment sparse[lo:hi] = labels[:hi-lo] with lo = int(start*sample_rate) >= 0
            if (seg_dst_start[i] < 0 || seg_dst_start[i] >= out_len || seg_len[i] == 0) continue;
            segs.src_off[segs.n] = seg_src_off[i];
            segs.dst_start[segs.n] = seg_dst_start[i];
            segs.len[segs.n] = seg_len[i];
            if (seg_len[i] > longest) longest = seg_len[i];
            ++segs.n;
        }
        if (!segs.n) continue;
        long long bx = (longest + 255) / 256;
        if (bx > 1024) bx = 1024;
        hipLaunchKernelGGL(k_scatter_segments, dim3((unsigned)bx, segs.n), dim3(256), 0, st, seg_labels_dev, segs, out_dev,
                           (long long)out_len);
    }
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// ---- RCCL gather of the per-pair results (the only collective on the path) ---------------------
// RCCL is resolved at run time (dlopen), so single-GPU users of libffsalign.so do not load it; in a
// torch process the already-loaded librccl.so.1 is picked up, so both share one RCCL.
namespace {
struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, ffs_comm_id, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi* rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    static std::string load_error;
    std::call_once(once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if ((api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;  // the copy this process already has
        for (int i = 0; !api.handle && i < 3; ++i) api.handle = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
        if (api.handle) {
            api.GetUniqueId = (int (*)(void*))dlsym(api.handle, "ncclGetUniqueId");
            api.CommInitRank = (int (*)(void**, int, ffs_comm_id, int))dlsym(api.handle, "ncclCommInitRank");
            api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(api.handle, "ncclAllGather");
            api.CommDestroy = (int (*)(void*))dlsym(api.handle, "ncclCommDestroy");
            api.GetErrorString = (const char* (*)(int))dlsym(api.handle, "ncclGetErrorString");
        } else {
            const char* e = dlerror();  // may be null
            load_error = e ? e : "no loader message";
        }
    });
    if (!api.handle || !api.GetUniqueId || !api.CommInitRank || !api.AllGather || !api.CommDestroy) {
        fail(FFS_E_RCCL, "librccl.so.1 could not be loaded or lacks the nccl* entry points: %s",
             load_error.empty() ? "symbol missing" : load_error.c_str());
        return nullptr;
    }
    return &api;
}
int rccl_fail(RcclApi* a, const char* what, int code) {
    return fail(FFS_E_RCCL, "%s failed: %s", what, (a && a->GetErrorString) ? a->GetErrorString(code) : "?");
}
}  // namespace

struct ffs_comm {
    void* comm = nullptr;
    int device = 0, rank = 0, world = 1;
};

int ffs_comm_unique_id(ffs_comm_id* id_out) {
    if (!id_out) return fail(FFS_E_INVALID, "id_out is null");
    RcclApi* a = rccl_api();
    if (!a) return FFS_E_RCCL;  // message set by rccl_api()
    const int rc = a->GetUniqueId(id_out);
    return rc ? rccl_fail(a, "ncclGetUniqueId", rc) : FFS_OK;
}

int ffs_comm_create(int device, int rank, int world_size, const ffs_comm_id* id, ffs_comm** out) {
    if (!out || !id || world_size < 1 || rank < 0 || rank >= world_size) return fail(FFS_E_INVALID, "bad argument");
    *out = nullptr;
    RcclApi* a = rccl_api();
    if (!a) return FFS_E_RCCL;  // message set by rccl_api()
    HIP_TRY(hipSetDevice(device));
    ffs_comm* c = new ffs_comm();
    c->device = device;
    c->rank = rank;
    c->world = world_size;
    const int rc = a->CommInitRank(&c->comm, world_size, *id, rank);
    if (rc) {
        delete c;
        return rccl_fail(a, "ncclCommInitRank", rc);
    }
    *out = c;
    return FFS_OK;
}

int ffs_gather_results(ffs_comm* c, const ffs_pair_result* send_dev, int64_t n_local, ffs_pair_result* recv_dev,
                       void* hip_stream) {
    if (!c || n_local < 0) return fail(FFS_E_INVALID, "bad argument");
    if (n_local == 0) return FFS_OK;
    if (!send_dev || !recv_dev) return fail(FFS_E_INVALID, "null device pointer");
    RcclApi* a = rccl_api();
    if (!a) return fail(FFS_E_RCCL, "librccl.so.1 could not be loaded");
    HIP_TRY(hipSetDevice(c->device));
    const int rc = a->AllGather(send_dev, recv_dev, (size_t)n_local * sizeof(ffs_pair_result), /*ncclUint8*/ 1, c->comm,
                                (hipStream_t)hip_stream);
    return rc ? rccl_fail(a, "ncclAllGather", rc) : FFS_OK;
}

int ffs_comm_destroy(ffs_comm* c) {
    if (!c) return FFS_OK;
    RcclApi* a = rccl_api();
    if (a && c->comm) {
        (void)hipSetDevice(c->device);
        (void)a->CommDestroy(c->comm);
    }
    delete c;
    return FFS_OK;
}

int ffs_plan_set_algorithm(ffs_plan* p, int algorithm) {
    if (!p) return fail(FFS_E_INVALID, "plan is null");
    if (algorithm != FFS_ALGO_AUTO && algorithm != FFS_ALGO_FFT && algorithm != FFS_ALGO_RUNS)
        return fail(FFS_E_INVALID, "unknown algorithm %d", algorithm);
    p->algo = algorithm;
    return FFS_OK;
}

int ffs_plan_runs_stats(ffs_plan* p, int64_t* calls, int64_t* sub_batches, int64_t* sub_batches_through_transforms,
                        int64_t* boundaries_last_call) {
    if (!p) return fail(FFS_E_INVALID, "plan is null");
    if (calls) *calls = p->runs_calls;
    if (sub_batches) *sub_batches = p->runs_chunks;
    if (sub_batches_through_transforms) *sub_batches_through_transforms = p->runs_fft_chunks;
    if (boundaries_last_call) *boundaries_last_call = p->runs_last_boundaries;
    return FFS_OK;
}

int ffs_plan_dispatch_report(ffs_plan* p, ffs_dispatch_report* out) {
    if (!p || !out) return fail(FFS_E_INVALID, "plan and out must not be null");
    *out = p->dispatch;
    return FFS_OK;
}

int ffs_plan_profile(ffs_plan* p, int enable) {
    if (!p) return fail(FFS_E_INVALID, "plan is null");
    p->profiling = enable != 0;
    return FFS_OK;
}

int ffs_plan_profile_read(ffs_plan* p, double* ms_total, int64_t* launches) {
    if (!p || !ms_total || !launches) return fail(FFS_E_INVALID, "null argument");
    for (auto& sp : p->ev_spans) {
        HIP_TRY(hipEventSynchronize(sp.second.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, sp.second.first, sp.second.second));
        ms_total[sp.first] += (double)ms;
        launches[sp.first] += 1;
    }
    p->ev_spans.clear();
    p->ev_used = 0;
    return FFS_OK;
}

static int vad_energy_impl(const int16_t* pcm_dev, int64_t n_samples, int frame_len, double energy_threshold_db,
                           float non_speech_label, float* labels_dev, uint8_t* bits_dev, void* hip_stream) {
    if (n_samples < 0 || frame_len < 1) return fail(FFS_E_INVALID, "bad n_samples/frame_len");
    if (n_samples == 0) return FFS_OK;
    if (!pcm_dev || (!labels_dev && !bits_dev)) return fail(FFS_E_INVALID, "null device pointer");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(labels_dev ? (const void*)labels_dev : (const void*)bits_dev))) return rc_dev;
    const long long n_frames = (n_samples + frame_len - 1) / frame_len;
    const double thr_lin = pow(10.0, energy_threshold_db / 10.0);
    long long blocks = ((n_frames + VAD_FPT - 1) / VAD_FPT + 3) / 4;  // one wave per VAD_FPT frames, four waves per block
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(k_vad_energy, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, pcm_dev,
                       (long long)n_samples, frame_len, n_frames, thr_lin, non_speech_label, labels_dev, bits_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_vad_energy(const int16_t* pcm_dev, int64_t n_samples, int frame_len, double energy_threshold_db,
                   float non_speech_label, float* labels_dev, void* hip_stream) {
    if (n_samples > 0 && !labels_dev) return fail(FFS_E_INVALID, "null device pointer");
    return vad_energy_impl(pcm_dev, n_samples, frame_len, energy_threshold_db, non_speech_label, labels_dev, nullptr,
                           hip_stream);
}

int ffs_vad_energy_bits(const int16_t* pcm_dev, int64_t n_samples, int frame_len, double energy_threshold_db,
                        uint8_t* bits_dev, void* hip_stream) {
    if (n_samples > 0 && !bits_dev) return fail(FFS_E_INVALID, "null device pointer");
    return vad_energy_impl(pcm_dev, n_samples, frame_len, energy_threshold_db, 0.0f, nullptr, bits_dev, hip_stream);
}

int ffs_vad_tokenize(const float* valid_dev, int64_t n_frames, int64_t chunk_frames, int min_length, int max_length,
                     int max_continuous_silence, float non_speech_label, float* labels_dev, void* hip_stream) {
    if (n_frames < 0 || chunk_frames < 1 || max_length < 1) return fail(FFS_E_INVALID, "bad argument");
    if (n_frames == 0) return FFS_OK;
    if (!valid_dev || !labels_dev || valid_dev == labels_dev) return fail(FFS_E_INVALID, "null or aliased buffers");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(labels_dev))) return rc_dev;
    const long long chunks = (n_frames + chunk_frames - 1) / chunk_frames;
    const long long longest = chunk_frames < n_frames ? chunk_frames : n_frames;
    if (longest <= TOK_SCAN_MAX && max_length >= min_length && min_length >= 0) {
        // one workgroup per chunk (validity, island starts and markers as bit words in LDS: ffs_kernels.h)
        hipLaunchKernelGGL(k_vad_tokenize_scan, dim3((unsigned)chunks), dim3(TOK_THREADS), 0, (hipStream_t)hip_stream, valid_dev,
                           (long long)n_frames, (long long)chunk_frames, min_length, max_length, max_continuous_silence,
                           non_speech_label, labels_dev);
    } else {
        hipLaunchKernelGGL(k_vad_tokenize, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, (hipStream_t)hip_stream,
                           valid_dev, (long long)n_frames, (long long)chunk_frames, min_length, max_length,
                           max_continuous_silence, non_speech_label, labels_dev);
    }
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// ---- adaptive energy VAD (ffs_adaptive_vad.h) -------------------------------------------------------------

int ffs_vad_levels(const int16_t* pcm_dev, int64_t n_samples, int frame_len, const double* edges_dev, int n_edges,
                   uint8_t* levels_dev, void* hip_stream) {
    if (n_samples < 0 || frame_len < 1)
        return fail(FFS_E_INVALID, "ffs_vad_levels: bad n_samples=%lld / frame_len=%d", (long long)n_samples, frame_len);
    if (n_edges < 1 || n_edges > VAD_MAX_EDGES)
        return fail(FFS_E_INVALID, "ffs_vad_levels: n_edges=%d outside [1, %d]", n_edges, VAD_MAX_EDGES);
    if (n_samples == 0) return FFS_OK;
    if (!pcm_dev || !edges_dev || !levels_dev) return fail(FFS_E_INVALID, "ffs_vad_levels: null device pointer");
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(edges_dev) & 7))
        return fail(FFS_E_INVALID, "ffs_vad_levels: misaligned PCM (2 bytes) or edge table (8 bytes)");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(levels_dev))) return rc_dev;
    const long long n_frames = (n_samples + frame_len - 1) / frame_len;
    long long blocks = ((n_frames + VAD_FPT - 1) / VAD_FPT + 3) / 4;  // k_vad_energy's grid: a wave per VAD_FPT frames
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(k_vad_levels, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, pcm_dev,
                       (long long)n_samples, frame_len, n_frames, edges_dev, n_edges, levels_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_vad_level_hist(const uint8_t* levels_dev, int64_t n_frames, int n_bins, uint32_t* hist_dev, void* hip_stream) {
    if (n_frames < 0) return fail(FFS_E_INVALID, "ffs_vad_level_hist: n_frames=%lld is negative", (long long)n_frames);
    if (n_bins < 2 || n_bins > VAD_MAX_BINS)
        return fail(FFS_E_INVALID, "ffs_vad_level_hist: n_bins=%d outside [2, %d]", n_bins, VAD_MAX_BINS);
    if (!hist_dev || (n_frames > 0 && !levels_dev)) return fail(FFS_E_INVALID, "ffs_vad_level_hist: null device pointer");
    if (reinterpret_cast<uintptr_t>(hist_dev) & 3) return fail(FFS_E_INVALID, "ffs_vad_level_hist: misaligned histogram (4 bytes)");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(hist_dev))) return rc_dev;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(hist_dev, 0, sizeof(uint32_t) * (size_t)n_bins, st));
    if (n_frames == 0) return FFS_OK;  // the histogram of no frames
    long long blocks = (n_frames + HIST_BYTES_PER_TRIP - 1) / HIST_BYTES_PER_TRIP;
    if (blocks > HIST_MAX_BLOCKS) blocks = HIST_MAX_BLOCKS;
    hipLaunchKernelGGL(k_vad_level_hist, dim3((unsigned)blocks), dim3(HIST_THREADS), 0, st, levels_dev, (long long)n_frames,
                       n_bins, hist_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_vad_pick_threshold(const uint32_t* hist_dev, int n_hist, int n_bins, int rule, int lo_bin, int t_min, int t_max,
                           int fallback_bin, int floor_ppm, int margin_bins, ffs_vad_threshold* records_dev, void* hip_stream) {
    static_assert(sizeof(ffs_vad_threshold) == sizeof(VadThreshold), "device records must match the header's");
    if (n_hist < 0) return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: n_hist=%d is negative", n_hist);
    if (n_bins < 2 || n_bins > VAD_MAX_BINS)
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: n_bins=%d outside [2, %d]", n_bins, VAD_MAX_BINS);
    if (rule != VAD_RULE_OTSU && rule != VAD_RULE_FLOOR) return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: unknown rule %d", rule);
    if (!(0 <= lo_bin && lo_bin < t_min && t_min <= t_max && t_max <= n_bins - 1))
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: need 0 <= lo_bin=%d < t_min=%d <= t_max=%d <= n_bins - 1 = %d", lo_bin,
                    t_min, t_max, n_bins - 1);
    if (fallback_bin < 0 || fallback_bin > n_bins)
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: fallback_bin=%d outside [0, %d]", fallback_bin, n_bins);
    if (floor_ppm < 0 || floor_ppm > 1000000)
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: floor_ppm=%d outside [0, 1000000]", floor_ppm);
    if (margin_bins < 0 || margin_bins > VAD_MAX_EDGES)
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: margin_bins=%d outside [0, %d]", margin_bins, VAD_MAX_EDGES);
    if (n_hist == 0) return FFS_OK;
    if (!hist_dev || !records_dev) return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: null histogram or record pointer");
    if ((reinterpret_cast<uintptr_t>(hist_dev) & 3) || (reinterpret_cast<uintptr_t>(records_dev) & 7))
        return fail(FFS_E_INVALID, "ffs_vad_pick_threshold: misaligned histogram (4 bytes) or record (8 bytes) pointer");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(records_dev))) return rc_dev;
    hipLaunchKernelGGL(k_vad_pick_threshold, dim3((unsigned)n_hist), dim3(64), 0, (hipStream_t)hip_stream, hist_dev, n_bins, rule,
                       lo_bin, t_min, t_max, fallback_bin, floor_ppm, margin_bins, (VadThreshold*)records_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_vad_level_labels(const uint8_t* levels_dev, int64_t n_frames, const int32_t* threshold_dev, int threshold_host,
                         float non_speech_label, float* labels_dev, uint8_t* bits_dev, void* hip_stream) {
    if (n_frames < 0) return fail(FFS_E_INVALID, "ffs_vad_level_labels: n_frames=%lld is negative", (long long)n_frames);
    if (!threshold_dev && (threshold_host < 0 || threshold_host > VAD_MAX_BINS))
        return fail(FFS_E_INVALID, "ffs_vad_level_labels: threshold_host=%d outside [0, %d]", threshold_host, VAD_MAX_BINS);
    if (n_frames == 0) return FFS_OK;
    if (!levels_dev || (!labels_dev && !bits_dev)) return fail(FFS_E_INVALID, "ffs_vad_level_labels: null device pointer");
    if ((reinterpret_cast<uintptr_t>(threshold_dev) & 3) || (reinterpret_cast<uintptr_t>(labels_dev) & 3))
        return fail(FFS_E_INVALID, "ffs_vad_level_labels: misaligned threshold or label pointer (4 bytes)");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(levels_dev))) return rc_dev;
    long long blocks = (n_frames + LABEL_THREADS - 1) / LABEL_THREADS;
    if (blocks > LABEL_MAX_BLOCKS) blocks = LABEL_MAX_BLOCKS;
    hipLaunchKernelGGL(k_vad_level_labels, dim3((unsigned)blocks), dim3(LABEL_THREADS), 0, (hipStream_t)hip_stream, levels_dev,
                       (long long)n_frames, (const int*)threshold_dev, threshold_host, non_speech_label, labels_dev, bits_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// ---- steady-run gate behind the adaptive VAD (ffs_vad_gate.h) ---------------------------------------------

int64_t ffs_vad_steady_gate_workspace_bytes(int64_t n_frames) {
    if (n_frames <= 0 || n_frames > VAD_MAX_FRAMES) return 0;  // nothing to carry: no frames, or the gate is skipped
    return ((n_frames + GATE_TILE - 1) / GATE_TILE) * (int64_t)GATE_WS_PER_TILE;
}

int ffs_vad_steady_gate(const uint8_t* levels_dev, int64_t n_frames, const int32_t* threshold_dev, int threshold_host,
                        int dip_bins, int64_t max_run, float non_speech_label, float* labels_dev, uint8_t* bits_dev,
                        ffs_vad_gate* record_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream) {
    static_assert(sizeof(ffs_vad_gate) == sizeof(VadGate), "device records must match the header's");
    if (n_frames < 0) return fail(FFS_E_INVALID, "ffs_vad_steady_gate: n_frames=%lld is negative", (long long)n_frames);
    if (!threshold_dev && (threshold_host < 0 || threshold_host > VAD_MAX_BINS))
        return fail(FFS_E_INVALID, "ffs_vad_steady_gate: threshold_host=%d outside [0, %d]", threshold_host, VAD_MAX_BINS);
    if (dip_bins < 0 || dip_bins > VAD_MAX_EDGES)
        return fail(FFS_E_INVALID, "ffs_vad_steady_gate: dip_bins=%d outside [0, %d]", dip_bins, VAD_MAX_EDGES);
    if (max_run < 1 || max_run > 2147483647ll)
        return fail(FFS_E_INVALID, "ffs_vad_steady_gate: max_run=%lld outside [1, 2^31 - 1]", (long long)max_run);
    if (!record_dev || (n_frames > 0 && !levels_dev)) return fail(FFS_E_INVALID, "ffs_vad_steady_gate: null levels or record pointer");
    if ((reinterpret_cast<uintptr_t>(threshold_dev) & 3) || (reinterpret_cast<uintptr_t>(labels_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(record_dev) & 7) || (reinterpret_cast<uintptr_t>(workspace_dev) & 7))
        return fail(FFS_E_INVALID, "ffs_vad_steady_gate: misaligned threshold or label (4 bytes), record or workspace (8 bytes) pointer");
    const int64_t need = ffs_vad_steady_gate_workspace_bytes(n_frames);
    if (workspace_bytes < need || (need > 0 && !workspace_dev))
        return fail(FFS_E_INVALID, "ffs_vad_steady_gate: workspace of %lld bytes, %lld needed for %lld frames", (long long)workspace_bytes,
                    (long long)need, (long long)n_frames);
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(record_dev))) return rc_dev;
    hipStream_t st = (hipStream_t)hip_stream;
    const int* thr_dev = (const int*)threshold_dev;
    const bool too_long = n_frames > VAD_MAX_FRAMES;
    const int n_tiles = too_long ? 0 : (int)((n_frames + GATE_TILE - 1) / GATE_TILE);
    GateTile* tiles = (GateTile*)workspace_dev;
    int2* carry = (int2*)(tiles + n_tiles);
    if (too_long && (labels_dev || bits_dev)) {  // the plain labels, as ffs_vad_level_labels launches them
        long long blocks = (n_frames + LABEL_THREADS - 1) / LABEL_THREADS;
        if (blocks > LABEL_MAX_BLOCKS) blocks = LABEL_MAX_BLOCKS;
        hipLaunchKernelGGL(k_vad_level_labels, dim3((unsigned)blocks), dim3(LABEL_THREADS), 0, st, levels_dev, (long long)n_frames,
                           thr_dev, threshold_host, non_speech_label, labels_dev, bits_dev);
    }
    if (n_tiles)
        hipLaunchKernelGGL(k_gate_tiles, dim3((unsigned)n_tiles), dim3(GATE_THREADS), 0, st, levels_dev, (long long)n_frames, thr_dev,
                           threshold_host, dip_bins, (int)max_run, tiles);
    hipLaunchKernelGGL(k_gate_carry, dim3(1), dim3(GATE_THREADS), 0, st, tiles, n_tiles, (long long)n_frames, thr_dev, threshold_host,
                       dip_bins, (int)max_run, too_long ? 1 : 0, carry, (VadGate*)record_dev);
    if (n_tiles && (labels_dev || bits_dev))
        hipLaunchKernelGGL(k_gate_labels, dim3((unsigned)n_tiles), dim3(GATE_THREADS), 0, st, levels_dev, (long long)n_frames, thr_dev,
                           threshold_host, dip_bins, (int)max_run, carry, non_speech_label, labels_dev, bits_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// ---- centre-channel VAD: mid / side levels of stereo PCM and the centre gate (ffs_stereo_vad.h) -----------

int ffs_vad_stereo_levels(const int16_t* pcm_dev, int64_t n_pairs, int frame_len, const double* edges_dev, int n_edges,
                          uint8_t* mid_levels_dev, uint8_t* side_levels_dev, void* hip_stream) {
    if (n_pairs < 0 || frame_len < 1)
        return fail(FFS_E_INVALID, "ffs_vad_stereo_levels: bad n_pairs=%lld / frame_len=%d", (long long)n_pairs, frame_len);
    if (n_edges < 1 || n_edges > VAD_MAX_EDGES)
        return fail(FFS_E_INVALID, "ffs_vad_stereo_levels: n_edges=%d outside [1, %d]", n_edges, VAD_MAX_EDGES);
    if (n_pairs == 0) return FFS_OK;
    if (!pcm_dev || !edges_dev || !mid_levels_dev || !side_levels_dev)
        return fail(FFS_E_INVALID, "ffs_vad_stereo_levels: null device pointer");
    if ((reinterpret_cast<uintptr_t>(pcm_dev) & 1) || (reinterpret_cast<uintptr_t>(edges_dev) & 7))
        return fail(FFS_E_INVALID, "ffs_vad_stereo_levels: misaligned PCM (2 bytes) or edge table (8 bytes)");
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(mid_levels_dev))) return rc_dev;
    const long long n_frames = (n_pairs + frame_len - 1) / frame_len;
    long long blocks = ((n_frames + VAD_FPT - 1) / VAD_FPT + 3) / 4;  // k_vad_levels' grid: a wave per VAD_FPT frames
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(k_vad_stereo_levels, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, pcm_dev,
                       (long long)n_pairs, frame_len, n_frames, edges_dev, n_edges, mid_levels_dev, side_levels_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_vad_centre_gate(const uint8_t* mid_dev, const uint8_t* side_dev, int64_t n_frames, const int32_t* threshold_dev,
                        int threshold_host, int min_contrast_bins, uint8_t* out_levels_dev, ffs_vad_centre* record_dev,
                        void* hip_stream) {
    static_assert(sizeof(ffs_vad_centre) == sizeof(VadCentre), "device records must match the header's");
    if (n_frames < 0) return fail(FFS_E_INVALID, "ffs_vad_centre_gate: n_frames=%lld is negative", (long long)n_frames);
    if (!threshold_dev && (threshold_host < 0 || threshold_host > VAD_MAX_BINS))
        return fail(FFS_E_INVALID, "ffs_vad_centre_gate: threshold_host=%d outside [0, %d]", threshold_host, VAD_MAX_BINS);
    if (min_contrast_bins < 0 || min_contrast_bins > VAD_MAX_EDGES)
        return fail(FFS_E_INVALID, "ffs_vad_centre_gate: min_contrast_bins=%d outside [0, %d]", min_contrast_bins, VAD_MAX_EDGES);
    if (!record_dev || (n_frames > 0 && (!mid_dev || !side_dev)))
        return fail(FFS_E_INVALID, "ffs_vad_centre_gate: null mid, side or record pointer");
    if ((reinterpret_cast<uintptr_t>(threshold_dev) & 3) || (reinterpret_cast<uintptr_t>(record_dev) & 7))
        return fail(FFS_E_INVALID, "ffs_vad_centre_gate: misaligned threshold (4 bytes) or record (8 bytes) pointer");
    if (out_levels_dev && n_frames > 0) {  // the n_frames output bytes may not overlap either input's
        const uintptr_t o = reinterpret_cast<uintptr_t>(out_levels_dev), n = (uintptr_t)n_frames;
        const uintptr_t m = reinterpret_cast<uintptr_t>(mid_dev), s = reinterpret_cast<uintptr_t>(side_dev);
        if ((o < m + n && m < o + n) || (o < s + n && s < o + n))
            return fail(FFS_E_INVALID, "ffs_vad_centre_gate: out_levels_dev overlaps an input");
    }
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(record_dev))) return rc_dev;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipMemsetAsync(record_dev, 0, sizeof(ffs_vad_centre), st));
    if (n_frames > 0) {
        long long blocks = (n_frames + CENTRE_THREADS - 1) / CENTRE_THREADS;
        if (blocks > CENTRE_MAX_BLOCKS) blocks = CENTRE_MAX_BLOCKS;
        hipLaunchKernelGGL(k_centre_gate, dim3((unsigned)blocks), dim3(CENTRE_THREADS), 0, st, mid_dev, side_dev, (long long)n_frames,
                           (const int*)threshold_dev, threshold_host, min_contrast_bins, out_levels_dev, (VadCentre*)record_dev);
    }
    hipLaunchKernelGGL(k_centre_finish, dim3(1), dim3(64), 0, st, (long long)n_frames, (const int*)threshold_dev, threshold_host,
                       min_contrast_bins, (VadCentre*)record_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

int ffs_speech_bounds(const float* frames_dev, int64_t n_frames, int64_t* bounds_dev, void* hip_stream) {
    if (!bounds_dev || (n_frames > 0 && !frames_dev) || n_frames < 0) return fail(FFS_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(bounds_dev))) return rc_dev;
    hipLaunchKernelGGL(k_bounds_init, dim3(1), dim3(1), 0, st, (long long*)bounds_dev);
    if (n_frames > 0) {
        long long blocks = (n_frames + 255) / 256;
        if (blocks > 512) blocks = 512;
        hipLaunchKernelGGL(k_speech_bounds, dim3((unsigned)blocks), dim3(256), 0, st, frames_dev, (long long)n_frames,
                           (long long*)bounds_dev);
    }
    hipLaunchKernelGGL(k_bounds_fix, dim3(1), dim3(1), 0, st, (long long*)bounds_dev);
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

/* ---- host code shared by the per-file reductions and by the two resampled-list exports ------------------------ */

namespace {
extern "C++" {  // (function templates, inside this file's extern "C" block)
// The launch of a reduction with one workgroup per file, behind its export's own checks: nothing for no files, else
// `launch()` under the guard of the output's device.
template <class Launch>
int launch_per_file(int n_files, const void* out_dev, Launch launch) {
    if (n_files == 0) return FFS_OK;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(out_dev))) return rc_dev;
    launch();
    HIP_TRY(hipGetLastError());
    return FFS_OK;
}

// A reduction of n_files * (k + 1) solve records to one record per file (ffs_null_stats, ffs_offset_stats): the checks
// in the exports' order -- the counts, `own_checks()` for an export's further arguments, the pointers -- then the launch.
template <class Checks, class Launch>
int record_stats(const char* fn, const char* k_name, int k_max, const void* rec_dev, int n_files, int k, const void* out_dev,
                 Checks own_checks, Launch launch) {
    if (n_files < 0) return fail(FFS_E_INVALID, "%s: n_files=%d is negative", fn, n_files);
    if (k < 1 || k > k_max) return fail(FFS_E_INVALID, "%s: %s=%d outside [1, %d]", fn, k_name, k, k_max);
    if (int rc = own_checks()) return rc;
    if (!rec_dev || !out_dev) return fail(FFS_E_INVALID, "%s: null record or output pointer", fn);
    if (((uintptr_t)rec_dev | (uintptr_t)out_dev) & 7)
        return fail(FFS_E_INVALID, "%s: misaligned record or output pointer (8 bytes)", fn);
    return launch_per_file(n_files, out_dev, launch);
}
}

// What tells the two list exports apart: their names, their limits and the launch of their kernel, which receives the
// staged vector table (on the host and on the device) and returns an FFS_* code.
struct ListExport {
    const char* fn;
    const char* k_name;
    const char* block_name;
    int k_max, block_max;
    int (*launch)(const SurrVec* vecs_host, const SurrVec* vecs_dev, int64_t n_vec, int k, int block, char* out_dev,
                  int32_t* status_dev, hipStream_t st);
};

// K resampled lists per vector (ffs_surrogate_lists, ffs_subsample_lists): every argument check before the device is
// touched, the vector table staged in pinned memory and uploaded behind the caller's stream, then the export's launch.
int resampled_lists(const ListExport& x, const void* const* list_dev, const int32_t* n_bound, const uint32_t* seed,
                    const int64_t* out_off, const int64_t* out_cap, int64_t n_vec, int k, int block, void* out_dev,
                    int64_t out_bytes, int32_t* status_dev, void* hip_stream) {
    if (n_vec < 0 || out_bytes < 0)
        return fail(FFS_E_INVALID, "%s: n_vec=%lld or out_bytes=%lld is negative", x.fn, (long long)n_vec, (long long)out_bytes);
    if (k < 1 || k > x.k_max) return fail(FFS_E_INVALID, "%s: %s=%d outside [1, %d]", x.fn, x.k_name, k, x.k_max);
    if (block < 1 || block > x.block_max)
        return fail(FFS_E_INVALID, "%s: %s=%d outside [1, %d]", x.fn, x.block_name, block, x.block_max);
    if (n_vec == 0) return FFS_OK;
    if (!list_dev || !n_bound || !seed || !out_off || !out_cap) return fail(FFS_E_INVALID, "%s: null vector table", x.fn);
    if (!out_dev || !status_dev) return fail(FFS_E_INVALID, "%s: null output or status pointer", x.fn);
    if (((uintptr_t)out_dev & 7) || ((uintptr_t)status_dev & 3))
        return fail(FFS_E_INVALID, "%s: misaligned output (8 bytes) or status (4 bytes) pointer", x.fn);
    if (n_vec * k >= (int64_t(1) << 31))
        return fail(FFS_E_INVALID, "%s: n_vec * %s = %lld, need < 2^31", x.fn, x.k_name, (long long)(n_vec * k));
    for (int64_t v = 0; v < n_vec; ++v) {
        if (!list_dev[v] || ((uintptr_t)list_dev[v] & 7))
            return fail(FFS_E_INVALID, "%s: vector %lld: null or misaligned list pointer", x.fn, (long long)v);
        if (n_bound[v] < 0) return fail(FFS_E_INVALID, "%s: vector %lld: n_bound=%d is negative", x.fn, (long long)v, n_bound[v]);
        if (out_cap[v] < (int64_t)n_bound[v] + 1 || out_cap[v] >= (int64_t(1) << 28))
            return fail(FFS_E_INVALID, "%s: vector %lld: capacity %lld below n_bound + 1 = %lld (or 2^28 and more)", x.fn,
                        (long long)v, (long long)out_cap[v], (long long)n_bound[v] + 1);
        if (out_off[v] < 0 || (out_off[v] & 7) || out_off[v] > out_bytes ||
            ffs_runs_list_bytes(out_cap[v]) * k > out_bytes - out_off[v])
            return fail(FFS_E_INVALID, "%s: vector %lld: its %d blocks lie outside the buffer or are misaligned", x.fn,
                        (long long)v, k);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    DeviceGuard guard;
    int rc_dev;
    if ((rc_dev = guard.enter(out_dev))) return rc_dev;
    PinnedStage* stage = nullptr;
    int rc = stage_acquire((size_t)n_vec * sizeof(SurrVec), &stage);
    if (rc) return rc;
    SurrVec* hv = (SurrVec*)stage->host;
    for (int64_t v = 0; v < n_vec; ++v)
        hv[v] = SurrVec{(const char*)list_dev[v], (long long)out_off[v], seed[v], n_bound[v], (int32_t)out_cap[v], 0};
    SurrVec* d = nullptr;
    HIP_TRY(hipMallocAsync((void**)&d, (size_t)n_vec * sizeof(SurrVec), st));
    if (hipMemcpyAsync(d, hv, (size_t)n_vec * sizeof(SurrVec), hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(FFS_E_HIP, "%s: copying the vector table failed", x.fn);
    if (rc == FFS_OK && hipEventRecord(stage->done, st) == hipSuccess) stage->pending = true;
    if (rc == FFS_OK) rc = x.launch(hv, d, n_vec, k, block, (char*)out_dev, status_dev, st);
    (void)hipFreeAsync(d, st);
    return rc;
}

// The surrogate kernel sorts a list's blocks in dynamic LDS: sized for the largest block count of the call.
int launch_surrogate_lists(const SurrVec* vecs_host, const SurrVec* vecs_dev, int64_t n_vec, int n_surrogates, int block_units,
                           char* out_dev, int32_t* status_dev, hipStream_t st) {
    int most_blocks = 1;
    for (int64_t v = 0; v < n_vec; ++v) {
        // (a list above the unit limit is answered by empty surrogates: its blocks never reach the sort)
        const int n_bound = vecs_host[v].n_bound;
        const int units = n_bound / 2 - 1 < SURR_MAX_UNITS ? n_bound / 2 - 1 : SURR_MAX_UNITS;
        const int blocks = units > 0 ? (units + block_units - 1) / block_units : 0;
        if (blocks > most_blocks) most_blocks = blocks;
    }
    const size_t lds = surr_lds_bytes(most_blocks);
    if (lds > (64u << 10))
        HIP_TRY(hipFuncSetAttribute((const void*)k_surrogate_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_surrogate_lists, dim3((unsigned)(n_vec * n_surrogates)), dim3(SURR_THREADS), lds, st, vecs_dev,
                       n_surrogates, block_units, out_dev, status_dev);
    if (hipGetLastError() != hipSuccess) return fail(FFS_E_HIP, "k_surrogate_lists launch failed");
    return FFS_OK;
}

int launch_subsample_lists(const SurrVec*, const SurrVec* vecs_dev, int64_t n_vec, int n_subsamples, int block_runs,
                           char* out_dev, int32_t* status_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_subsample_lists, dim3((unsigned)(n_vec * n_subsamples)), dim3(STAB_THREADS), 0, st, vecs_dev,
                       n_subsamples, block_runs, out_dev, status_dev);
    if (hipGetLastError() != hipSuccess) return fail(FFS_E_HIP, "k_subsample_lists launch failed");
    return FFS_OK;
}

constexpr ListExport SURROGATE_LISTS = {"ffs_surrogate_lists", "n_surrogates", "block_units", SURR_MAX_K, SURR_MAX_UNITS,
                                        launch_surrogate_lists};
constexpr ListExport SUBSAMPLE_LISTS = {"ffs_subsample_lists", "n_subsamples", "block_runs", STAB_MAX_K, STAB_MAX_BLOCK_RUNS,
                                        launch_subsample_lists};
}  // namespace

int ffs_sweep_peaks(const ffs_cand_result* rec_dev, const int64_t* first_dev, int n_files, int top_k,
                    int64_t exclusion_steps, ffs_sweep_profile* out_dev, void* hip_stream) {
    static_assert(sizeof(ffs_sweep_profile) == sizeof(SweepProfile) && sizeof(ffs_cand_result) == sizeof(CandResult),
                  "device records must match the header's");
    if (n_files < 0) return fail(FFS_E_INVALID, "ffs_sweep_peaks: n_files=%d is negative", n_files);
    if (top_k < 1 || top_k > SWEEP_MAX_PEAKS)
        return fail(FFS_E_INVALID, "ffs_sweep_peaks: top_k=%d outside [1, %d]", top_k, SWEEP_MAX_PEAKS);
    if (exclusion_steps < 1)
        return fail(FFS_E_INVALID, "ffs_sweep_peaks: exclusion_steps=%lld, need >= 1", (long long)exclusion_steps);
    if (!rec_dev || !first_dev || !out_dev) return fail(FFS_E_INVALID, "ffs_sweep_peaks: null record, first or output pointer");
    if (((uintptr_t)rec_dev | (uintptr_t)first_dev | (uintptr_t)out_dev) & 7)
        return fail(FFS_E_INVALID, "ffs_sweep_peaks: misaligned record, first or output pointer (8 bytes)");
    // (its pointer checks cover `first_dev` and word them so: only the launch is the reductions' shared one)
    return launch_per_file(n_files, out_dev, [&] {
        hipLaunchKernelGGL(k_sweep_peaks, dim3((unsigned)n_files), dim3(SWEEP_THREADS), 0, (hipStream_t)hip_stream,
                           (const CandResult*)rec_dev, first_dev, top_k, exclusion_steps, (SweepProfile*)out_dev);
    });
}

int ffs_surrogate_lists(const void* const* list_dev, const int32_t* n_bound, const uint32_t* seed, const int64_t* out_off,
                        const int64_t* out_cap, int64_t n_vec, int n_surrogates, int block_units, void* out_dev,
                        int64_t out_bytes, int32_t* status_dev, void* hip_stream) {
    return resampled_lists(SURROGATE_LISTS, list_dev, n_bound, seed, out_off, out_cap, n_vec, n_surrogates, block_units, out_dev,
                           out_bytes, status_dev, hip_stream);
}

int ffs_null_stats(const ffs_cand_result* rec_dev, int n_files, int n_surrogates, ffs_null_result* out_dev, void* hip_stream) {
    static_assert(sizeof(ffs_null_result) == sizeof(NullResult), "device records must match the header's");
    return record_stats("ffs_null_stats", "n_surrogates", SURR_MAX_K, rec_dev, n_files, n_surrogates, out_dev,
                        [] { return FFS_OK; }, [&] {
        hipLaunchKernelGGL(k_null_stats, dim3((unsigned)n_files), dim3(SWEEP_THREADS), 0, (hipStream_t)hip_stream,
                           (const CandResult*)rec_dev, n_surrogates, (NullResult*)out_dev);
    });
}

int ffs_subsample_lists(const void* const* list_dev, const int32_t* n_bound, const uint32_t* seed, const int64_t* out_off,
                        const int64_t* out_cap, int64_t n_vec, int n_subsamples, int block_runs, void* out_dev,
                        int64_t out_bytes, int32_t* status_dev, void* hip_stream) {
    return resampled_lists(SUBSAMPLE_LISTS, list_dev, n_bound, seed, out_off, out_cap, n_vec, n_subsamples, block_runs, out_dev,
                           out_bytes, status_dev, hip_stream);
}

int ffs_offset_stats(const ffs_cand_result* rec_dev, int n_files, int n_subsamples, int64_t tol, ffs_stability_result* out_dev,
                     void* hip_stream) {
    static_assert(sizeof(ffs_stability_result) == sizeof(StabilityResult), "device records must match the header's");
    return record_stats("ffs_offset_stats", "n_subsamples", STAB_MAX_K, rec_dev, n_files, n_subsamples, out_dev,
                        [&] { return tol < 0 ? fail(FFS_E_INVALID, "ffs_offset_stats: tol=%lld is negative", (long long)tol) : FFS_OK; },
                        [&] {
        hipLaunchKernelGGL(k_offset_stats, dim3((unsigned)n_files), dim3(STAB_THREADS), 0, (hipStream_t)hip_stream,
                           (const CandResult*)rec_dev, n_subsamples, (long long)tol, (StabilityResult*)out_dev);
    });
}

/* ---- host code shared by the split, split range and quality plans --------------------------------------------- */

namespace {
int64_t split_align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// A device descriptor block, its pinned host staging and the event that marks the staging free again: fill the
// staging after wait_free(), then upload() it.  The device block may end in `dev_extra` bytes of device-only scratch.
struct DescStaging {
    void* dev = nullptr;
    void* host = nullptr;
    hipEvent_t free_event = nullptr;  // the last upload has left the staging buffer

    // FFS_OK, FFS_E_NOMEM when the device block is refused, FFS_E_HIP for the staging or the event (nothing kept)
    int create(size_t bytes, size_t dev_extra = 0) {
        if (hipMalloc(&dev, bytes + dev_extra) != hipSuccess) {
            dev = nullptr;
            return FFS_E_NOMEM;
        }
        if (hipHostMalloc(&host, bytes, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&free_event, hipEventDisableTiming) != hipSuccess) {
            release();
            return FFS_E_HIP;
        }
        return FFS_OK;
    }
    void release() {
        if (free_event) (void)hipEventDestroy(free_event);
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        dev = host = nullptr;
        free_event = nullptr;
    }
    int wait_free() {
        HIP_TRY(hipEventSynchronize(free_event));
        return FFS_OK;
    }
    int upload(size_t bytes, hipStream_t st) {
        HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(free_event, st));
        return FFS_OK;
    }
};

// A workspace laid out as a byte count that hands out typed blocks.  A plan states its layout once, as a function of a
// Carver, and runs it twice: over no memory to sum the bytes, then over the allocation to place the same blocks.
extern "C++" {  // (a member template, inside this file's extern "C" block)
struct Carver {
    char* base;  // nullptr: only count
    int64_t used = 0;

    // `count` elements, the block's bytes rounded up to a multiple of `pad`
    template <typename T>
    T* take(int64_t count, int64_t pad = 1) {
        T* at = base ? (T*)(base + used) : nullptr;
        used += split_align_up(count * (int64_t)sizeof(T), pad);
        return at;
    }
};
}

// What every plan holds: its device, the pairs one sub-batch solves, the workspace, the `done` event, and the blocks
// that calls made on first use.
struct PlanCore {
    int device = 0;
    int pairs_in_flight = 0;
    void* work = nullptr;
    int64_t work_bytes = 0;
    hipEvent_t done = nullptr;  // the plan's last call has finished with the workspace
    DescStaging desc;           // the descriptors of one sub-batch, made at create (each plan says what they are)
    std::vector<void*> blocks;            // device blocks made after open()
    std::vector<DescStaging*> stagings;   // descriptor blocks made after open()
    int64_t extra_bytes = 0;              // device bytes of both

    int64_t workspace_bytes() const { return work_bytes + extra_bytes; }

    // A block made by the first call that needs it, after that call's checks: "<plan>: <bytes> <kind> workspace bytes"
    // when the device refuses it.
    int add_block(void** out, int64_t bytes, const char* plan, const char* kind) {
        void* mem = nullptr;
        if (hipMalloc(&mem, (size_t)bytes) != hipSuccess)
            return fail(FFS_E_NOMEM, "%s: %lld %s workspace bytes", plan, (long long)bytes, kind);
        blocks.push_back(mem);
        extra_bytes += bytes;
        *out = mem;
        return FFS_OK;
    }
    // the retime workspace before it is made again larger (the caller has waited for `done`)
    void drop_block(void* block, int64_t bytes) {
        const auto at = std::find(blocks.begin(), blocks.end(), block);
        if (at == blocks.end()) return;
        (void)hipFree(block);
        blocks.erase(at);
        extra_bytes -= bytes;
    }
    // descriptors (and `dev_extra` bytes of device scratch behind them) made by the first call that needs them
    int add_staging(DescStaging* s, size_t bytes, size_t dev_extra, const char* what) {
        if (int rc = s->create(bytes, dev_extra)) return fail(rc, "%s", what);
        stagings.push_back(s);
        extra_bytes += (int64_t)(bytes + dev_extra);
        return FFS_OK;
    }

    // at create: the workspace, then `done`; on failure the caller destroys the plan
    int open(int dev, int pif, int64_t bytes, const char* what) {
        device = dev;
        pairs_in_flight = pif;
        if (hipMalloc(&work, bytes) != hipSuccess) {
            work = nullptr;
            return fail(FFS_E_NOMEM, "%s: %lld workspace bytes", what, (long long)bytes);
        }
        work_bytes = bytes;
        if (hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
            done = nullptr;
            return fail(FFS_E_HIP, "%s: event", what);
        }
        return FFS_OK;
    }
    // at destroy, before anything else is freed: wait for the last call, then free the workspace and every later block
    void close() {
        (void)hipSetDevice(device);
        if (done) {
            (void)hipEventSynchronize(done);
            (void)hipEventDestroy(done);
        }
        if (work) (void)hipFree(work);
        for (void* b : blocks) (void)hipFree(b);
        for (DescStaging* s : stagings) s->release();
        desc.release();
    }
    // every batch call, after its checks: on the plan's device, `st` waits until the previous call (any stream) is done
    int begin(hipStream_t st) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamWaitEvent(st, done, 0));
        return FFS_OK;
    }
    int end(hipStream_t st) {
        HIP_TRY(hipEventRecord(done, st));
        return FFS_OK;
    }
};

struct Levels {
    double s0, s1, r0, r1;      // 2 * level - 1 (aligners.py:55-57)
    double c00, c01, c10, c11;  // s~_x * r~_y for (s bit, r bit) = (0,0), (0,1), (1,0), (1,1)
};

// The per-pair host arrays of a batch call.
struct Pairs {
    const void* const* ref_ptr;
    const int64_t* ref_len;
    const double *ref_lo, *ref_hi;
    const void* const* sub_ptr;
    const int64_t* sub_len;
    const double *sub_lo, *sub_hi;

    bool any_null() const { return !ref_ptr || !ref_len || !ref_lo || !ref_hi || !sub_ptr || !sub_len || !sub_lo || !sub_hi; }

    // the checks of pair p that every batch call makes before its own limits
    int check(int p) const {
        if (ref_len[p] <= 0 || sub_len[p] <= 0)
            return fail(FFS_E_EMPTY, "cannot align empty speech data (reference length=%lld, subtitle length=%lld)",
                        (long long)(ref_len[p] > 0 ? ref_len[p] : 0), (long long)(sub_len[p] > 0 ? sub_len[p] : 0));
        if (!ref_ptr[p] || !sub_ptr[p] || ((uintptr_t)ref_ptr[p] & 3) || ((uintptr_t)sub_ptr[p] & 3))
            return fail(FFS_E_INVALID, "pair %d: null or misaligned vector", p);
        if (!(std::isfinite(ref_lo[p]) && std::isfinite(ref_hi[p]) && std::isfinite(sub_lo[p]) && std::isfinite(sub_hi[p])))
            return fail(FFS_E_INVALID, "pair %d: levels must be finite", p);
        return FFS_OK;
    }
    // ... and for the kernels that index samples with an int32
    int check_short(int p) const {
        if (int rc = check(p)) return rc;
        if (ref_len[p] > INT32_MAX / 2 || sub_len[p] > INT32_MAX / 2)
            return fail(FFS_E_INVALID, "pair %d: vectors longer than 2^30 samples", p);
        return FFS_OK;
    }

    Levels levels(int p) const {
#pragma clang fp contract(off)
        Levels v;
        v.s0 = mapped(sub_lo[p]);
        v.s1 = mapped(sub_hi[p]);
        v.r0 = mapped(ref_lo[p]);
        v.r1 = mapped(ref_hi[p]);
        v.c00 = v.s0 * v.r0;
        v.c01 = v.s0 * v.r1;
        v.c10 = v.s1 * v.r0;
        v.c11 = v.s1 * v.r1;
        return v;
    }

    // pair p's SplitDesc, its prefixes at pre_s and pre_r in the workspace, its outputs at row p
    ffsa::SplitDesc split_desc(int p, int32_t* pre_s, int32_t* pre_r) const {
        const Levels v = levels(p);
        ffsa::SplitDesc d;
        d.r = (const uint32_t*)ref_ptr[p];
        d.s = (const uint32_t*)sub_ptr[p];
        d.R = ref_len[p];
        d.S = sub_len[p];
        d.c00 = v.c00;
        d.c01 = v.c01;
        d.c10 = v.c10;
        d.c11 = v.c11;
        d.pre_r = pre_r;
        d.pre_s = pre_s;
        d.out_row = p;
        return d;
    }

    // pair p's RefineDesc, its null-score scratch at pair_ws (or none), its outputs at row p
    ffsa::RefineDesc refine_desc(int p, double* pair_ws) const {
        const Levels v = levels(p);
        ffsa::RefineDesc d;
        d.r = (const uint32_t*)ref_ptr[p];
        d.s = (const uint32_t*)sub_ptr[p];
        d.R = ref_len[p];
        d.S = sub_len[p];
        d.r0 = v.r0;
        d.r1 = v.r1;
        d.s0 = v.s0;
        d.s1 = v.s1;
        d.c00 = v.c00;
        d.c01 = v.c01;
        d.c10 = v.c10;
        d.c11 = v.c11;
        d.pair_ws = pair_ws;
        d.out_row = p;
        return d;
    }
};

/* The opening of every batch call: FFS_E_INVALID for a null plan ("null <name> plan"), n_pairs < 0 or, with pairs to
   solve, a null argument; FFS_OK when there are no pairs (the call is done); CALL_GO_ON otherwise. */
constexpr int CALL_GO_ON = 1;
int check_call(const void* plan, const char* name, int n_pairs, bool null_argument) {
    if (!plan) return fail(FFS_E_INVALID, "null %s plan", name);
    if (n_pairs < 0) return fail(FFS_E_INVALID, "n_pairs < 0");
    if (n_pairs == 0) return FFS_OK;
    if (null_argument) return fail(FFS_E_INVALID, "null argument");
    return CALL_GO_ON;
}

int check_block_samples(int64_t K) {
    if (K < 256 || K > ffsa::SPLIT_MAX_K || K % 32 != 0)
        return fail(FFS_E_INVALID, "block_samples=%lld: need a multiple of 32 in [256, 32768]", (long long)K);
    return FFS_OK;
}

// W = max_offset_samples of the window family, against the kernels' limit and the plan's
int check_window(int64_t W, int64_t plan_max_lags) {
    if (W < 1 || 2 * W > 262144) return fail(FFS_E_INVALID, "max_offset_samples=%lld: need 1 <= W, 2W <= 262144", (long long)W);
    if (2 * W > plan_max_lags)
        return fail(FFS_E_INVALID, "2 * max_offset_samples = %lld exceeds the plan's max_lags %lld", (long long)(2 * W),
                    (long long)plan_max_lags);
    return FFS_OK;
}

int check_split_penalty(double split_penalty) {
    if (!(split_penalty >= 0.0)) return fail(FFS_E_INVALID, "split_penalty must be >= 0 (not NaN)");
    return FFS_OK;
}

// `cap_note` names the cap where it is the plan's own
int check_step(int max_step, int cap, const char* cap_note, double step_cost) {
    if (max_step < 0 || max_step > cap) return fail(FFS_E_INVALID, "max_step=%d outside [0, %d]%s", max_step, cap, cap_note);
    if (!(step_cost >= 0.0) || !std::isfinite(step_cost)) return fail(FFS_E_INVALID, "step_cost must be finite and >= 0");
    return FFS_OK;
}

int check_peaks(int top_k, int64_t exclusion_samples) {
    if (top_k < 1 || top_k > ffsa::QUAL_MAX_PEAKS) return fail(FFS_E_INVALID, "top_k=%d outside [1, 8]", top_k);
    if (exclusion_samples < 1) return fail(FFS_E_INVALID, "exclusion_samples=%lld: need >= 1", (long long)exclusion_samples);
    return FFS_OK;
}

// pair p's blocks of K samples against the plan's limit; keeps the largest count
int check_blocks(int p, int64_t S, int64_t K, int64_t plan_max_blocks, int64_t* max_b) {
    const int64_t B = (S + K - 1) / K;
    if (B > plan_max_blocks)
        return fail(FFS_E_INVALID, "pair %d: %lld blocks exceed the plan's max_blocks %lld", p, (long long)B,
                    (long long)plan_max_blocks);
    *max_b = std::max(*max_b, B);
    return FFS_OK;
}
}  // namespace

/* ---- split-aware alignment (csrc/ffs_split.h) ---------------------------------------------------------------- */

namespace {
// What the split plan and the drift plan share: counts over a window of max_lags = 2W lags, the DP's tables, prefixes.
// The split DP keeps one stay bit per (block, lag) and one V row; the drift DP keeps DRIFT_PLANES code bits and two V rows.
struct WindowPlan : PlanCore {
    int64_t max_blocks, max_lags, max_samples;
    int64_t lpad, pw_s, pw_r, pre_slot;  // padded lag row, prefix words per vector and per slot
    ffsa::SplitWs ws;            // counts, stay bits (split only), V, arg
    unsigned long long* codes;   // drift only: [slot][max_blocks][lpad / 64][DRIFT_PLANES]
    int64_t codes_slot;
    int32_t* pre;                // [slot][pw_s + pw_r]
                                 // desc: SplitDesc[pairs_in_flight]

    void carve(Carver& c, bool drift) {
        const int64_t n = pairs_in_flight;
        ws.counts = c.take<uint16_t>(n * ws.counts_slot);
        ws.stay = drift ? nullptr : c.take<unsigned long long>(n * ws.stay_slot);
        codes = drift ? c.take<unsigned long long>(n * codes_slot) : nullptr;
        ws.V = c.take<double>(n * ws.v_slot);
        ws.arg = c.take<int32_t>(n * ws.arg_slot);
        pre = c.take<int32_t>(n * pre_slot);
    }
};

int window_plan_dims_check(const char* what, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples) {
    if (pairs_in_flight < 1 || max_blocks < 1 || max_lags < 2 || max_lags > 262144 || max_samples < 1)
        return fail(FFS_E_INVALID, "%s: need pairs_in_flight >= 1, max_blocks >= 1, 2 <= max_lags <= 262144, "
                                   "max_samples >= 1", what);
    return FFS_OK;
}

// the sizes, the workspace and the descriptors of a new window plan; on failure the caller destroys the plan
int window_plan_open(WindowPlan* p, const char* what, bool drift, int device, int pairs_in_flight, int64_t max_blocks,
                     int64_t max_lags, int64_t max_samples) {
    p->pairs_in_flight = pairs_in_flight;
    p->max_blocks = max_blocks;
    p->max_lags = max_lags;
    p->max_samples = max_samples;
    p->lpad = split_align_up(max_lags, 64);
    p->pw_s = max_samples / 32 + 2;
    p->pw_r = (max_samples + max_lags / 2) / 32 + 2;
    p->pre_slot = split_align_up(p->pw_s + p->pw_r, 64);                                          // int32
    p->ws.counts_row = p->lpad;
    p->ws.stay_row = p->lpad / 64;
    p->ws.counts_slot = split_align_up(max_blocks * p->lpad, 128);                                // uint16
    p->ws.stay_slot = drift ? 0 : split_align_up(max_blocks * (p->lpad / 64), 32);                // uint64
    p->codes_slot = drift ? split_align_up(max_blocks * (p->lpad / 64) * ffsa::DRIFT_PLANES, 32) : 0;  // uint64
    p->ws.v_slot = (drift ? 2 : 1) * split_align_up(p->lpad, 32);                                 // double
    p->ws.arg_slot = split_align_up(max_blocks, 64);                                              // int32
    Carver size{nullptr};
    p->carve(size, drift);
    if (int rc = p->open(device, pairs_in_flight, size.used, what)) return rc;
    Carver place{(char*)p->work};
    p->carve(place, drift);
    if (p->desc.create(sizeof(ffsa::SplitDesc) * (size_t)pairs_in_flight) != FFS_OK)
        return fail(FFS_E_HIP, "%s: descriptor buffers / events", what);
    return FFS_OK;
}

// the per-pair checks of the window calls: the subtitle's length and blocks against the plan; the largest block count
int window_limits_check(const WindowPlan* plan, int n_pairs, const Pairs& a, int64_t K, int64_t* max_b) {
    *max_b = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = a.check(p)) return rc;
        if (a.sub_len[p] > plan->max_samples)
            return fail(FFS_E_INVALID, "pair %d: subtitle length %lld exceeds the plan's max_samples %lld", p,
                        (long long)a.sub_len[p], (long long)plan->max_samples);
        if (int rc = check_blocks(p, a.sub_len[p], K, plan->max_blocks, max_b)) return rc;
    }
    return FFS_OK;
}

// the SplitDesc rows of the sub-batch [p0, p0 + np) filled and uploaded; its largest block count
int window_stage(WindowPlan* plan, const Pairs& a, int p0, int np, int64_t K, hipStream_t st, int64_t* chunk_b) {
    if (int rc = plan->desc.wait_free()) return rc;
    ffsa::SplitDesc* hd = (ffsa::SplitDesc*)plan->desc.host;
    *chunk_b = 0;
    for (int i = 0; i < np; ++i) {
        int32_t* pre_s = plan->pre + (int64_t)i * plan->pre_slot;
        hd[i] = a.split_desc(p0 + i, pre_s, pre_s + plan->pw_s);
        *chunk_b = std::max(*chunk_b, (hd[i].S + K - 1) / K);
    }
    return plan->desc.upload(sizeof(ffsa::SplitDesc) * np, st);
}

// the prefixes and the per-(block, lag) counts of a staged sub-batch of np pairs and at most chunk_b blocks
void window_counts(const WindowPlan* plan, int np, int64_t K, int64_t W, int64_t chunk_b, hipStream_t st) {
    const ffsa::SplitDesc* dd = (const ffsa::SplitDesc*)plan->desc.dev;
    const int n_tiles = (int)((2 * W + ffsa::SPLIT_TILE - 1) / ffsa::SPLIT_TILE);
    const int n_bgroups = (int)((chunk_b + ffsa::SPLIT_BPW - 1) / ffsa::SPLIT_BPW);
    hipLaunchKernelGGL(ffsa::k_split_prefix, dim3(2 * np), dim3(ffsa::SPLIT_PREFIX_THREADS), 0, st, dd, (int64_t)W);
    hipLaunchKernelGGL(ffsa::k_split_counts, dim3((unsigned)((int64_t)n_tiles * n_bgroups * np)),
                       dim3(ffsa::SPLIT_CNT_THREADS), 0, st, dd, plan->ws, (int)K, (int64_t)W, n_tiles, n_bgroups);
}
}  // namespace

struct ffs_split_plan : WindowPlan {
    uint32_t* curves = nullptr;        // report calls only, made by the first: per-piece n11 rows, [slot][max_blocks][lpad]
    DescStaging refine;                // refine calls only, made by the first: RefineDesc[pairs_in_flight], then on the device
    double* refine_scratch = nullptr;  // the null-score scratch [pairs_in_flight][4]
    DescStaging cue;                   // cue report calls only, made by the first: CueDesc[pairs_in_flight]
    DescStaging retime;                // cue retime calls only, made by the first: RetimeDesc[pairs_in_flight]
    void* retime_ws = nullptr;  // profiles and backpointers of one sub-batch, 6 bytes per (cue, delta); grows on demand
    int64_t retime_ws_bytes = 0;
};

int ffs_split_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                          ffs_split_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (int rc = window_plan_dims_check("split plan", pairs_in_flight, max_blocks, max_lags, max_samples)) return rc;
    HIP_TRY(hipSetDevice(device));
    ffs_split_plan* p = new (std::nothrow) ffs_split_plan();
    if (!p) return fail(FFS_E_NOMEM, "split plan");
    if (int rc = window_plan_open(p, "split plan", false, device, pairs_in_flight, max_blocks, max_lags, max_samples)) {
        ffs_split_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FFS_OK;
}

int ffs_split_plan_destroy(ffs_split_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

int64_t ffs_split_plan_workspace_bytes(const ffs_split_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

namespace {
struct SplitReportArgs {  // the per-piece report of ffs_align_split_report_batch
    int top_k;
    int64_t exclusion;
    ffs_piece_report* out;
    int32_t* n_pieces;
};

// ffs_align_split_batch, and with `rep` the piece reports after each sub-batch's DP
int split_batch(ffs_split_plan* plan, int n_pairs, const Pairs& a, int64_t block_samples, int64_t max_offset_samples,
                double split_penalty, int32_t* block_offset_out_dev, double* block_score_out_dev, double* total_out_dev,
                const SplitReportArgs* rep, void* hip_stream) {
    if (int rc = check_call(plan, "split", n_pairs, a.any_null() || !block_offset_out_dev || !block_score_out_dev || !total_out_dev);
        rc != CALL_GO_ON)
        return rc;
    const int64_t K = block_samples, W = max_offset_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_window(W, plan->max_lags)) return rc;
    if (int rc = check_split_penalty(split_penalty)) return rc;
    if (rep) {
        if (int rc = check_peaks(rep->top_k, rep->exclusion)) return rc;
        if (!rep->out || !rep->n_pieces) return fail(FFS_E_INVALID, "null argument");
        if (((uintptr_t)rep->out & 7) || ((uintptr_t)rep->n_pieces & 3)) return fail(FFS_E_INVALID, "misaligned report outputs");
    }
    int64_t max_b = 0;
    if (int rc = window_limits_check(plan, n_pairs, a, K, &max_b)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    if (rep && !plan->curves)  // the first report call: one uint32 n11 row per (slot, block)
        if (int rc = plan->add_block((void**)&plan->curves, (int64_t)plan->pairs_in_flight * plan->ws.counts_slot * 4,
                                     "split plan", "report"))
            return rc;
    const int64_t L = 2 * W;
    const ffsa::SplitDesc* dd = (const ffsa::SplitDesc*)plan->desc.dev;
    for (int p0 = 0; p0 < n_pairs; p0 += plan->pairs_in_flight) {
        const int np = std::min(plan->pairs_in_flight, n_pairs - p0);
        int64_t chunk_b = 0;
        if (int rc = window_stage(plan, a, p0, np, K, st, &chunk_b)) return rc;
        window_counts(plan, np, K, W, chunk_b, st);
        hipLaunchKernelGGL(ffsa::k_split_dp, dim3(np), dim3(ffsa::SPLIT_DP_THREADS), 0, st, dd, plan->ws, (int)K, (int64_t)W,
                           split_penalty, max_b, block_offset_out_dev, block_score_out_dev, total_out_dev);
        if (rep) {
            hipLaunchKernelGGL(ffsa::k_split_pieces, dim3(np), dim3(ffsa::PIECE_SCAN_THREADS), 0, st, dd, (int)K, max_b,
                               block_offset_out_dev, (ffsa::PieceReport*)rep->out, rep->n_pieces);
            const int n_sum_tiles = (int)((L + ffsa::PIECE_SUM_TILE - 1) / ffsa::PIECE_SUM_TILE);
            hipLaunchKernelGGL(ffsa::k_split_piece_sums, dim3((unsigned)((int64_t)n_sum_tiles * np)),
                               dim3(ffsa::PIECE_SUM_THREADS), 0, st, dd, plan->ws, plan->curves, (int)K, (int64_t)W,
                               n_sum_tiles, max_b, (const int32_t*)block_offset_out_dev);
            // one workgroup per possible piece (at most one per block); those past the pair's count return at once
            hipLaunchKernelGGL(ffsa::k_split_piece_report, dim3((unsigned)(chunk_b * np)), dim3(ffsa::QUAL_PEAK_THREADS), 0,
                               st, dd, plan->ws, (const uint32_t*)plan->curves, (int64_t)W, (int)chunk_b, max_b,
                               rep->top_k, rep->exclusion, (const int32_t*)rep->n_pieces, (ffsa::PieceReport*)rep->out);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}
}  // namespace

int ffs_align_split_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                          const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                          const double* sub_lo, const double* sub_hi, int64_t block_samples, int64_t max_offset_samples,
                          double split_penalty, int32_t* block_offset_out_dev, double* block_score_out_dev,
                          double* total_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    return split_batch(plan, n_pairs, a, block_samples, max_offset_samples, split_penalty, block_offset_out_dev,
                       block_score_out_dev, total_out_dev, nullptr, hip_stream);
}

int ffs_align_split_report_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int top_k, int64_t exclusion_samples,
                                 int32_t* block_offset_out_dev, double* block_score_out_dev, double* total_out_dev,
                                 ffs_piece_report* report_out_dev, int32_t* n_pieces_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    const SplitReportArgs rep{top_k, exclusion_samples, report_out_dev, n_pieces_out_dev};
    return split_batch(plan, n_pairs, a, block_samples, max_offset_samples, split_penalty, block_offset_out_dev,
                       block_score_out_dev, total_out_dev, &rep, hip_stream);
}

/* ---- sample-exact break refinement (csrc/ffs_split_refine.h) -------------------------------------------------- */

namespace {
// ffs_split_refine_batch (the breaks are the changes of offset, two constant lags per break), and with `drift`
// ffs_drift_refine_batch (the breaks are the jump flags of block_jump_dev, the lags follow the path)
int refine_batch(ffs_split_plan* plan, int n_pairs, const Pairs& a, int64_t block_samples,
                 const int32_t* block_offset_dev, bool drift, const uint8_t* block_jump_dev, int64_t radius_samples,
                 double unmatched_margin, ffs_break_refine* out_dev, int32_t* n_breaks_out_dev, void* hip_stream) {
    if (int rc = check_call(plan, "split", n_pairs,
                            a.any_null() || !block_offset_dev || !out_dev || !n_breaks_out_dev || (drift && !block_jump_dev));
        rc != CALL_GO_ON)
        return rc;
    if (((uintptr_t)block_offset_dev & 3) || ((uintptr_t)out_dev & 7) || ((uintptr_t)n_breaks_out_dev & 3))
        return fail(FFS_E_INVALID, "misaligned block offsets or refine outputs");
    const int64_t K = block_samples, Rr = radius_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (Rr < 1 || Rr > ffsa::REFINE_MAX_RADIUS)
        return fail(FFS_E_INVALID, "radius_samples=%lld: need 1 <= radius <= %lld", (long long)Rr,
                    (long long)ffsa::REFINE_MAX_RADIUS);
    const bool single = std::isnan(unmatched_margin);
    if (!single && !(unmatched_margin >= 0.0 && std::isfinite(unmatched_margin)))
        return fail(FFS_E_INVALID, "unmatched_margin must be finite and >= 0, or NaN for a single cut");
    int64_t max_b = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = a.check_short(p)) return rc;
        max_b = std::max(max_b, (a.sub_len[p] + K - 1) / K);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    if (!plan->refine.dev) {  // the first refine call: descriptors, their staging and the null-score scratch
        const size_t desc_bytes = sizeof(ffsa::RefineDesc) * (size_t)pif, scratch_bytes = sizeof(double) * 4 * (size_t)pif;
        if (int rc = plan->add_staging(&plan->refine, desc_bytes, scratch_bytes, "split plan: refine workspace")) return rc;
        plan->refine_scratch = (double*)((char*)plan->refine.dev + desc_bytes);
    }
    ffsa::RefineDesc* hd = (ffsa::RefineDesc*)plan->refine.host;
    const ffsa::RefineDesc* dd = (const ffsa::RefineDesc*)plan->refine.dev;
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        if (int rc = plan->refine.wait_free()) return rc;
        int64_t chunk_b = 0;
        for (int i = 0; i < np; ++i) {
            hd[i] = a.refine_desc(p0 + i, plan->refine_scratch + 4 * (int64_t)i);
            chunk_b = std::max(chunk_b, (hd[i].S + K - 1) / K);
        }
        if (int rc = plan->refine.upload(sizeof(ffsa::RefineDesc) * np, st)) return rc;
        if (drift)
            hipLaunchKernelGGL(ffsa::k_drift_refine_jumps, dim3(np), dim3(ffsa::REFINE_TABLE_THREADS), 0, st, dd, (int)K,
                               max_b, Rr, unmatched_margin, block_offset_dev, block_jump_dev, (ffsa::BreakRefine*)out_dev,
                               n_breaks_out_dev);
        else
            hipLaunchKernelGGL(ffsa::k_refine_breaks, dim3(np), dim3(ffsa::REFINE_TABLE_THREADS), 0, st, dd, (int)K, max_b,
                               Rr, unmatched_margin, block_offset_dev, (ffsa::BreakRefine*)out_dev, n_breaks_out_dev);
        if (chunk_b > 1) {  // one workgroup per possible break (at most one per block after the first)
            const int n_slots = (int)(chunk_b - 1);
            const dim3 grid((unsigned)((int64_t)n_slots * np));
            if (drift)
                hipLaunchKernelGGL(ffsa::k_drift_refine_cut, grid, dim3(ffsa::REFINE_THREADS), 0, st, dd, n_slots, (int)K,
                                   max_b, single, block_offset_dev, (const int32_t*)n_breaks_out_dev,
                                   (ffsa::BreakRefine*)out_dev);
            else
                hipLaunchKernelGGL(ffsa::k_refine_cut, grid, dim3(ffsa::REFINE_THREADS), 0, st, dd, n_slots, max_b, single,
                                   (const int32_t*)n_breaks_out_dev, (ffsa::BreakRefine*)out_dev);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}
}  // namespace

int ffs_split_refine_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                           const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                           const double* sub_lo, const double* sub_hi, int64_t block_samples,
                           const int32_t* block_offset_dev, int64_t radius_samples, double unmatched_margin,
                           ffs_break_refine* out_dev, int32_t* n_breaks_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    return refine_batch(plan, n_pairs, a, block_samples, block_offset_dev, false, nullptr, radius_samples, unmatched_margin,
                        out_dev, n_breaks_out_dev, hip_stream);
}

/* ---- sample-exact jumps of a drift solve (csrc/ffs_drift_refine.h) --------------------------------------------- */

int ffs_drift_refine_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                           const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                           const double* sub_lo, const double* sub_hi, int64_t block_samples,
                           const int32_t* block_offset_dev, const uint8_t* block_jump_dev, int64_t radius_samples,
                           double unmatched_margin, ffs_break_refine* out_dev, int32_t* n_jumps_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    return refine_batch(plan, n_pairs, a, block_samples, block_offset_dev, true, block_jump_dev, radius_samples,
                        unmatched_margin, out_dev, n_jumps_out_dev, hip_stream);
}

/* ---- per-cue evidence report (csrc/ffs_cue_report.h) ------------------------------------------------------------ */

namespace {
// the checks the cue report and the cue retime calls share
int check_cue_window(int64_t radius_samples, int64_t max_radius, int64_t context_samples) {
    if (radius_samples < 0 || radius_samples > max_radius)
        return fail(FFS_E_INVALID, "radius_samples=%lld: need 0 <= radius <= %lld", (long long)radius_samples, (long long)max_radius);
    if (context_samples < 0 || context_samples > ffsa::CUE_MAX_CONTEXT)
        return fail(FFS_E_INVALID, "context_samples=%lld: need 0 <= context <= %lld", (long long)context_samples,
                    (long long)ffsa::CUE_MAX_CONTEXT);
    return FFS_OK;
}

int check_cue_table_size(int64_t n_cues) {
    if (n_cues < 0 || n_cues > INT32_MAX / 2) return fail(FFS_E_INVALID, "n_cues=%lld: need 0 <= n_cues <= 2^30", (long long)n_cues);
    return FFS_OK;
}

// pair p's vectors and its slice of the cue table
int check_cue_pair(int p, const Pairs& a, const int64_t* cue_first, const int64_t* cue_count, int64_t n_cues) {
    if (int rc = a.check_short(p)) return rc;
    if (cue_count[p] < 0) return fail(FFS_E_INVALID, "pair %d: cue_count=%lld < 0", p, (long long)cue_count[p]);
    if (cue_first[p] < 0 || cue_first[p] > n_cues || cue_count[p] > n_cues - cue_first[p])
        return fail(FFS_E_INVALID, "pair %d: cues [%lld, +%lld) outside the table of %lld", p, (long long)cue_first[p],
                    (long long)cue_count[p], (long long)n_cues);
    return FFS_OK;
}
}  // namespace

int ffs_cue_report_batch(ffs_split_plan* plan, int n_pairs,const void* const* ref_ptr, const int64_t* ref_len,
                         const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                         const double* sub_lo, const double* sub_hi, const ffs_cue* cue_dev, int64_t n_cues,
                         const int64_t* cue_first, const int64_t* cue_count, int64_t radius_samples,
                         int64_t context_samples, ffs_cue_report* out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "split", n_pairs, a.any_null() || !cue_first || !cue_count); rc != CALL_GO_ON) return rc;
    if (int rc = check_cue_window(radius_samples, ffsa::CUE_MAX_RADIUS, context_samples)) return rc;
    if (int rc = check_cue_table_size(n_cues)) return rc;
    int64_t total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = check_cue_pair(p, a, cue_first, cue_count, n_cues)) return rc;
        total += cue_count[p];
    }
    if (total == 0) return FFS_OK;
    if (!cue_dev || !out_dev || ((uintptr_t)cue_dev & 7) || ((uintptr_t)out_dev & 7))
        return fail(FFS_E_INVALID, "null or misaligned cue table or report output");
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    if (!plan->cue.dev)  // the first cue report call: descriptors and their staging
        if (int rc = plan->add_staging(&plan->cue, sizeof(ffsa::CueDesc) * (size_t)pif, 0, "split plan: cue report workspace"))
            return rc;
    ffsa::CueDesc* hd = (ffsa::CueDesc*)plan->cue.host;
    const ffsa::CueDesc* dd = (const ffsa::CueDesc*)plan->cue.dev;
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        int nd = 0;
        int64_t grid = 0;
        for (int i = 0; i < np; ++i) grid += cue_count[p0 + i];
        if (grid == 0) continue;
        if (int rc = plan->cue.wait_free()) return rc;
        grid = 0;
        for (int i = 0; i < np; ++i) {  // pairs without cues get no descriptor
            const int p = p0 + i;
            if (cue_count[p] == 0) continue;
            ffsa::CueDesc& c = hd[nd++];
            c.v = a.refine_desc(p, nullptr);
            c.cue_first = cue_first[p];
            c.grid_first = grid;
            c.cue_count = cue_count[p];
            grid += cue_count[p];
        }
        if (int rc = plan->cue.upload(sizeof(ffsa::CueDesc) * nd, st)) return rc;
        hipLaunchKernelGGL(ffsa::k_cue_report, dim3((unsigned)grid), dim3(ffsa::CUE_THREADS), 0, st, dd, nd,
                           (const ffsa::Cue*)cue_dev, (int)radius_samples, (int)context_samples, (ffsa::CueReport*)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- joint cue retiming (csrc/ffs_cue_retime.h) ------------------------------------------------------------------ */

namespace {
// the pairs [p0, p0 + np) of the next sub-batch: at most pairs_in_flight of them, their cells within the workspace cap
// (every pair alone fits: checked before); returns np and the sub-batch's cues
int retime_cut(const int64_t* cue_count, int n_pairs, int p0, int pif, int64_t n_delta, int64_t* rows_out) {
    int np = 0;
    int64_t rows = 0;
    while (p0 + np < n_pairs && np < pif) {
        const int64_t c = cue_count[p0 + np];
        if (np > 0 && (rows + c) * n_delta * ffsa::RETIME_CELL_BYTES > ffsa::RETIME_WORK_CAP) break;
        rows += c;
        ++np;
    }
    *rows_out = rows;
    return np;
}
}  // namespace

int ffs_cue_retime_batch(ffs_split_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                         const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                         const double* sub_lo, const double* sub_hi, const ffs_cue* cue_dev, int64_t n_cues,
                         const int64_t* cue_first, const int64_t* cue_count, int64_t radius_samples,
                         int64_t context_samples, int64_t penalty_q, int64_t jump_q, int flags, ffs_cue_retime* out_dev,
                         ffs_retime_summary* summary_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "split", n_pairs, a.any_null() || !cue_first || !cue_count); rc != CALL_GO_ON) return rc;
    if (int rc = check_cue_window(radius_samples, ffsa::RETIME_MAX_RADIUS, context_samples)) return rc;
    if (penalty_q < 0 || penalty_q > ffsa::RETIME_MAX_PENALTY_Q)
        return fail(FFS_E_INVALID, "penalty_q=%lld: need 0 <= penalty_q <= 2^20", (long long)penalty_q);
    if (jump_q < ffsa::RETIME_NO_JUMP || jump_q > ffsa::RETIME_MAX_JUMP_Q)
        return fail(FFS_E_INVALID, "jump_q=%lld: need -1 (no jump) or 0 <= jump_q <= 2^40", (long long)jump_q);
    if (flags & ~ffsa::RETIME_KEEP_ORDER) return fail(FFS_E_INVALID, "flags=%d: unknown bits", flags);
    if (int rc = check_cue_table_size(n_cues)) return rc;
    const int64_t n_delta = 2 * radius_samples + 1;
    int64_t total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = check_cue_pair(p, a, cue_first, cue_count, n_cues)) return rc;
        if (cue_count[p] * n_delta * ffsa::RETIME_CELL_BYTES > ffsa::RETIME_WORK_CAP)
            return fail(FFS_E_INVALID, "pair %d: %lld cues x %lld shifts x 6 bytes exceed the retime workspace cap of %lld bytes",
                        p, (long long)cue_count[p], (long long)n_delta, (long long)ffsa::RETIME_WORK_CAP);
        total += cue_count[p];
    }
    if (!summary_out_dev || ((uintptr_t)summary_out_dev & 7)) return fail(FFS_E_INVALID, "null or misaligned summary output");
    if (total > 0 && (!cue_dev || !out_dev || ((uintptr_t)cue_dev & 7) || ((uintptr_t)out_dev & 7)))
        return fail(FFS_E_INVALID, "null or misaligned cue table or retime output");
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    if (!plan->retime.dev)  // the first retime call: descriptors and their staging
        if (int rc = plan->add_staging(&plan->retime, sizeof(ffsa::RetimeDesc) * (size_t)pif, 0, "split plan: cue retime descriptors"))
            return rc;
    int64_t need = 0;  // the largest sub-batch's cells
    for (int p0 = 0; p0 < n_pairs;) {
        int64_t rows;
        p0 += retime_cut(cue_count, n_pairs, p0, pif, n_delta, &rows);
        need = std::max(need, split_align_up(rows * n_delta * ffsa::RETIME_CELL_BYTES, 256));
    }
    if (need > plan->retime_ws_bytes) {  // grow: no earlier call may still use the old block
        HIP_TRY(hipEventSynchronize(plan->done));
        plan->drop_block(plan->retime_ws, plan->retime_ws_bytes);
        plan->retime_ws = nullptr;
        plan->retime_ws_bytes = 0;
        if (int rc = plan->add_block(&plan->retime_ws, need, "split plan", "cue retime")) return rc;
        plan->retime_ws_bytes = need;
    }
    ffsa::RetimeDesc* hd = (ffsa::RetimeDesc*)plan->retime.host;
    const ffsa::RetimeDesc* dd = (const ffsa::RetimeDesc*)plan->retime.dev;
    const int n_rounds = (int)((n_delta + 63) / 64);
    for (int p0 = 0; p0 < n_pairs;) {
        int64_t rows;
        const int np = retime_cut(cue_count, n_pairs, p0, pif, n_delta, &rows);
        if (int rc = plan->retime.wait_free()) return rc;
        int64_t row = 0;
        for (int i = 0; i < np; ++i) {  // every pair gets a descriptor: one without cues still gets its summary
            const int p = p0 + i;
            ffsa::RetimeDesc& c = hd[i];
            c.r = (const uint32_t*)a.ref_ptr[p];
            c.s = (const uint32_t*)a.sub_ptr[p];
            c.R = ref_len[p];
            c.S = sub_len[p];
            c.cue_first = cue_first[p];
            c.cue_count = cue_count[p];
            c.grid_first = row * n_rounds;
            c.ws_first = row;
            c.out_row = p;
            row += cue_count[p];
        }
        if (int rc = plan->retime.upload(sizeof(ffsa::RetimeDesc) * np, st)) return rc;
        int32_t* prof = (int32_t*)plan->retime_ws;
        int16_t* bp = (int16_t*)((char*)plan->retime_ws + rows * n_delta * 4);
        if (rows > 0)
            hipLaunchKernelGGL(ffsa::k_retime_profile, dim3((unsigned)(rows * n_rounds)), dim3(ffsa::RETIME_PROFILE_THREADS),
                               0, st, dd, np, (const ffsa::Cue*)cue_dev, (int)radius_samples, (int)context_samples,
                               n_rounds, prof);
        hipLaunchKernelGGL(ffsa::k_retime_dp, dim3(np), dim3(ffsa::RETIME_DP_THREADS), 0, st, dd,
                           (const ffsa::Cue*)cue_dev, (int)radius_samples, penalty_q, jump_q, flags, (const int32_t*)prof, bp,
                           (ffsa::RetimeRec*)out_dev, (ffsa::RetimeSummary*)summary_out_dev);
        HIP_TRY(hipGetLastError());
        p0 += np;
    }
    return plan->end(st);
}

/* ---- split-aware alignment over a lag range (csrc/ffs_split_range.h) ------------------------------------------- */

namespace {
// What the split range plan and the drift range plan share: the DP's tables over up to max_lags lags, prefixes over whole
// vectors, SplitDesc and RangeLag rows.  `ws.stay` holds one bit plane per (block, lag) in the split range plan and
// drift_range_planes(max_step_cap) of them in the drift range plan, which also keeps two V rows.
struct RangePlan : PlanCore {
    int64_t max_blocks, max_lags, max_samples;
    int64_t pw, pre_slot;       // prefix words per vector and per slot
    ffsa::RangeWs ws;
    int32_t* pre;               // [slot][2 * pw]: s, then r
                                // desc: SplitDesc[pairs_in_flight], then RangeLag[pairs_in_flight]

    const ffsa::SplitDesc* dd() const { return (const ffsa::SplitDesc*)desc.dev; }
    const ffsa::RangeLag* dl() const { return (const ffsa::RangeLag*)(dd() + pairs_in_flight); }

    void carve(Carver& c) {
        const int64_t n = pairs_in_flight;
        ws.stay = c.take<unsigned long long>(n * ws.stay_slot);
        ws.V = c.take<double>(n * ws.v_slot);
        ws.pv = c.take<double>(n * 2 * ws.part_row);
        ws.pj = c.take<int32_t>(n * 2 * ws.part_row);
        ws.arg = c.take<int32_t>(n * ws.arg_slot);
        pre = c.take<int32_t>(n * pre_slot);
    }
};

// `more_need`: what the drift range plan's message adds about max_step_cap
int range_plan_dims_check(const char* what, const char* more_need, int pairs_in_flight, int64_t max_blocks, int64_t max_lags,
                          int64_t max_samples, int max_step_cap) {
    if (pairs_in_flight < 1 || pairs_in_flight > 65535 || max_blocks < 1 || max_lags < 1 || max_lags > INT32_MAX ||
        max_samples < 1 || max_samples > INT32_MAX / 2 || max_step_cap < 0 || max_step_cap > ffsa::DRIFT_RANGE_MAX_STEP)
        return fail(FFS_E_INVALID, "%s: need 1 <= pairs_in_flight <= 65535, max_blocks >= 1, "
                                   "1 <= max_lags <= 2^31 - 1, 1 <= max_samples <= 2^30 - 1%s", what, more_need);
    return FFS_OK;
}

// the sizes, the workspace and the descriptors of a new range plan of `planes` bit planes per (block, lag) and `v_rows`
// V rows; on failure the caller destroys the plan
int range_plan_open(RangePlan* p, const char* what, int planes, int v_rows, int device, int pairs_in_flight,
                    int64_t max_blocks, int64_t max_lags, int64_t max_samples) {
    p->pairs_in_flight = pairs_in_flight;
    p->max_blocks = max_blocks;
    p->max_lags = max_lags;
    p->max_samples = max_samples;
    p->pw = max_samples / 32 + 2;
    p->pre_slot = split_align_up(2 * p->pw, 64);                                                  // int32
    p->ws.stay_row = (max_lags + 63) / 64;  // 64-lag words per block row and plane
    p->ws.part_row = split_align_up((max_lags + ffsa::RANGE_TILE - 1) / ffsa::RANGE_TILE, 32);
    p->ws.stay_slot = split_align_up(max_blocks * p->ws.stay_row * planes, 32);                   // uint64
    p->ws.v_slot = v_rows * split_align_up(p->ws.stay_row * 64, 32);                              // double
    p->ws.arg_slot = split_align_up(max_blocks, 64);                                              // int32
    Carver size{nullptr};
    p->carve(size);
    if (int rc = p->open(device, pairs_in_flight, size.used, what)) return rc;
    Carver place{(char*)p->work};
    p->carve(place);
    if (p->desc.create((sizeof(ffsa::SplitDesc) + sizeof(ffsa::RangeLag)) * (size_t)pairs_in_flight) != FFS_OK)
        return fail(FFS_E_HIP, "%s: descriptor buffers / events", what);
    return FFS_OK;
}

// the per-pair checks of the range calls: lengths and blocks against the plan, the lag ranges; the largest block count
int range_limits_check(const RangePlan* plan, int n_pairs, const Pairs& a, int64_t K, const int64_t* lag_lo,
                       const int64_t* lag_hi, int64_t* max_b) {
    *max_b = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = a.check(p)) return rc;
        if (a.sub_len[p] > plan->max_samples || a.ref_len[p] > plan->max_samples)
            return fail(FFS_E_INVALID, "pair %d: lengths %lld / %lld exceed the plan's max_samples %lld", p,
                        (long long)a.ref_len[p], (long long)a.sub_len[p], (long long)plan->max_samples);
        if (int rc = check_blocks(p, a.sub_len[p], K, plan->max_blocks, max_b)) return rc;
        if (lag_lo[p] > lag_hi[p] || lag_lo[p] < -(int64_t)INT32_MAX || lag_hi[p] > INT32_MAX)
            return fail(FFS_E_INVALID, "pair %d: lag range [%lld, %lld]: need -(2^31 - 1) <= lag_lo <= lag_hi <= 2^31 - 1", p,
                        (long long)lag_lo[p], (long long)lag_hi[p]);
        if (lag_hi[p] - lag_lo[p] + 1 > plan->max_lags)
            return fail(FFS_E_INVALID, "pair %d: %lld lags exceed the plan's max_lags %lld", p,
                        (long long)(lag_hi[p] - lag_lo[p] + 1), (long long)plan->max_lags);
    }
    return FFS_OK;
}

struct RangeChunk {  // of one staged sub-batch: its largest block count, tile count and lag range
    int64_t chunk_b, max_tiles, max_l;
};

// the SplitDesc and RangeLag rows of the sub-batch [p0, p0 + np) filled and uploaded in one copy (the RangeLag half is at
// a fixed offset: the whole used span goes)
int range_stage(RangePlan* plan, const Pairs& a, const int64_t* lag_lo, const int64_t* lag_hi, int p0, int np, int64_t K,
                hipStream_t st, RangeChunk* chunk) {
    if (int rc = plan->desc.wait_free()) return rc;
    const int pif = plan->pairs_in_flight;
    ffsa::SplitDesc* hd = (ffsa::SplitDesc*)plan->desc.host;
    ffsa::RangeLag* hl = (ffsa::RangeLag*)(hd + pif);
    *chunk = RangeChunk{0, 0, 0};
    for (int i = 0; i < np; ++i) {
        const int p = p0 + i;
        int32_t* pre_s = plan->pre + (int64_t)i * plan->pre_slot;
        hd[i] = a.split_desc(p, pre_s, pre_s + plan->pw);
        hl[i].lag_lo = lag_lo[p];
        hl[i].L = lag_hi[p] - lag_lo[p] + 1;
        chunk->chunk_b = std::max(chunk->chunk_b, (hd[i].S + K - 1) / K);
        chunk->max_tiles = std::max(chunk->max_tiles, (hl[i].L + ffsa::RANGE_TILE - 1) / ffsa::RANGE_TILE);
        chunk->max_l = std::max(chunk->max_l, hl[i].L);
    }
    return plan->desc.upload(sizeof(ffsa::SplitDesc) * pif + sizeof(ffsa::RangeLag) * np, st);
}

// prefixes over every sample of both vectors of a staged sub-batch (W = max_samples: min(R, S + W) = R)
void range_prefixes(const RangePlan* plan, int np, hipStream_t st) {
    hipLaunchKernelGGL(ffsa::k_split_prefix, dim3(2 * np), dim3(ffsa::SPLIT_PREFIX_THREADS), 0, st, plan->dd(),
                       (int64_t)plan->max_samples);
}

// A solved path on the host for the two range reports: the block offsets, and with `jump_dev` the jump flags, copied
// behind the stream's earlier work, one synchronise, then every block's offset against its pair's lag range.
int read_path(const RangePlan* plan, int n_pairs, const Pairs& a, int64_t K, int64_t max_b, const int64_t* lag_lo,
              const int64_t* lag_hi, const int32_t* offset_dev, const uint8_t* jump_dev, std::vector<int32_t>* offs,
              std::vector<uint8_t>* jumps, hipStream_t st) {
    offs->resize((size_t)n_pairs * max_b);
    HIP_TRY(hipSetDevice(plan->device));
    HIP_TRY(hipMemcpyAsync(offs->data(), offset_dev, offs->size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (jump_dev) {
        jumps->resize((size_t)n_pairs * max_b);
        HIP_TRY(hipMemcpyAsync(jumps->data(), jump_dev, jumps->size(), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t B = (a.sub_len[p] + K - 1) / K;
        for (int64_t b = 0; b < B; ++b) {
            const int64_t o = (*offs)[(size_t)p * max_b + b];
            if (o < lag_lo[p] || o > lag_hi[p])
                return fail(FFS_E_INVALID, "pair %d: block %lld offset %lld outside the lag range [%lld, %lld]", p,
                            (long long)b, (long long)o, (long long)lag_lo[p], (long long)lag_hi[p]);
        }
    }
    return FFS_OK;
}
}  // namespace

struct ffs_split_range_plan : RangePlan {
    uint32_t* rows = nullptr;   // report calls only, made by the first: piece n11 rows, [slot][CUT_ROUND_PIECES][lpad]
    int64_t lpad;               // max_lags padded to 64
    DescStaging items;          // report calls only, made by the first: CutItem[item_cap]
    int64_t item_cap;
};

int ffs_split_range_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                                ffs_split_range_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (int rc = range_plan_dims_check("split range plan", "", pairs_in_flight, max_blocks, max_lags, max_samples, 0)) return rc;
    HIP_TRY(hipSetDevice(device));
    ffs_split_range_plan* p = new (std::nothrow) ffs_split_range_plan();
    if (!p) return fail(FFS_E_NOMEM, "split range plan");
    p->lpad = split_align_up(max_lags, 64);
    // a pair's report items over all its rounds: sum of ceil(piece words / CW) <= ceil(words / CW) + pieces
    constexpr int CW = ffsa::CUT_CHUNK_WORDS;
    p->item_cap = (int64_t)pairs_in_flight * ((max_samples / 32 + 1 + CW - 1) / CW + max_blocks);
    if (int rc = range_plan_open(p, "split range plan", 1, 1, device, pairs_in_flight, max_blocks, max_lags, max_samples)) {
        ffs_split_range_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FFS_OK;
}

int ffs_split_range_plan_destroy(ffs_split_range_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

int64_t ffs_split_range_plan_workspace_bytes(const ffs_split_range_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

int ffs_align_split_range_batch(ffs_split_range_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                const int64_t* lag_lo, const int64_t* lag_hi, double split_penalty,
                                int32_t* block_offset_out_dev, double* block_score_out_dev, double* total_out_dev,
                                void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "split range", n_pairs,
                            a.any_null() || !lag_lo || !lag_hi || !block_offset_out_dev || !block_score_out_dev || !total_out_dev);
        rc != CALL_GO_ON)
        return rc;
    if (((uintptr_t)block_offset_out_dev & 3) || ((uintptr_t)block_score_out_dev & 7) || ((uintptr_t)total_out_dev & 7))
        return fail(FFS_E_INVALID, "misaligned outputs");
    const int64_t K = block_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_split_penalty(split_penalty)) return rc;
    int64_t max_b = 0;
    if (int rc = range_limits_check(plan, n_pairs, a, K, lag_lo, lag_hi, &max_b)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    const ffsa::SplitDesc* dd = plan->dd();
    const ffsa::RangeLag* dl = plan->dl();
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        RangeChunk c;
        if (int rc = range_stage(plan, a, lag_lo, lag_hi, p0, np, K, st, &c)) return rc;
        range_prefixes(plan, np, st);
        for (int64_t b = 0; b < c.chunk_b; ++b)
            hipLaunchKernelGGL(ffsa::k_range_step, dim3((unsigned)c.max_tiles, (unsigned)np), dim3(ffsa::RANGE_THREADS), 0, st,
                               dd, dl, plan->ws, (int)K, b, split_penalty);
        hipLaunchKernelGGL(ffsa::k_range_backtrack, dim3(np), dim3(ffsa::RANGE_THREADS), 0, st, dd, dl, plan->ws, (int)K,
                           max_b, block_offset_out_dev, total_out_dev);
        constexpr int waves = ffsa::RANGE_SCORE_THREADS / 64;
        hipLaunchKernelGGL(ffsa::k_range_scores, dim3((unsigned)((max_b + waves - 1) / waves), (unsigned)np),
                           dim3(ffsa::RANGE_SCORE_THREADS), 0, st, dd, dl, (int)K, max_b, block_offset_out_dev,
                           block_score_out_dev);
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- per-piece report over a lag range (csrc/ffs_cut_report.h) ------------------------------------------------- */

int ffs_split_range_report_batch(ffs_split_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                 const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                 const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                 const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                 const int64_t* lag_hi, const int32_t* block_offset_dev, int top_k,
                                 int64_t exclusion_samples, ffs_piece_report* out_dev, int32_t* n_pieces_out_dev,
                                 void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "split range", n_pairs,
                            a.any_null() || !lag_lo || !lag_hi || !block_offset_dev || !out_dev || !n_pieces_out_dev);
        rc != CALL_GO_ON)
        return rc;
    if (((uintptr_t)block_offset_dev & 3) || ((uintptr_t)out_dev & 7) || ((uintptr_t)n_pieces_out_dev & 3))
        return fail(FFS_E_INVALID, "misaligned block offsets or report outputs");
    const int64_t K = block_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_peaks(top_k, exclusion_samples)) return rc;
    int64_t max_b = 0;
    if (int rc = range_limits_check(plan, n_pairs, a, K, lag_lo, lag_hi, &max_b)) return rc;
    // the block offsets on the host: the rounds' work items are made from their pieces
    hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int32_t> offs;
    if (int rc = read_path(plan, n_pairs, a, K, max_b, lag_lo, lag_hi, block_offset_dev, nullptr, &offs, nullptr, st)) return rc;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    constexpr int G = ffsa::CUT_ROUND_PIECES, CW = ffsa::CUT_CHUNK_WORDS;
    // the first report call: G n11 rows per pair in flight, and the work items of one sub-batch
    if (!plan->rows)
        if (int rc = plan->add_block((void**)&plan->rows, (int64_t)pif * G * plan->lpad * 4, "split range plan", "report"))
            return rc;
    if (!plan->items.dev)
        if (int rc = plan->add_staging(&plan->items, (size_t)plan->item_cap * sizeof(ffsa::CutItem), 0,
                                       "split range plan: report work items"))
            return rc;
    const ffsa::SplitDesc* dd = plan->dd();
    const ffsa::RangeLag* dl = plan->dl();
    ffsa::CutItem* hi_items = (ffsa::CutItem*)plan->items.host;
    const ffsa::CutItem* di_items = (const ffsa::CutItem*)plan->items.dev;
    std::vector<int64_t> round_start;  // per round: its first work item (+ the end)
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        RangeChunk c;
        if (int rc = range_stage(plan, a, lag_lo, lag_hi, p0, np, K, st, &c)) return rc;
        // the pieces of each pair (maximal runs of equal block offsets, as k_split_pieces forms them) -> work items,
        // round by round: round r holds the pieces r*G .. r*G + G - 1 of every pair
        std::vector<std::vector<int64_t>> starts(np);
        int64_t max_pieces = 0;
        for (int i = 0; i < np; ++i) {
            const int p = p0 + i;
            const int64_t B = (sub_len[p] + K - 1) / K;
            const int32_t* o = offs.data() + (size_t)p * max_b;
            for (int64_t b = 0; b < B; ++b)
                if (b == 0 || o[b] != o[b - 1]) starts[i].push_back(b);
            starts[i].push_back(B);
            max_pieces = std::max(max_pieces, (int64_t)starts[i].size() - 1);
        }
        const int64_t n_rounds = (max_pieces + G - 1) / G;
        if (int rc = plan->items.wait_free()) return rc;
        round_start.assign(1, 0);
        int64_t n_items = 0;
        for (int64_t r = 0; r < n_rounds; ++r) {
            for (int i = 0; i < np; ++i) {
                const int64_t S = sub_len[p0 + i];
                for (int g = 0; g < G; ++g) {
                    const int64_t k = r * G + g;
                    if (k + 1 >= (int64_t)starts[i].size()) break;
                    const int64_t w0 = starts[i][k] * K / 32, w1 = (std::min(starts[i][k + 1] * K, S) + 31) / 32;
                    for (int64_t c = w0; c < w1; c += CW) {
                        ffsa::CutItem& it = hi_items[n_items++];
                        it.g0 = c;
                        it.row = i * G + g;
                        it.nw = (int32_t)std::min<int64_t>(CW, w1 - c);
                    }
                }
            }
            round_start.push_back(n_items);
        }
        if (int rc = plan->items.upload(sizeof(ffsa::CutItem) * n_items, st)) return rc;
        range_prefixes(plan, np, st);
        hipLaunchKernelGGL(ffsa::k_split_pieces, dim3(np), dim3(ffsa::PIECE_SCAN_THREADS), 0, st, dd, (int)K, max_b,
                           block_offset_dev, (ffsa::PieceReport*)out_dev, n_pieces_out_dev);
        const int64_t n_tiles = (c.max_l + ffsa::QUAL_TILE - 1) / ffsa::QUAL_TILE;
        for (int64_t r = 0; r < n_rounds; ++r) {
            HIP_TRY(hipMemsetAsync(plan->rows, 0, (size_t)np * G * plan->lpad * 4, st));
            for (int64_t q = round_start[r]; q < round_start[r + 1]; q += ffsa::CUT_MAX_ITEMS) {
                const int64_t nq = std::min<int64_t>(ffsa::CUT_MAX_ITEMS, round_start[r + 1] - q);
                hipLaunchKernelGGL(ffsa::k_cut_piece_counts, dim3((unsigned)n_tiles, (unsigned)nq),
                                   dim3(ffsa::QUAL_CNT_THREADS), 0, st, dd, dl, di_items + q, plan->rows, plan->lpad);
            }
            hipLaunchKernelGGL(ffsa::k_cut_piece_report, dim3((unsigned)(np * G)), dim3(ffsa::QUAL_PEAK_THREADS), 0, st,
                               dd, dl, (const uint32_t*)plan->rows, plan->lpad, (int)(r * G), max_b, top_k,
                               exclusion_samples, (const int32_t*)n_pieces_out_dev, (ffsa::PieceReport*)out_dev);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- drift-tolerant alignment (csrc/ffs_drift.h) --------------------------------------------------------------- */

struct ffs_drift_plan : WindowPlan {
    double* rows = nullptr;      // report calls only, made by the first: [slot][DRIFT_ROUND_SEGMENTS][lpad] path curves
    void* smooth_mem = nullptr;  // smooth calls only, made by the first: the tables of ffsa::SmoothWs
    ffsa::SmoothWs sw;
};

int ffs_drift_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                          ffs_drift_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (int rc = window_plan_dims_check("drift plan", pairs_in_flight, max_blocks, max_lags, max_samples)) return rc;
    HIP_TRY(hipSetDevice(device));
    ffs_drift_plan* p = new (std::nothrow) ffs_drift_plan();
    if (!p) return fail(FFS_E_NOMEM, "drift plan");
    if (int rc = window_plan_open(p, "drift plan", true, device, pairs_in_flight, max_blocks, max_lags, max_samples)) {
        ffs_drift_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FFS_OK;
}

int ffs_drift_plan_destroy(ffs_drift_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

int64_t ffs_drift_plan_workspace_bytes(const ffs_drift_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

namespace {
struct DriftReportArgs {  // the per-segment report of ffs_align_drift_report_batch
    int top_k;
    int64_t exclusion;
    ffs_segment_report* out;
    int32_t* n_segments;
};

struct DriftSmoothArgs {  // the smooth fit of ffs_align_drift_smooth_batch
    int knot_blocks, radius;
    double bend_cost;
    int32_t* smooth_offset;
    uint8_t* knot;
    ffs_smooth_segment* out;
    int32_t* n_segments;
};

// The smooth workspace of a plan of `max_blocks` blocks, made by its first smooth call: line scores, back-pointers,
// segment / interval tables, and with `band` that many uint16 band cells behind them (the drift range plan's).
int smooth_workspace(PlanCore* plan, int64_t max_blocks, void** mem, ffsa::SmoothWs* sw, int64_t band_cells, uint16_t** band) {
    if (*mem) return FFS_OK;
    const int64_t n = plan->pairs_in_flight, mb = split_align_up(max_blocks, 16);
    auto carve = [&](Carver& c) {
        sw->T = c.take<double>(n * mb * ffsa::SMOOTH_MAX_STATES);
        sw->back = c.take<uint8_t>(n * mb * ffsa::SMOOTH_MAX_STATES, 64);
        sw->seg = c.take<ffsa::SmoothSeg>(n * mb);
        sw->iv = c.take<ffsa::SmoothInt>(n * mb);
        sw->seg_of = c.take<int32_t>(n * mb);
        sw->n_int = c.take<int32_t>(n, 64);
        if (band) *band = c.take<uint16_t>(band_cells);
    };
    Carver size{nullptr};
    carve(size);
    if (int rc = plan->add_block(mem, size.used, "drift plan", "smooth")) return rc;
    Carver place{(char*)*mem};
    carve(place);
    sw->stride = mb;
    return FFS_OK;
}

// the parameter and output checks of a smooth fit
int check_smooth_args(const DriftSmoothArgs& fit) {
    if (fit.knot_blocks < 1 || fit.knot_blocks > ffsa::SMOOTH_MAX_KNOT_BLOCKS)
        return fail(FFS_E_INVALID, "knot_blocks=%d outside [1, %d]", fit.knot_blocks, ffsa::SMOOTH_MAX_KNOT_BLOCKS);
    if (fit.radius < 0 || fit.radius > ffsa::SMOOTH_MAX_RADIUS)
        return fail(FFS_E_INVALID, "radius=%d outside [0, %d]", fit.radius, ffsa::SMOOTH_MAX_RADIUS);
    if (!(fit.bend_cost >= 0.0) || !std::isfinite(fit.bend_cost)) return fail(FFS_E_INVALID, "bend_cost must be finite and >= 0");
    if (!fit.smooth_offset || !fit.knot || !fit.out || !fit.n_segments) return fail(FFS_E_INVALID, "null argument");
    if (((uintptr_t)fit.smooth_offset & 3) || ((uintptr_t)fit.out & 7) || ((uintptr_t)fit.n_segments & 3))
        return fail(FFS_E_INVALID, "misaligned smooth outputs");
    return FFS_OK;
}

// ffs_align_drift_batch; with `rep` the segment reports, with `fit` the smooth fit after each sub-batch's DP
int drift_batch(ffs_drift_plan* plan, int n_pairs, const Pairs& a, int64_t block_samples, int64_t max_offset_samples,
                double split_penalty, int max_step, double step_cost, int32_t* block_offset_out_dev,
                double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev, const DriftReportArgs* rep,
                const DriftSmoothArgs* fit, void* hip_stream) {
    if (int rc = check_call(plan, "drift", n_pairs,
                            a.any_null() || !block_offset_out_dev || !block_score_out_dev || !block_jump_out_dev || !total_out_dev);
        rc != CALL_GO_ON)
        return rc;
    const int64_t K = block_samples, W = max_offset_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_window(W, plan->max_lags)) return rc;
    if (int rc = check_split_penalty(split_penalty)) return rc;
    if (int rc = check_step(max_step, ffsa::DRIFT_MAX_STEP, "", step_cost)) return rc;
    if (rep) {
        if (int rc = check_peaks(rep->top_k, rep->exclusion)) return rc;
        if (!rep->out || !rep->n_segments) return fail(FFS_E_INVALID, "null argument");
        if (((uintptr_t)rep->out & 7) || ((uintptr_t)rep->n_segments & 3)) return fail(FFS_E_INVALID, "misaligned report outputs");
    }
    if (fit)
        if (int rc = check_smooth_args(*fit)) return rc;
    int64_t max_b = 0;
    if (int rc = window_limits_check(plan, n_pairs, a, K, &max_b)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    if (fit)
        if (int rc = smooth_workspace(plan, plan->max_blocks, &plan->smooth_mem, &plan->sw, 0, nullptr)) return rc;
    constexpr int G = ffsa::DRIFT_ROUND_SEGMENTS;
    if (rep && !plan->rows)  // the first report call: G fp64 path-curve rows per slot
        if (int rc = plan->add_block((void**)&plan->rows, (int64_t)plan->pairs_in_flight * G * plan->lpad * 8, "drift plan",
                                     "report"))
            return rc;
    const int64_t L = 2 * W;
    const ffsa::SplitDesc* dd = (const ffsa::SplitDesc*)plan->desc.dev;
    std::vector<int32_t> n_seg;  // report calls: the sub-batch's segment counts, read back to size its rounds
    for (int p0 = 0; p0 < n_pairs; p0 += plan->pairs_in_flight) {
        const int np = std::min(plan->pairs_in_flight, n_pairs - p0);
        int64_t chunk_b = 0;
        if (int rc = window_stage(plan, a, p0, np, K, st, &chunk_b)) return rc;
        window_counts(plan, np, K, W, chunk_b, st);
        hipLaunchKernelGGL(ffsa::k_drift_dp, dim3(np), dim3(ffsa::SPLIT_DP_THREADS), 0, st, dd, plan->ws, plan->codes,
                           plan->codes_slot, (int)K, (int64_t)W, split_penalty, max_step, step_cost, max_b,
                           block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev);
        if (rep) {
            ffsa::SegmentReport* out = (ffsa::SegmentReport*)rep->out;
            hipLaunchKernelGGL(ffsa::k_drift_segments, dim3(np), dim3(ffsa::DRIFT_SEG_THREADS), 0, st, dd, (int)K, max_b,
                               (const int32_t*)block_offset_out_dev, (const uint8_t*)block_jump_out_dev, out,
                               rep->n_segments);
            HIP_TRY(hipGetLastError());
            // rounds of G segments per pair: as many as the sub-batch's largest segment count asks for
            n_seg.resize((size_t)np);
            HIP_TRY(hipMemcpyAsync(n_seg.data(), rep->n_segments + p0, sizeof(int32_t) * np, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int most = *std::max_element(n_seg.begin(), n_seg.end());
            const int n_sum_tiles = (int)((L + ffsa::DRIFT_SUM_TILE - 1) / ffsa::DRIFT_SUM_TILE);
            for (int first = 0; first < most; first += G) {
                hipLaunchKernelGGL(ffsa::k_drift_path_sums, dim3((unsigned)((int64_t)n_sum_tiles * G * np)),
                                   dim3(ffsa::DRIFT_SUM_THREADS), 0, st, dd, plan->ws, plan->rows, plan->lpad, (int)K,
                                   (int64_t)W, n_sum_tiles, first, max_b, (const int32_t*)block_offset_out_dev,
                                   (const int32_t*)rep->n_segments, (const ffsa::SegmentReport*)out);
                hipLaunchKernelGGL(ffsa::k_drift_segment_report, dim3((unsigned)(G * np)), dim3(ffsa::QUAL_PEAK_THREADS),
                                   0, st, dd, plan->ws, (const double*)plan->rows, plan->lpad, (int64_t)W, first, max_b,
                                   rep->top_k, rep->exclusion, (const int32_t*)rep->n_segments, out);
            }
        }
        if (fit) {
            ffsa::SmoothSegment* out = (ffsa::SmoothSegment*)fit->out;
            hipLaunchKernelGGL(ffsa::k_smooth_intervals, dim3(np), dim3(ffsa::SMOOTH_INT_THREADS), 0, st, dd, plan->sw, (int)K,
                               fit->knot_blocks, max_b, (const int32_t*)block_offset_out_dev,
                               (const uint8_t*)block_jump_out_dev, fit->smooth_offset, fit->knot, out, fit->n_segments);
            hipLaunchKernelGGL(ffsa::k_drift_line_sums, dim3((unsigned)(np * ffsa::SMOOTH_LINE_GROUPS)),
                               dim3(ffsa::SMOOTH_LINE_THREADS), 0, st, dd, plan->ws, plan->sw, (int)K, (int64_t)W, fit->radius,
                               max_b, (const int32_t*)block_offset_out_dev);
            hipLaunchKernelGGL(ffsa::k_drift_knot_dp, dim3((unsigned)(np * ffsa::SMOOTH_DP_GROUPS)),
                               dim3(ffsa::SMOOTH_DP_THREADS), 0, st, dd, plan->sw, fit->knot_blocks, fit->radius,
                               fit->bend_cost, max_b, (const int32_t*)block_offset_out_dev,
                               (const int32_t*)fit->n_segments, fit->smooth_offset, out);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}
}  // namespace

int ffs_align_drift_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                          const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                          const double* sub_lo, const double* sub_hi, int64_t block_samples, int64_t max_offset_samples,
                          double split_penalty, int max_step, double step_cost, int32_t* block_offset_out_dev,
                          double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                          void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    return drift_batch(plan, n_pairs, a, block_samples, max_offset_samples, split_penalty, max_step, step_cost,
                       block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev, nullptr, nullptr,
                       hip_stream);
}

int ffs_align_drift_report_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int max_step, double step_cost, int top_k,
                                 int64_t exclusion_samples, int32_t* block_offset_out_dev, double* block_score_out_dev,
                                 uint8_t* block_jump_out_dev, double* total_out_dev, ffs_segment_report* report_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    const DriftReportArgs rep{top_k, exclusion_samples, report_out_dev, n_segments_out_dev};
    return drift_batch(plan, n_pairs, a, block_samples, max_offset_samples, split_penalty, max_step, step_cost,
                       block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev, &rep, nullptr,
                       hip_stream);
}

int ffs_align_drift_smooth_batch(ffs_drift_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                 const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                 const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                 int64_t max_offset_samples, double split_penalty, int max_step, double step_cost,
                                 int knot_blocks, int radius, double bend_cost, int32_t* block_offset_out_dev,
                                 double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                                 int32_t* smooth_offset_out_dev, uint8_t* knot_out_dev, ffs_smooth_segment* segment_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    const DriftSmoothArgs fit{knot_blocks, radius, bend_cost, smooth_offset_out_dev, knot_out_dev, segment_out_dev,
                              n_segments_out_dev};
    return drift_batch(plan, n_pairs, a, block_samples, max_offset_samples, split_penalty, max_step, step_cost,
                       block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev, nullptr, &fit,
                       hip_stream);
}

/* ---- drift-tolerant alignment over a lag range (csrc/ffs_drift_range.h) ---------------------------------------- */

struct ffs_drift_range_plan : RangePlan {  // ws.stay = the code planes (max_step_cap's count), V = two rows per slot
    int max_step_cap;
    void* smooth_mem = nullptr;     // smooth calls only, made by the first: the tables of ffsa::SmoothWs, then the band rows
    ffsa::SmoothWs sw;
    uint16_t* band = nullptr;       // [slot][sw.stride][range_band_row(max_step_cap, 256, 16)]
    void* report_mem = nullptr;     // report calls only, made by the first: the fp64 score rows, then the uint32 n11 rows
    double* rep_scores = nullptr;   // [slot][RPATH_ROUND_SEGMENTS][rep_lpad]
    uint32_t* rep_rows = nullptr;   // [slot][RPATH_ROUND_SEGMENTS][rep_lpad]
    int64_t rep_lpad;               // max_lags + 1 cells, padded to 64
    DescStaging rep_items;          // report calls only, made by the first: RangePathItem[rep_item_cap]
    int64_t rep_item_cap;
};

int ffs_drift_range_plan_create(int device, int pairs_in_flight, int64_t max_blocks, int64_t max_lags, int64_t max_samples,
                                int max_step_cap, ffs_drift_range_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (int rc = range_plan_dims_check("drift range plan", ", 0 <= max_step_cap <= 7", pairs_in_flight, max_blocks, max_lags,
                                       max_samples, max_step_cap))
        return rc;
    HIP_TRY(hipSetDevice(device));
    ffs_drift_range_plan* p = new (std::nothrow) ffs_drift_range_plan();
    if (!p) return fail(FFS_E_NOMEM, "drift range plan");
    p->max_step_cap = max_step_cap;
    p->rep_lpad = split_align_up(max_lags + 1, 64);
    p->rep_item_cap = (int64_t)pairs_in_flight * ffsa::range_path_item_cap(max_samples, max_blocks);
    if (int rc = range_plan_open(p, "drift range plan", ffsa::drift_range_planes(max_step_cap), 2, device, pairs_in_flight,
                                 max_blocks, max_lags, max_samples)) {
        ffs_drift_range_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FFS_OK;
}

int ffs_drift_range_plan_destroy(ffs_drift_range_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

int64_t ffs_drift_range_plan_workspace_bytes(const ffs_drift_range_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

namespace {
// ffs_align_drift_range_batch; with `fit` the smooth fit after each sub-batch's scores
int drift_range_batch(ffs_drift_range_plan* plan, int n_pairs, const Pairs& a, int64_t block_samples, const int64_t* lag_lo,
                      const int64_t* lag_hi, double split_penalty, int max_step, double step_cost,
                      int32_t* block_offset_out_dev, double* block_score_out_dev, uint8_t* block_jump_out_dev,
                      double* total_out_dev, const DriftSmoothArgs* fit, void* hip_stream) {
    if (int rc = check_call(plan, "drift range", n_pairs,
                            a.any_null() || !lag_lo || !lag_hi || !block_offset_out_dev || !block_score_out_dev ||
                                !block_jump_out_dev || !total_out_dev);
        rc != CALL_GO_ON)
        return rc;
    if (((uintptr_t)block_offset_out_dev & 3) || ((uintptr_t)block_score_out_dev & 7) || ((uintptr_t)total_out_dev & 7))
        return fail(FFS_E_INVALID, "misaligned outputs");
    const int64_t K = block_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_split_penalty(split_penalty)) return rc;
    if (int rc = check_step(max_step, plan->max_step_cap, " (the plan's max_step_cap)", step_cost)) return rc;
    if (fit)
        if (int rc = check_smooth_args(*fit)) return rc;
    int64_t max_b = 0;
    if (int rc = range_limits_check(plan, n_pairs, a, K, lag_lo, lag_hi, &max_b)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    ffsa::RangeBand band{nullptr, 0};
    if (fit) {  // the first smooth call: the fit's tables and band rows wide enough for every later call
        const int64_t cap_row = ffsa::range_band_row(plan->max_step_cap, ffsa::SMOOTH_MAX_KNOT_BLOCKS, ffsa::SMOOTH_MAX_RADIUS);
        if (int rc = smooth_workspace(plan, plan->max_blocks, &plan->smooth_mem, &plan->sw,
                                      (int64_t)pif * split_align_up(plan->max_blocks, 16) * cap_row, &plan->band))
            return rc;
        band.cells = plan->band;
        band.row = ffsa::range_band_row(max_step, fit->knot_blocks, fit->radius);
    }
    const int planes = ffsa::drift_range_planes(max_step);
    const ffsa::SplitDesc* dd = plan->dd();
    const ffsa::RangeLag* dl = plan->dl();
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        RangeChunk c;
        if (int rc = range_stage(plan, a, lag_lo, lag_hi, p0, np, K, st, &c)) return rc;
        range_prefixes(plan, np, st);
        const int64_t chunk_b = c.chunk_b;
        for (int64_t b = 0; b < chunk_b; ++b)
            hipLaunchKernelGGL(ffsa::k_range_drift_step, dim3((unsigned)c.max_tiles, (unsigned)np), dim3(ffsa::RANGE_THREADS),
                               0, st, dd, dl, plan->ws, (int)K, b, split_penalty, max_step, step_cost, planes);
        hipLaunchKernelGGL(ffsa::k_range_drift_backtrack, dim3(np), dim3(ffsa::RANGE_THREADS), 0, st, dd, dl, plan->ws,
                           (int)K, max_b, max_step, planes, block_offset_out_dev, block_jump_out_dev, total_out_dev);
        constexpr int waves = ffsa::RANGE_SCORE_THREADS / 64;
        hipLaunchKernelGGL(ffsa::k_range_scores, dim3((unsigned)((max_b + waves - 1) / waves), (unsigned)np),
                           dim3(ffsa::RANGE_SCORE_THREADS), 0, st, dd, dl, (int)K, max_b, block_offset_out_dev,
                           block_score_out_dev);
        if (fit) {
            ffsa::SmoothSegment* out = (ffsa::SmoothSegment*)fit->out;
            hipLaunchKernelGGL(ffsa::k_smooth_intervals, dim3(np), dim3(ffsa::SMOOTH_INT_THREADS), 0, st, dd, plan->sw, (int)K,
                               fit->knot_blocks, max_b, (const int32_t*)block_offset_out_dev,
                               (const uint8_t*)block_jump_out_dev, fit->smooth_offset, fit->knot, out, fit->n_segments);
            hipLaunchKernelGGL(ffsa::k_range_band_counts, dim3((unsigned)chunk_b, (unsigned)np), dim3(ffsa::RBAND_THREADS), 0,
                               st, dd, plan->sw, band, (int)K, fit->knot_blocks, fit->radius, max_b,
                               (const int32_t*)block_offset_out_dev);
            hipLaunchKernelGGL(ffsa::k_range_line_sums, dim3((unsigned)(np * ffsa::SMOOTH_LINE_GROUPS)),
                               dim3(ffsa::SMOOTH_LINE_THREADS), 0, st, dd, dl, plan->sw, band, (int)K, fit->radius, max_b,
                               (const int32_t*)block_offset_out_dev);
            hipLaunchKernelGGL(ffsa::k_drift_knot_dp, dim3((unsigned)(np * ffsa::SMOOTH_DP_GROUPS)),
                               dim3(ffsa::SMOOTH_DP_THREADS), 0, st, dd, plan->sw, fit->knot_blocks, fit->radius,
                               fit->bend_cost, max_b, (const int32_t*)block_offset_out_dev,
                               (const int32_t*)fit->n_segments, fit->smooth_offset, out);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}
}  // namespace

int ffs_align_drift_range_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                                const double* ref_lo, const double* ref_hi, const void* const* sub_ptr,
                                const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int64_t block_samples,
                                const int64_t* lag_lo, const int64_t* lag_hi, double split_penalty, int max_step,
                                double step_cost, int32_t* block_offset_out_dev, double* block_score_out_dev,
                                uint8_t* block_jump_out_dev, double* total_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    return drift_range_batch(plan, n_pairs, a, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost,
                             block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev, nullptr,
                             hip_stream);
}

int ffs_align_drift_range_smooth_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                       const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                       const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                       const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                       const int64_t* lag_hi, double split_penalty, int max_step, double step_cost,
                                       int knot_blocks, int radius, double bend_cost, int32_t* block_offset_out_dev,
                                       double* block_score_out_dev, uint8_t* block_jump_out_dev, double* total_out_dev,
                                       int32_t* smooth_offset_out_dev, uint8_t* knot_out_dev,
                                       ffs_smooth_segment* segment_out_dev, int32_t* n_segments_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    const DriftSmoothArgs fit{knot_blocks, radius, bend_cost, smooth_offset_out_dev, knot_out_dev, segment_out_dev,
                              n_segments_out_dev};
    return drift_range_batch(plan, n_pairs, a, block_samples, lag_lo, lag_hi, split_penalty, max_step, step_cost,
                             block_offset_out_dev, block_score_out_dev, block_jump_out_dev, total_out_dev, &fit,
                             hip_stream);
}

/* ---- per-segment path report over a lag range (csrc/ffs_drift_range_report.h) ---------------------------------- */

int ffs_drift_range_report_batch(ffs_drift_range_plan* plan, int n_pairs, const void* const* ref_ptr,
                                 const int64_t* ref_len, const double* ref_lo, const double* ref_hi,
                                 const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo,
                                 const double* sub_hi, int64_t block_samples, const int64_t* lag_lo,
                                 const int64_t* lag_hi, const int32_t* block_offset_dev, const uint8_t* block_jump_dev,
                                 int top_k, int64_t exclusion_samples, ffs_segment_report* report_out_dev,
                                 int32_t* n_segments_out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "drift range", n_pairs,
                            a.any_null() || !lag_lo || !lag_hi || !block_offset_dev || !block_jump_dev || !report_out_dev ||
                                !n_segments_out_dev);
        rc != CALL_GO_ON)
        return rc;
    if (((uintptr_t)block_offset_dev & 3) || ((uintptr_t)report_out_dev & 7) || ((uintptr_t)n_segments_out_dev & 3))
        return fail(FFS_E_INVALID, "misaligned block offsets or report outputs");
    const int64_t K = block_samples;
    if (int rc = check_block_samples(K)) return rc;
    if (int rc = check_peaks(top_k, exclusion_samples)) return rc;
    int64_t max_b = 0;
    if (int rc = range_limits_check(plan, n_pairs, a, K, lag_lo, lag_hi, &max_b)) return rc;
    // the path on the host: the rounds' work items are made from its segments and their runs
    hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int32_t> offs;
    std::vector<uint8_t> jumps;
    if (int rc = read_path(plan, n_pairs, a, K, max_b, lag_lo, lag_hi, block_offset_dev, block_jump_dev, &offs, &jumps, st))
        return rc;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    constexpr int G = ffsa::RPATH_ROUND_SEGMENTS;
    const int64_t lpad = plan->rep_lpad;
    // the first report call: G score and n11 rows per pair in flight, one sub-batch's items
    if (!plan->report_mem) {
        auto carve = [&](Carver& c) {
            plan->rep_scores = c.take<double>((int64_t)pif * G * lpad);
            plan->rep_rows = c.take<uint32_t>((int64_t)pif * G * lpad);
        };
        Carver size{nullptr};
        carve(size);
        if (int rc = plan->add_block(&plan->report_mem, size.used, "drift range plan", "report")) return rc;
        Carver place{(char*)plan->report_mem};
        carve(place);
    }
    if (!plan->rep_items.dev)
        if (int rc = plan->add_staging(&plan->rep_items, (size_t)plan->rep_item_cap * sizeof(ffsa::RangePathItem), 0,
                                       "drift range plan: report work items"))
            return rc;
    const ffsa::SplitDesc* dd = plan->dd();
    const ffsa::RangeLag* dl = plan->dl();
    const ffsa::RangePathItem* di_items = (const ffsa::RangePathItem*)plan->rep_items.dev;
    ffsa::SegmentReport* out = (ffsa::SegmentReport*)report_out_dev;
    std::vector<std::vector<ffsa::RangePathSegment>> segs;
    std::vector<ffsa::RangePathItem> items;
    std::vector<int64_t> round_start;  // per round: its first work item (+ the end)
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        RangeChunk c;
        if (int rc = range_stage(plan, a, lag_lo, lag_hi, p0, np, K, st, &c)) return rc;
        // the segments of each pair (as k_drift_segments forms them) -> work items, round by round: round r holds the
        // segments r*G .. r*G + G - 1 of every pair
        segs.resize((size_t)np);
        int64_t most = 0;
        for (int i = 0; i < np; ++i) {
            const int p = p0 + i;
            ffsa::range_path_segments(offs.data() + (size_t)p * max_b, jumps.data() + (size_t)p * max_b,
                                      (sub_len[p] + K - 1) / K, segs[i]);
            most = std::max(most, (int64_t)segs[i].size());
        }
        const int64_t n_rounds = (most + G - 1) / G;
        items.clear();
        round_start.assign(1, 0);
        for (int64_t r = 0; r < n_rounds; ++r) {
            for (int i = 0; i < np; ++i) {
                const int p = p0 + i;
                for (int g = 0; g < G && r * G + g < (int64_t)segs[i].size(); ++g)
                    ffsa::range_path_items(offs.data() + (size_t)p * max_b, segs[i][(size_t)(r * G + g)], K, sub_len[p],
                                           lag_lo[p], lag_hi[p] - lag_lo[p] + 1, i * G + g, items);
            }
            round_start.push_back((int64_t)items.size());
        }
        if ((int64_t)items.size() > plan->rep_item_cap)
            return fail(FFS_E_INVALID, "drift range report: %lld work items exceed the table of %lld",
                        (long long)items.size(), (long long)plan->rep_item_cap);
        if (int rc = plan->rep_items.wait_free()) return rc;
        memcpy(plan->rep_items.host, items.data(), items.size() * sizeof(ffsa::RangePathItem));
        if (int rc = plan->rep_items.upload(sizeof(ffsa::RangePathItem) * items.size(), st)) return rc;
        range_prefixes(plan, np, st);
        hipLaunchKernelGGL(ffsa::k_drift_segments, dim3(np), dim3(ffsa::DRIFT_SEG_THREADS), 0, st, dd, (int)K, max_b,
                           block_offset_dev, block_jump_dev, out, n_segments_out_dev);
        const int64_t n_tiles = (c.max_l + ffsa::QUAL_TILE - 1) / ffsa::QUAL_TILE;
        const int n_sum_tiles = (int)((c.max_l + ffsa::DRIFT_SUM_TILE - 1) / ffsa::DRIFT_SUM_TILE);
        for (int64_t r = 0; r < n_rounds; ++r) {
            HIP_TRY(hipMemsetAsync(plan->rep_rows, 0, (size_t)np * G * lpad * 4, st));
            for (int64_t q = round_start[r]; q < round_start[r + 1]; q += ffsa::RPATH_MAX_ITEMS) {
                const int64_t nq = std::min<int64_t>(ffsa::RPATH_MAX_ITEMS, round_start[r + 1] - q);
                hipLaunchKernelGGL(ffsa::k_range_path_counts, dim3((unsigned)n_tiles, (unsigned)nq),
                                   dim3(ffsa::QUAL_CNT_THREADS), 0, st, dd, di_items + q, plan->rep_rows, lpad);
            }
            hipLaunchKernelGGL(ffsa::k_range_path_scores, dim3((unsigned)((int64_t)n_sum_tiles * G * np)),
                               dim3(ffsa::DRIFT_SUM_THREADS), 0, st, dd, dl, (const uint32_t*)plan->rep_rows,
                               plan->rep_scores, lpad, (int)K, n_sum_tiles, (int)(r * G), max_b, block_offset_dev,
                               (const int32_t*)n_segments_out_dev, (const ffsa::SegmentReport*)out);
            hipLaunchKernelGGL(ffsa::k_range_segment_report, dim3((unsigned)(np * G)), dim3(ffsa::QUAL_PEAK_THREADS), 0, st,
                               dd, dl, (const uint32_t*)plan->rep_rows, (const double*)plan->rep_scores, lpad,
                               (int)(r * G), max_b, top_k, exclusion_samples, (const int32_t*)n_segments_out_dev, out);
        }
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- alignment quality report (csrc/ffs_quality.h) ------------------------------------------------------------- */

namespace {
// the window, the peak parameters and the output records of the quality and the match calls
int check_quality_args(int64_t max_offset_samples, int top_k, int64_t exclusion_samples, const void* out_dev) {
    if (max_offset_samples < -1) return fail(FFS_E_INVALID, "max_offset_samples=%lld: need >= 0, or -1 for none", (long long)max_offset_samples);
    if (int rc = check_peaks(top_k, exclusion_samples)) return rc;
    if ((uintptr_t)out_dev & 7) return fail(FFS_E_INVALID, "misaligned output records");
    return FFS_OK;
}

// pair p's lag window (R and S samples, max_offset_samples) against the plan's lags
int check_window_lags(int p, int64_t R, int64_t S, int64_t max_offset_samples, int64_t plan_max_lags) {
    int64_t wl = 0, wh = -1;
    if (lag_window(R, S, ffs_fft_length(R, S), max_offset_samples, &wl, &wh) && wh - wl + 1 > plan_max_lags)
        return fail(FFS_E_INVALID, "pair %d: %lld lags exceed the plan's max_lags %lld", p, (long long)(wh - wl + 1),
                    (long long)plan_max_lags);
    return FFS_OK;
}

// the lengths of a pair and its lag window in its (zeroed) descriptor: the window's lags, and of them those with an overlap
void qual_window(ffsa::QualDesc* q, int64_t R, int64_t S, int64_t max_offset_samples) {
    q->R = R;
    q->S = S;
    int64_t wl = 0, wh = -1;
    if (lag_window(R, S, ffs_fft_length(R, S), max_offset_samples, &wl, &wh)) {
        q->d_lo = wl;
        q->n_lags = wh - wl + 1;
        const int64_t clo = std::max(wl, 1 - S), chi = std::min(wh, R - 1);
        q->c_lo = clo;
        q->n_count = chi >= clo ? chi - clo + 1 : 0;
    }
    q->cd.R = (int32_t)R;
    q->cd.S = (int32_t)S;
}

// k_quality_counts over n descriptors of at most max_count counted lags and max_sw subtitle words, in chunks of subtitle
// words: enough workgroups to fill the device (about 4 per CU), at least 64 words each so that the atomics stay a small
// fraction of the work, at most QUAL_MAX_CHUNK (LDS)
void quality_counts(const ffsa::QualDesc* dq, int n, int64_t max_count, int64_t max_sw, int n_sm, hipStream_t st) {
    const int64_t n_tiles = (max_count + ffsa::QUAL_TILE - 1) / ffsa::QUAL_TILE;
    const int64_t want = std::max<int64_t>(1, (int64_t)n_sm * 4);
    int64_t cw = (n * n_tiles * max_sw + want - 1) / want;
    cw = std::min<int64_t>(ffsa::QUAL_MAX_CHUNK, std::max<int64_t>(64, cw));
    const int64_t n_chunks = (max_sw + cw - 1) / cw;
    hipLaunchKernelGGL(ffsa::k_quality_counts, dim3((unsigned)(n * n_tiles * n_chunks)), dim3(ffsa::QUAL_CNT_THREADS), 0, st, dq,
                       (int)n_tiles, (int)n_chunks, (int)cw);
}
}  // namespace

struct ffs_quality_plan : PlanCore {
    int64_t max_lags, max_samples;
    int64_t lpad, pre_slot;     // padded curve row, prefix words per slot (both vectors)
    uint32_t* curve;            // [slot][lpad]
    double* sc;                 // [slot][lpad]
    int32_t* pre;               // [slot][pre_slot]
                                // desc: SplitDesc[pairs_in_flight] (k_split_prefix), then QualDesc[pairs_in_flight]

    void carve(Carver& c) {
        const int64_t n = pairs_in_flight;
        sc = c.take<double>(n * lpad);
        curve = c.take<uint32_t>(n * lpad);
        pre = c.take<int32_t>(n * pre_slot);
    }
};

int ffs_quality_plan_create(int device, int pairs_in_flight, int64_t max_lags, int64_t max_samples, ffs_quality_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (pairs_in_flight < 1 || max_lags < 1 || max_lags > (int64_t(1) << 31) || max_samples < 1 || max_samples >= (int64_t(1) << 30))
        return fail(FFS_E_INVALID, "quality plan: need pairs_in_flight >= 1, 1 <= max_lags <= 2^31, 1 <= max_samples < 2^30");
    HIP_TRY(hipSetDevice(device));
    ffs_quality_plan* p = new (std::nothrow) ffs_quality_plan();
    if (!p) return fail(FFS_E_NOMEM, "quality plan");
    p->max_lags = max_lags;
    p->max_samples = max_samples;
    p->lpad = split_align_up(max_lags, 64);
    p->pre_slot = split_align_up(2 * (max_samples / 32 + 2), 64);
    p->pairs_in_flight = pairs_in_flight;
    Carver size{nullptr};
    p->carve(size);
    if (int rc = p->open(device, pairs_in_flight, size.used, "quality plan")) {
        ffs_quality_plan_destroy(p);
        return rc;
    }
    Carver place{(char*)p->work};
    p->carve(place);
    if (p->desc.create((sizeof(ffsa::SplitDesc) + sizeof(ffsa::QualDesc)) * (size_t)pairs_in_flight) != FFS_OK) {
        ffs_quality_plan_destroy(p);
        return fail(FFS_E_HIP, "quality plan: descriptor buffers / events");
    }
    *out = p;
    return FFS_OK;
}

int ffs_quality_plan_destroy(ffs_quality_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

int64_t ffs_quality_plan_workspace_bytes(const ffs_quality_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

int ffs_align_quality_batch(ffs_quality_plan* plan, int n_pairs, const void* const* ref_ptr, const int64_t* ref_len,
                            const double* ref_lo, const double* ref_hi, const void* const* sub_ptr, const int64_t* sub_len,
                            const double* sub_lo, const double* sub_hi, int64_t max_offset_samples, int top_k,
                            int64_t exclusion_samples, ffs_quality_result* out_dev, void* hip_stream) {
    const Pairs a{ref_ptr, ref_len, ref_lo, ref_hi, sub_ptr, sub_len, sub_lo, sub_hi};
    if (int rc = check_call(plan, "quality", n_pairs, a.any_null() || !out_dev); rc != CALL_GO_ON) return rc;
    if (int rc = check_quality_args(max_offset_samples, top_k, exclusion_samples, out_dev)) return rc;
    int64_t max_sw = 0;
    for (int p = 0; p < n_pairs; ++p) {
        if (int rc = a.check(p)) return rc;
        if (ref_len[p] > plan->max_samples || sub_len[p] > plan->max_samples)
            return fail(FFS_E_INVALID, "pair %d: lengths %lld / %lld exceed the plan's max_samples %lld", p,
                        (long long)ref_len[p], (long long)sub_len[p], (long long)plan->max_samples);
        if (int rc = check_window_lags(p, ref_len[p], sub_len[p], max_offset_samples, plan->max_lags)) return rc;
        max_sw = std::max(max_sw, (sub_len[p] + 31) / 32);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    const int pif = plan->pairs_in_flight;
    ffsa::SplitDesc* hs = (ffsa::SplitDesc*)plan->desc.host;
    ffsa::QualDesc* hq = (ffsa::QualDesc*)(hs + pif);
    const ffsa::SplitDesc* ds = (const ffsa::SplitDesc*)plan->desc.dev;
    const ffsa::QualDesc* dq = (const ffsa::QualDesc*)(ds + pif);
    int n_sm = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_sm, hipDeviceAttributeMultiprocessorCount, plan->device));
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        if (int rc = plan->desc.wait_free()) return rc;
        int64_t max_count = 0;
        for (int i = 0; i < np; ++i) {
            const int p = p0 + i;
            const int64_t R = ref_len[p], S = sub_len[p];
            int32_t* pre_s = plan->pre + (int64_t)i * plan->pre_slot;
            ffsa::SplitDesc& sd = hs[i];
            sd = a.split_desc(p, pre_s, pre_s + (S / 32 + 2));
            const Levels v = a.levels(p);
            ffsa::QualDesc& q = hq[i];
            memset(&q, 0, sizeof q);
            q.r = sd.r;
            q.s = sd.s;
            qual_window(&q, R, S, max_offset_samples);
            q.cd.s0 = v.s0;
            q.cd.s1 = v.s1;
            q.cd.r0 = v.r0;
            q.cd.r1 = v.r1;
            q.pre_r = sd.pre_r;
            q.pre_s = sd.pre_s;
            q.curve = plan->curve + (int64_t)i * plan->lpad;
            q.sc = plan->sc + (int64_t)i * plan->lpad;
            q.out_row = p;
            max_count = std::max(max_count, q.n_count);
        }
        // one upload of both arrays (the QualDesc half is at a fixed offset: copy the whole used span)
        if (int rc = plan->desc.upload(sizeof(ffsa::SplitDesc) * pif + sizeof(ffsa::QualDesc) * np, st)) return rc;
        HIP_TRY(hipMemsetAsync(plan->curve, 0, (size_t)np * plan->lpad * 4, st));
        // prefixes over every sample of both vectors (W beyond any length: k_split_prefix then covers all of r)
        hipLaunchKernelGGL(ffsa::k_split_prefix, dim3(2 * np), dim3(ffsa::SPLIT_PREFIX_THREADS), 0, st, ds,
                           (int64_t)(int64_t(1) << 40));
        if (max_count > 0) quality_counts(dq, np, max_count, max_sw, n_sm, st);
        hipLaunchKernelGGL(ffsa::k_quality_peaks, dim3(np), dim3(ffsa::QUAL_PEAK_THREADS), 0, st, dq, top_k,
                           exclusion_samples, (ffsa::QualResult*)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- all-pairs quality report from boundary lists (csrc/ffs_match.h) ------------------------------------------- */

struct ffs_match_plan : PlanCore {
    int64_t max_lags, max_samples, max_vectors;
    int64_t lpad, vec_words, pre_words;  // padded curve row; bit words / prefix words per vector slot
    uint32_t* curve;                     // [slot][lpad]
    double* sc;                          // [slot][lpad]
    uint32_t* bits;                      // [vector][vec_words]
    int32_t* pre;                        // [vector][pre_words]
    ffsa::MatchHdr* hdr_dev;             // [vector]
    ffsa::MatchHdr* hdr_host;            // pinned
    DescStaging vec;                     // per call: list pointers, ExpandVec and SplitDesc tables of the vectors
                                         // desc: QualDesc[pairs_in_flight], then MatchLists[pairs_in_flight]
    size_t off_expand, off_split, vec_bytes;

    void carve(Carver& c) {
        const int64_t n = pairs_in_flight, nv = max_vectors;
        sc = c.take<double>(n * lpad);
        curve = c.take<uint32_t>(n * lpad);
        bits = c.take<uint32_t>(nv * vec_words);
        pre = c.take<int32_t>(nv * pre_words);
        hdr_dev = c.take<ffsa::MatchHdr>(nv, 64);
    }
};

int ffs_match_plan_create(int device, int pairs_in_flight, int64_t max_lags, int64_t max_samples, int64_t max_vectors,
                          ffs_match_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (pairs_in_flight < 1 || max_lags < 1 || max_lags > (int64_t(1) << 31) || max_samples < 1 ||
        max_samples >= (int64_t(1) << 29) || max_vectors < 2 || max_vectors > (int64_t(1) << 24))
        return fail(FFS_E_INVALID, "match plan: need pairs_in_flight >= 1, 1 <= max_lags <= 2^31, 1 <= max_samples < 2^29, "
                                   "2 <= max_vectors <= 2^24");
    HIP_TRY(hipSetDevice(device));
    ffs_match_plan* p = new (std::nothrow) ffs_match_plan();
    if (!p) return fail(FFS_E_NOMEM, "match plan");
    p->max_lags = max_lags;
    p->max_samples = max_samples;
    p->max_vectors = max_vectors;
    p->lpad = split_align_up(max_lags, 64);
    p->vec_words = split_align_up(max_samples / 32 + 1, 16);
    p->pre_words = split_align_up(max_samples / 32 + 2, 16);
    const int64_t nv = max_vectors;
    p->pairs_in_flight = pairs_in_flight;
    Carver size{nullptr};
    p->carve(size);
    if (int rc = p->open(device, pairs_in_flight, size.used, "match plan")) {
        ffs_match_plan_destroy(p);
        return rc;
    }
    Carver place{(char*)p->work};
    p->carve(place);
    p->off_expand = (size_t)split_align_up(nv * 8, 64);
    p->off_split = p->off_expand + (size_t)split_align_up(nv * (int64_t)sizeof(ExpandVec), 64);
    p->vec_bytes = p->off_split + sizeof(ffsa::SplitDesc) * (size_t)((nv + 1) / 2);
    if (hipHostMalloc((void**)&p->hdr_host, (size_t)nv * sizeof(ffsa::MatchHdr), hipHostMallocDefault) != hipSuccess) {
        p->hdr_host = nullptr;
        ffs_match_plan_destroy(p);
        return fail(FFS_E_HIP, "match plan: header staging");
    }
    if (p->vec.create(p->vec_bytes) != FFS_OK ||
        p->desc.create((sizeof(ffsa::QualDesc) + sizeof(ffsa::MatchLists)) * (size_t)pairs_in_flight) != FFS_OK) {
        ffs_match_plan_destroy(p);
        return fail(FFS_E_HIP, "match plan: descriptor buffers / events");
    }
    *out = p;
    return FFS_OK;
}

int ffs_match_plan_destroy(ffs_match_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    plan->vec.release();
    if (plan->hdr_host) (void)hipHostFree(plan->hdr_host);
    delete plan;
    return FFS_OK;
}

int64_t ffs_match_plan_workspace_bytes(const ffs_match_plan* plan) { return plan ? plan->workspace_bytes() : 0; }

int ffs_match_quality_batch(ffs_match_plan* plan, int n_ref, const void* const* ref_list, const int64_t* ref_len,
                            const double* ref_lo, const double* ref_hi, int n_sub, const void* const* sub_list,
                            const int64_t* sub_len, const double* sub_lo, const double* sub_hi, int n_pairs,
                            const int32_t* pair_ref, const int32_t* pair_sub, int64_t max_offset_samples, int top_k,
                            int64_t exclusion_samples, int algorithm, ffs_quality_result* out_dev, void* hip_stream) {
    if (!plan) return fail(FFS_E_INVALID, "null match plan");
    if (n_pairs < 0 || n_ref < 0 || n_sub < 0) return fail(FFS_E_INVALID, "n_pairs / n_ref / n_sub < 0");
    if (n_pairs == 0) return FFS_OK;
    if (!ref_list || !ref_len || !ref_lo || !ref_hi || !sub_list || !sub_len || !sub_lo || !sub_hi || !pair_ref || !pair_sub ||
        !out_dev)
        return fail(FFS_E_INVALID, "null argument");
    if (int rc = check_quality_args(max_offset_samples, top_k, exclusion_samples, out_dev)) return rc;
    if (algorithm != FFS_MATCH_AUTO && algorithm != FFS_MATCH_RUNS && algorithm != FFS_MATCH_BITS)
        return fail(FFS_E_INVALID, "algorithm=%d: need FFS_MATCH_AUTO, FFS_MATCH_RUNS or FFS_MATCH_BITS", algorithm);
    const int64_t nv = (int64_t)n_ref + n_sub;
    if (nv > plan->max_vectors)
        return fail(FFS_E_INVALID, "%d references + %d subtitle vectors exceed the plan's max_vectors %lld", n_ref, n_sub,
                    (long long)plan->max_vectors);
    // vector v < n_ref: reference v; else subtitle vector v - n_ref
    auto v_list = [&](int64_t v) { return v < n_ref ? ref_list[v] : sub_list[v - n_ref]; };
    auto v_len = [&](int64_t v) { return v < n_ref ? ref_len[v] : sub_len[v - n_ref]; };
    for (int64_t v = 0; v < nv; ++v) {
        const bool is_ref = v < n_ref;
        const int64_t i = is_ref ? v : v - n_ref;
        const char* role = is_ref ? "reference" : "subtitle vector";
        if (v_len(v) <= 0)
            return fail(FFS_E_EMPTY, "cannot align empty speech data (%s %lld has length %lld)", role, (long long)i,
                        (long long)(v_len(v) > 0 ? v_len(v) : 0));
        if (!v_list(v) || ((uintptr_t)v_list(v) & 7)) return fail(FFS_E_INVALID, "%s %lld: null or misaligned list block", role, (long long)i);
        if (v_len(v) > plan->max_samples)
            return fail(FFS_E_INVALID, "%s %lld: %lld samples exceed the plan's max_samples %lld", role, (long long)i,
                        (long long)v_len(v), (long long)plan->max_samples);
        const double lo = is_ref ? ref_lo[i] : sub_lo[i], hi = is_ref ? ref_hi[i] : sub_hi[i];
        if (!(std::isfinite(lo) && std::isfinite(hi))) return fail(FFS_E_INVALID, "%s %lld: levels must be finite", role, (long long)i);
    }
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_ref[p] < 0 || pair_ref[p] >= n_ref || pair_sub[p] < 0 || pair_sub[p] >= n_sub)
            return fail(FFS_E_INVALID, "pair %d: index (%d, %d) outside the %d references x %d subtitle vectors", p,
                        (int)pair_ref[p], (int)pair_sub[p], n_ref, n_sub);
        if (int rc = check_window_lags(p, ref_len[pair_ref[p]], sub_len[pair_sub[p]], max_offset_samples, plan->max_lags))
            return rc;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    // the lists' headers (the one device step in front of the checks: it writes the plan's workspace only)
    if (int rc = plan->vec.wait_free()) return rc;
    char* hv = (char*)plan->vec.host;
    const char* dv = (const char*)plan->vec.dev;
    const void** h_ptr = (const void**)hv;
    ExpandVec* h_ev = (ExpandVec*)(hv + plan->off_expand);
    ffsa::SplitDesc* h_sd = (ffsa::SplitDesc*)(hv + plan->off_split);
    memset(h_sd, 0, sizeof(ffsa::SplitDesc) * (size_t)((nv + 1) / 2));
    for (int64_t v = 0; v < nv; ++v) {
        const char* blk = (const char*)v_list(v);
        uint32_t* bits = plan->bits + v * plan->vec_words;
        int32_t* pre = plan->pre + v * plan->pre_words;
        h_ptr[v] = blk;
        h_ev[v] = ExpandVec{(const int2*)(blk + 16), (const int2*)blk, (unsigned*)bits, (int32_t)v_len(v), 0};
        ffsa::SplitDesc& sd = h_sd[v >> 1];  // two vectors per descriptor: the even one as its `s`, the odd one as its `r`
        if (v & 1) {
            sd.r = bits;
            sd.R = v_len(v);
            sd.pre_r = pre;
        } else {
            sd.s = bits;
            sd.S = v_len(v);
            sd.pre_s = pre;
        }
    }
    if (int rc = plan->vec.upload(plan->vec_bytes, st)) return rc;
    hipLaunchKernelGGL(ffsa::k_match_headers, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, (const int2* const*)dv,
                       (int)nv, plan->hdr_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(plan->hdr_host, plan->hdr_dev, (size_t)nv * sizeof(ffsa::MatchHdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const ffsa::MatchHdr* hd = plan->hdr_host;
    for (int64_t v = 0; v < nv; ++v) {
        const bool is_ref = v < n_ref;
        const long long i = is_ref ? v : v - n_ref;
        const char* role = is_ref ? "reference" : "subtitle vector";
        if (hd[v].n >= hd[v].cap)
            return fail(FFS_E_INVALID, "%s %lld: truncated boundary list (%d boundaries, capacity %d)", role, i, hd[v].n, hd[v].cap);
        if (hd[v].n < 0 || (hd[v].n & 1) || hd[v].len != v_len(v))
            return fail(FFS_E_INVALID, "%s %lld: not the boundary list of a vector of %lld samples (n=%d, len=%d)", role, i,
                        (long long)v_len(v), hd[v].n, hd[v].len);
    }
    // per vector, once: bits and word prefixes in the workspace
    int64_t max_len = 0;
    for (int64_t v = 0; v < nv; ++v) max_len = std::max(max_len, v_len(v));
    const int chunks_per_vec = (int)(((max_len + 31) / 32 + 255) / 256);
    hipLaunchKernelGGL(k_runs_expand, dim3((unsigned)(nv * chunks_per_vec)), dim3(256), 0, st,
                       (const ExpandVec*)(dv + plan->off_expand), chunks_per_vec, (int*)nullptr);
    hipLaunchKernelGGL(ffsa::k_split_prefix, dim3((unsigned)nv), dim3(ffsa::SPLIT_PREFIX_THREADS), 0, st,
                       (const ffsa::SplitDesc*)(dv + plan->off_split), (int64_t)(int64_t(1) << 40));
    HIP_TRY(hipGetLastError());
    const int pif = plan->pairs_in_flight;
    ffsa::QualDesc* hq = (ffsa::QualDesc*)plan->desc.host;
    ffsa::MatchLists* hl = (ffsa::MatchLists*)(hq + pif);
    const ffsa::QualDesc* dq = (const ffsa::QualDesc*)plan->desc.dev;
    const ffsa::MatchLists* dl = (const ffsa::MatchLists*)(dq + pif);
    int n_sm = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_sm, hipDeviceAttributeMultiprocessorCount, plan->device));
    std::vector<int> order((size_t)pif);
    for (int p0 = 0; p0 < n_pairs; p0 += pif) {
        const int np = std::min(pif, n_pairs - p0);
        if (int rc = plan->desc.wait_free()) return rc;
        // list pairs first, bit pairs behind them (k_quality_peaks finds a pair's record by its out_row)
        int n_runs = 0, n_bits = 0;
        for (int i = 0; i < np; ++i) {
            const int p = p0 + i;
            const int64_t vr = pair_ref[p], vs = (int64_t)n_ref + pair_sub[p];
            bool runs = algorithm == FFS_MATCH_RUNS;
            if (algorithm == FFS_MATCH_AUTO)  // coincidences per lag |P||Q| / R against S / 32 word steps per lag
                runs = (double)hd[vr].n * (double)hd[vs].n * FFS_MATCH_AUTO_COST <= (double)v_len(vr) * ((double)v_len(vs) / 32.0);
            if (runs)
                order[(size_t)n_runs++] = p;
            else
                order[(size_t)(np - 1 - n_bits++)] = p;
        }
        int64_t max_lags_runs = 0, max_count_bits = 0, max_sw = 0;
        for (int i = 0; i < np; ++i) {
            const int p = order[(size_t)i];
            const int ir = pair_ref[p], is = pair_sub[p];
            const int64_t vr = ir, vs = (int64_t)n_ref + is;
            const int64_t R = ref_len[ir], S = sub_len[is];
            ffsa::QualDesc& q = hq[i];
            memset(&q, 0, sizeof q);
            q.r = plan->bits + vr * plan->vec_words;
            q.s = plan->bits + vs * plan->vec_words;
            qual_window(&q, R, S, max_offset_samples);
            q.cd.s0 = mapped(sub_lo[is]);
            q.cd.s1 = mapped(sub_hi[is]);
            q.cd.r0 = mapped(ref_lo[ir]);
            q.cd.r1 = mapped(ref_hi[ir]);
            q.pre_r = plan->pre + vr * plan->pre_words;
            q.pre_s = plan->pre + vs * plan->pre_words;
            q.curve = plan->curve + (int64_t)i * plan->lpad;
            q.sc = plan->sc + (int64_t)i * plan->lpad;
            q.out_row = p;
            hl[i] = ffsa::MatchLists{(const int2*)((const char*)ref_list[ir] + 16), (const int2*)((const char*)sub_list[is] + 16),
                                     hd[vr].n, hd[vs].n, hd[vr].ones, 0};
            if (i < n_runs) {
                max_lags_runs = std::max(max_lags_runs, q.n_lags);
            } else {
                max_count_bits = std::max(max_count_bits, q.n_count);
                max_sw = std::max(max_sw, (S + 31) / 32);
            }
        }
        // one upload of both arrays (the MatchLists half is at a fixed offset: copy the whole used span)
        if (int rc = plan->desc.upload(sizeof(ffsa::QualDesc) * pif + sizeof(ffsa::MatchLists) * np, st)) return rc;
        if (n_runs > 0 && max_lags_runs > 0) {
            const int64_t n_tiles = (max_lags_runs + ffsa::MATCH_TILE - 1) / ffsa::MATCH_TILE;
            hipLaunchKernelGGL(ffsa::k_runs_curve, dim3((unsigned)(n_runs * n_tiles)), dim3(ffsa::MATCH_THREADS), 0, st, dq, dl,
                               (int)n_tiles);
        }
        if (n_bits > 0 && max_count_bits > 0) {
            HIP_TRY(hipMemsetAsync(plan->curve + (int64_t)n_runs * plan->lpad, 0, (size_t)n_bits * plan->lpad * 4, st));
            quality_counts(dq + n_runs, n_bits, max_count_bits, max_sw, n_sm, st);
        }
        hipLaunchKernelGGL(ffsa::k_quality_peaks, dim3(np), dim3(ffsa::QUAL_PEAK_THREADS), 0, st, dq, top_k,
                           exclusion_samples, (ffsa::QualResult*)out_dev);
        HIP_TRY(hipGetLastError());
    }
    return plan->end(st);
}

/* ---- progressive alignment: the report of a growing reference prefix (csrc/ffs_progressive.h) -------------------- */

namespace {
struct ProgSlot {  // what the host knows of a slot: every refusal is decided from this, before any launch
    bool open = false;
    int n_cand = 0;
    int64_t W = 0, L = 0;
    bool sampled = false;  // a sampled slot (csrc/ffs_sampled.h): L = |K|, the merged intervals in the plan's tables
    int64_t T = 0;
    int n_iv = 0;
    int64_t S[ffsa::PROG_MAX_CAND];
    double s0[ffsa::PROG_MAX_CAND], s1[ffsa::PROG_MAX_CAND], r0, r1;  // mapped levels
};

// index of the first of the n ascending, disjoint intervals iv[2k], iv[2k + 1] that ends at or behind a (n: none)
int prog_first_ending_at(const int64_t* iv, int n, int64_t a) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (iv[2 * mid + 1] < a)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
}  // namespace

struct ffs_prog_plan : PlanCore {
    int max_slots, max_cand;
    int64_t max_lags, max_ref, max_sub;
    int64_t lpad, rw, sw;       // padded curve row, words (and prefix entries) per reference and per candidate
    uint32_t* ref;              // [slot][rw]
    int32_t* pre_r;             // [slot][rw]
    uint32_t* sub;              // [slot][cand][sw]
    int32_t* pre_s;             // [slot][cand][sw]
    uint32_t* curve;            // [slot][cand][lpad]
    double* sc;                 // [slot][cand][lpad]
    std::vector<ProgSlot> slots;
    std::vector<char> named;    // per slot: named by the call being checked
                                // desc: ProgOpenDesc[max_slots * max_cand] at open; at append ProgSlotDesc[max_slots],
                                // then QualDesc[max_slots * max_cand]
    // sampled slots, made by the first ffs_prog_open_sampled
    uint32_t* side = nullptr;   // [slot][cand][3][lpad]: ov, n1x, nx1
    DescStaging samp_desc;      // SampOpenDesc[max_slots * max_cand] at open; at append ProgSlotDesc[max_slots],
                                // SampSlotDesc[max_slots], then SampDesc[max_slots * max_cand]
    std::vector<int64_t> iv;    // [slot][FFS_PROG_MAX_INTERVALS][2]: the merged known intervals, ascending
    int64_t sampled_bytes = 0;  // what the three above hold, each counted when it is made

    void carve(Carver& c) {
        const int64_t n = max_slots, nc = (int64_t)max_slots * max_cand;
        sc = c.take<double>(nc * lpad);
        curve = c.take<uint32_t>(nc * lpad);
        ref = c.take<uint32_t>(n * rw);
        pre_r = c.take<int32_t>(n * rw);
        sub = c.take<uint32_t>(nc * sw);
        pre_s = c.take<int32_t>(nc * sw);
    }

    // the rows of one slot, and of one (slot, candidate)
    uint32_t* ref_row(int s) const { return ref + (int64_t)s * rw; }
    int32_t* pre_r_row(int s) const { return pre_r + (int64_t)s * rw; }
    int64_t cand_at(int s, int c) const { return (int64_t)s * max_cand + c; }
    uint32_t* sub_row(int s, int c) const { return sub + cand_at(s, c) * sw; }
    int32_t* pre_s_row(int s, int c) const { return pre_s + cand_at(s, c) * sw; }
    uint32_t* curve_row(int s, int c) const { return curve + cand_at(s, c) * lpad; }
    double* sc_row(int s, int c) const { return sc + cand_at(s, c) * lpad; }
    uint32_t* side_row(int s, int c) const { return side + cand_at(s, c) * 3 * lpad; }
    int64_t* iv_row(int s) { return iv.data() + (size_t)s * FFS_PROG_MAX_INTERVALS * 2; }

    // one slot of a call: in range; `want_open`: and open
    int check_slot(const char* call, int s, bool want_open) const {
        if (s < 0 || s >= max_slots) return fail(FFS_E_INVALID, "%s: slot %d outside [0, %d)", call, s, max_slots);
        if (want_open && !slots[s].open) return fail(FFS_E_INVALID, "%s: slot %d is not open", call, s);
        return FFS_OK;
    }

    // the slot list of a call: every slot in range and named once; `want_open`: and open
    // (a slot named twice is reported as that: its first mention has passed the openness check)
    int check_slots(const char* call, int n, const int32_t* slot, bool want_open) {
        std::fill(named.begin(), named.end(), 0);
        for (int i = 0; i < n; ++i) {
            const int s = slot[i];
            if (int rc = check_slot(call, s, want_open)) return rc;
            if (named[s]) return fail(FFS_E_INVALID, "%s: slot %d named twice", call, s);
            named[s] = 1;
        }
        return FFS_OK;
    }

    // may [a, a + n) join a sampled slot's known intervals: inside [0, T), disjoint from them, the table not overfull
    int check_interval(const char* call, int s, int64_t a, int64_t n) {
        const ProgSlot& ps = slots[s];
        if (a < 0 || a > ps.T || n > ps.T - a)
            return fail(FFS_E_INVALID, "%s: slot %d: [%lld, %lld + %lld) outside the reference [0, %lld)", call, s, (long long)a,
                        (long long)a, (long long)n, (long long)ps.T);
        if (n == 0) return FFS_OK;
        const int64_t b = a + n;
        const int64_t* iv = iv_row(s);
        // the table is ascending and disjoint: only the first interval that ends at or behind a, and the one after an
        // abutting one, can meet [a, b) -- a search, so that the host's share of a call does not grow with what is known
        int joins = 0, k = prog_first_ending_at(iv, ps.n_iv, a);
        if (k < ps.n_iv && iv[2 * k + 1] == a) ++joins, ++k;
        if (k < ps.n_iv && iv[2 * k] < b)
            return fail(FFS_E_INVALID, "%s: slot %d: [%lld, %lld) overlaps the known interval [%lld, %lld)", call, s,
                        (long long)a, (long long)b, (long long)iv[2 * k], (long long)iv[2 * k + 1]);
        if (k < ps.n_iv && iv[2 * k] == b) ++joins;
        if (ps.n_iv + 1 - joins > FFS_PROG_MAX_INTERVALS)
            return fail(FFS_E_INVALID, "%s: slot %d: more than %d known intervals", call, s, FFS_PROG_MAX_INTERVALS);
        return FFS_OK;
    }

    // merge a checked, non-empty [a, b) into a sampled slot's table: it stays ascending
    void merge_interval(int s, int64_t a, int64_t b) {
        ProgSlot& ps = slots[s];
        int64_t* iv = iv_row(s);
        const int at = prog_first_ending_at(iv, ps.n_iv, a);
        int last = at;                                    // [at, last): the intervals that abut [a, b)
        if (last < ps.n_iv && iv[2 * last + 1] == a) a = iv[2 * last++];
        if (last < ps.n_iv && iv[2 * last] == b) b = iv[2 * last++ + 1];
        const int removed = last - at;
        if (removed == 0)
            memmove(iv + 2 * (at + 1), iv + 2 * at, sizeof(int64_t) * 2 * (size_t)(ps.n_iv - at));
        else if (removed == 2)
            memmove(iv + 2 * (at + 1), iv + 2 * (at + 2), sizeof(int64_t) * 2 * (size_t)(ps.n_iv - at - 2));
        iv[2 * at] = a;
        iv[2 * at + 1] = b;
        ps.n_iv += 1 - removed;
    }
};

int ffs_prog_plan_create(int device, int max_slots, int max_cand, int64_t max_lags, int64_t max_ref_samples,
                         int64_t max_sub_samples, ffs_prog_plan** out) {
    if (!out) return fail(FFS_E_INVALID, "null output handle");
    *out = nullptr;
    if (max_slots < 1 || max_slots > 65536 || max_cand < 1 || max_cand > ffsa::PROG_MAX_CAND || max_lags < 2 ||
        max_lags > 262144 || max_ref_samples < 1 || max_ref_samples >= (int64_t(1) << 30) || max_sub_samples < 1 ||
        max_sub_samples >= (int64_t(1) << 30))
        return fail(FFS_E_INVALID, "progressive plan: need 1 <= max_slots <= 65536, 1 <= max_cand <= 8, 2 <= max_lags <= "
                                   "262144, 1 <= max_ref_samples, max_sub_samples < 2^30");
    HIP_TRY(hipSetDevice(device));
    ffs_prog_plan* p = new (std::nothrow) ffs_prog_plan();
    if (!p) return fail(FFS_E_NOMEM, "progressive plan");
    p->max_slots = max_slots;
    p->max_cand = max_cand;
    p->max_lags = max_lags;
    p->max_ref = max_ref_samples;
    p->max_sub = max_sub_samples;
    p->lpad = split_align_up(max_lags, 64);
    p->rw = split_align_up(max_ref_samples / 32 + 2, 16);
    p->sw = split_align_up(max_sub_samples / 32 + 2, 16);
    p->slots.resize(max_slots);
    p->named.resize(max_slots);
    Carver size{nullptr};
    p->carve(size);
    if (int rc = p->open(device, max_slots, size.used, "progressive plan")) {
        ffs_prog_plan_destroy(p);
        return rc;
    }
    Carver place{(char*)p->work};
    p->carve(place);
    const size_t nc = (size_t)max_slots * max_cand;
    const size_t desc_bytes = std::max(sizeof(ffsa::ProgOpenDesc) * nc,
                                       sizeof(ffsa::ProgSlotDesc) * (size_t)max_slots + sizeof(ffsa::QualDesc) * nc);
    if (p->desc.create(desc_bytes) != FFS_OK) {
        ffs_prog_plan_destroy(p);
        return fail(FFS_E_HIP, "progressive plan: descriptor buffers / events");
    }
    *out = p;
    return FFS_OK;
}

int ffs_prog_plan_destroy(ffs_prog_plan* plan) {
    if (!plan) return FFS_OK;
    plan->close();
    delete plan;
    return FFS_OK;
}

// (what sampled slots add on first use is reported by ffs_prog_plan_sampled_bytes, not here: the formula stays)
int64_t ffs_prog_plan_workspace_bytes(const ffs_prog_plan* plan) { return plan ? plan->work_bytes : 0; }

namespace {
// ffs_prog_open, and with `ref_total` ffs_prog_open_sampled: the same checks and the same k_prog_open
int prog_open(const char* call, ffs_prog_plan* plan, int n, const int32_t* slot, const int32_t* n_cand,
              const void* const* sub_ptr, const int64_t* sub_len, const double* sub_lo, const double* sub_hi,
              const double* ref_lo, const double* ref_hi, const int64_t* max_offset_samples, const int64_t* ref_total,
              bool sampled, void* hip_stream) {
    if (int rc = check_call(plan, "progressive", n,
                            !slot || !n_cand || !sub_ptr || !sub_len || !sub_lo || !sub_hi || !ref_lo || !ref_hi ||
                                !max_offset_samples || (sampled && !ref_total));
        rc != CALL_GO_ON)
        return rc;
    if (n > plan->max_slots) return fail(FFS_E_INVALID, "%s: %d slots exceed the plan's max_slots %d", call, n, plan->max_slots);
    if (int rc = plan->check_slots(call, n, slot, false)) return rc;
    const int mc = plan->max_cand;
    for (int i = 0; i < n; ++i) {
        if (n_cand[i] < 1 || n_cand[i] > mc)
            return fail(FFS_E_INVALID, "%s: slot %d: n_cand=%d outside [1, %d]", call, slot[i], n_cand[i], mc);
        if (int rc = check_window(max_offset_samples[i], plan->max_lags)) return rc;
        if (!(std::isfinite(ref_lo[i]) && std::isfinite(ref_hi[i])))
            return fail(FFS_E_INVALID, "%s: slot %d: levels must be finite", call, slot[i]);
        for (int c = 0; c < n_cand[i]; ++c) {
            const int64_t k = (int64_t)i * mc + c;
            if (!sub_ptr[k] || ((uintptr_t)sub_ptr[k] & 3))
                return fail(FFS_E_INVALID, "%s: slot %d candidate %d: null or misaligned vector", call, slot[i], c);
            if (sub_len[k] < 1 || sub_len[k] > plan->max_sub)
                return fail(FFS_E_INVALID, "%s: slot %d candidate %d: length %lld outside [1, max_sub_samples %lld]", call,
                            slot[i], c, (long long)sub_len[k], (long long)plan->max_sub);
            if (!(std::isfinite(sub_lo[k]) && std::isfinite(sub_hi[k])))
                return fail(FFS_E_INVALID, "%s: slot %d candidate %d: levels must be finite", call, slot[i], c);
        }
        if (sampled && (ref_total[i] < 1 || ref_total[i] > plan->max_ref))
            return fail(FFS_E_INVALID, "%s: slot %d: ref_total=%lld outside [1, max_ref_samples %lld]", call, slot[i],
                        (long long)ref_total[i], (long long)plan->max_ref);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    if (sampled) {  // the first sampled slot of this plan: side curves, descriptors, interval tables
        const size_t ms = (size_t)plan->max_slots, nc = ms * plan->max_cand;
        if (!plan->side) {
            const int64_t side_bytes = (int64_t)nc * 3 * plan->lpad * (int64_t)sizeof(uint32_t);
            void* mem = nullptr;
            if (int rc = plan->add_block(&mem, side_bytes, "progressive plan", "sampled side curve")) return rc;
            plan->side = (uint32_t*)mem;
            plan->sampled_bytes += side_bytes;
        }
        if (!plan->samp_desc.dev) {
            const size_t desc_bytes =
                std::max(sizeof(ffsa::SampOpenDesc) * nc,
                         (sizeof(ffsa::ProgSlotDesc) + sizeof(ffsa::SampSlotDesc)) * ms + sizeof(ffsa::SampDesc) * nc);
            if (int rc = plan->add_staging(&plan->samp_desc, desc_bytes, 0, "progressive plan: sampled descriptor buffers / events"))
                return rc;
            plan->iv.assign(ms * FFS_PROG_MAX_INTERVALS * 2, 0);
            plan->sampled_bytes += (int64_t)desc_bytes + (int64_t)(plan->iv.size() * sizeof(int64_t));
        }
    }
    if (int rc = plan->desc.wait_free()) return rc;
    if (sampled)
        if (int rc = plan->samp_desc.wait_free()) return rc;
    ffsa::ProgOpenDesc* hd = (ffsa::ProgOpenDesc*)plan->desc.host;
    ffsa::SampOpenDesc* hz = sampled ? (ffsa::SampOpenDesc*)plan->samp_desc.host : nullptr;
    int nd = 0;
    for (int i = 0; i < n; ++i) {
        ProgSlot& ps = plan->slots[slot[i]];
        ps.open = true;
        ps.sampled = sampled;
        ps.T = sampled ? ref_total[i] : 0;
        ps.n_iv = 0;
        ps.n_cand = n_cand[i];
        ps.W = max_offset_samples[i];
        ps.L = 0;
        ps.r0 = mapped(ref_lo[i]);
        ps.r1 = mapped(ref_hi[i]);
        for (int c = 0; c < n_cand[i]; ++c) {
            const int64_t k = (int64_t)i * mc + c;
            ps.S[c] = sub_len[k];
            ps.s0[c] = mapped(sub_lo[k]);
            ps.s1[c] = mapped(sub_hi[k]);
            if (sampled) {
                ffsa::SampOpenDesc& z = hz[nd];
                z.side = plan->side_row(slot[i], c);
                z.pre_r = c == 0 ? plan->pre_r_row(slot[i]) : nullptr;
                z.lpad = plan->lpad;
                z.r_words = plan->rw;
            }
            ffsa::ProgOpenDesc& d = hd[nd++];
            d.src = (const uint32_t*)sub_ptr[k];
            d.s = plan->sub_row(slot[i], c);
            d.pre_s = plan->pre_s_row(slot[i], c);
            d.curve = plan->curve_row(slot[i], c);
            d.r = c == 0 ? plan->ref_row(slot[i]) : nullptr;
            d.pre_r = c == 0 ? plan->pre_r_row(slot[i]) : nullptr;
            d.S = sub_len[k];
            d.lpad = plan->lpad;
            d.r_words = plan->rw;
        }
    }
    if (int rc = plan->desc.upload(sizeof(ffsa::ProgOpenDesc) * nd, st)) return rc;
    hipLaunchKernelGGL(ffsa::k_prog_open, dim3((unsigned)nd), dim3(ffsa::PROG_THREADS), 0, st,
                       (const ffsa::ProgOpenDesc*)plan->desc.dev);
    if (sampled) {
        if (int rc = plan->samp_desc.upload(sizeof(ffsa::SampOpenDesc) * nd, st)) return rc;
        hipLaunchKernelGGL(ffsa::k_samp_zero, dim3((unsigned)nd), dim3(ffsa::PROG_THREADS), 0, st,
                           (const ffsa::SampOpenDesc*)plan->samp_desc.dev);
    }
    HIP_TRY(hipGetLastError());
    return plan->end(st);
}

// The rest of entry i of an append to prefix slots, in the plan's `desc` (ProgSlotDesc[max_slots], then QualDesc[]): what
// k_prog_ingest reads into `s`, and one QualDesc per candidate from index nq on.  Returns the next free QualDesc.
int prog_fill_prefix(ffs_prog_plan* plan, ffsa::ProgSlotDesc& s, int i, int slot, const void* chunk, int first_bit, int nq) {
    const ProgSlot& ps = plan->slots[slot];
    ffsa::QualDesc* hq = (ffsa::QualDesc*)((ffsa::ProgSlotDesc*)plan->desc.host + plan->max_slots);
    s.chunk = (const uint32_t*)chunk;
    s.r = plan->ref_row(slot);
    s.pre_r = plan->pre_r_row(slot);
    s.W = ps.W;
    s.first_bit = first_bit;
    s.desc0 = nq;
    for (int c = 0; c < ps.n_cand; ++c) {
        ffsa::QualDesc& q = hq[nq++];
        memset(&q, 0, sizeof q);
        q.r = s.r;
        q.s = plan->sub_row(slot, c);
        q.R = ps.L;
        q.S = ps.S[c];
        q.d_lo = -ps.W + 1;
        q.n_lags = 2 * ps.W;
        const int64_t clo = std::max(q.d_lo, 1 - q.S), chi = std::min(ps.W, q.R - 1);
        q.c_lo = clo;
        q.n_count = chi >= clo ? chi - clo + 1 : 0;
        q.cd.R = (int32_t)q.R;
        q.cd.S = (int32_t)q.S;
        q.cd.s0 = ps.s0[c];
        q.cd.s1 = ps.s1[c];
        q.cd.r0 = ps.r0;
        q.cd.r1 = ps.r1;
        q.pre_r = s.pre_r;
        q.pre_s = plan->pre_s_row(slot, c);
        q.curve = plan->curve_row(slot, c);
        q.sc = plan->sc_row(slot, c);
        q.out_row = (int64_t)i * plan->max_cand + c;
    }
    return nq;
}

// The same for sampled slots, in the plan's `samp_desc` (ProgSlotDesc[max_slots], SampSlotDesc[max_slots], then
// SampDesc[]): entry i's SampSlotDesc for a chunk at `a`, and one SampDesc per candidate.
int prog_fill_sampled(ffs_prog_plan* plan, int i, int slot, const void* chunk, int first_bit, int64_t a, int64_t n_new,
                      int nq) {
    const ProgSlot& ps = plan->slots[slot];
    ffsa::SampSlotDesc* hs = (ffsa::SampSlotDesc*)((ffsa::ProgSlotDesc*)plan->samp_desc.host + plan->max_slots);
    ffsa::SampDesc* hq = (ffsa::SampDesc*)(hs + plan->max_slots);
    ffsa::SampSlotDesc& s = hs[i];
    memset(&s, 0, sizeof s);
    s.chunk = (const uint32_t*)chunk;
    s.r = plan->ref_row(slot);
    s.pre_r = plan->pre_r_row(slot);
    s.a = a;
    s.n_new = n_new;
    s.T = ps.T;
    s.W = ps.W;
    s.first_bit = first_bit;
    s.n_cand = ps.n_cand;
    s.desc0 = nq;
    for (int c = 0; c < ps.n_cand; ++c) {
        ffsa::SampDesc& q = hq[nq++];
        memset(&q, 0, sizeof q);
        q.s = plan->sub_row(slot, c);
        q.pre_s = plan->pre_s_row(slot, c);
        q.n11 = plan->curve_row(slot, c);
        q.side = plan->side_row(slot, c);
        q.sc = plan->sc_row(slot, c);
        q.S = ps.S[c];
        q.lpad = plan->lpad;
        q.n_lags = 2 * ps.W;
        q.d_lo = -ps.W + 1;
        q.out_row = (int64_t)i * plan->max_cand + c;
        q.s0 = ps.s0[c];
        q.s1 = ps.s1[c];
        q.r0 = ps.r0;
        q.r1 = ps.r1;
    }
    return nq;
}

// ffs_prog_append, and with `position` ffs_prog_append_at: the same checks in the same order, the same begin / stage /
// upload / end, the same four launches.  The kinds differ in one range check, in the staging block and its fill
// (above), and in the ingest, counts and peaks kernels.  No slot's state moves before every check of every slot passed.
int prog_append(const char* call, ffs_prog_plan* plan, int n, const int32_t* slot, const void* const* chunk_dev,
                const int32_t* first_bit, const int64_t* position, const int64_t* n_new, int top_k,
                int64_t exclusion_samples, ffs_quality_result* cand_out_dev, ffs_prog_state* state_out_dev, bool sampled,
                void* hip_stream) {
    static_assert(sizeof(ffs_prog_state) == sizeof(ffsa::ProgState), "device records must match the header's");
    if (int rc = check_call(plan, "progressive", n,
                            !slot || !chunk_dev || !first_bit || (sampled && !position) || !n_new || !cand_out_dev ||
                                !state_out_dev);
        rc != CALL_GO_ON)
        return rc;
    if (int rc = check_peaks(top_k, exclusion_samples)) return rc;
    if (((uintptr_t)cand_out_dev | (uintptr_t)state_out_dev) & 7) return fail(FFS_E_INVALID, "misaligned output records");
    if (n > plan->max_slots) return fail(FFS_E_INVALID, "%s: %d slots exceed the plan's max_slots %d", call, n, plan->max_slots);
    if (int rc = plan->check_slots(call, n, slot, true)) return rc;
    for (int i = 0; i < n; ++i) {
        const ProgSlot& ps = plan->slots[slot[i]];
        if (ps.sampled != sampled)
            return sampled ? fail(FFS_E_INVALID, "%s: slot %d is a prefix slot: use ffs_prog_append", call, slot[i])
                           : fail(FFS_E_INVALID, "%s: slot %d is a sampled slot: use ffs_prog_append_at", call, slot[i]);
        if (!chunk_dev[i] || ((uintptr_t)chunk_dev[i] & 3))
            return fail(FFS_E_INVALID, "%s: slot %d: null or misaligned chunk", call, slot[i]);
        if (first_bit[i] < 0 || first_bit[i] > 31)
            return fail(FFS_E_INVALID, "%s: slot %d: first_bit=%d outside [0, 32)", call, slot[i], first_bit[i]);
        if (n_new[i] < 0) return fail(FFS_E_INVALID, "%s: slot %d: n_new=%lld is negative", call, slot[i], (long long)n_new[i]);
        if (sampled) {
            if (int rc = plan->check_interval(call, slot[i], position[i], n_new[i])) return rc;
        } else if (n_new[i] > plan->max_ref - ps.L) {
            return fail(FFS_E_INVALID, "%s: slot %d: %lld + %lld samples exceed the plan's max_ref_samples %lld", call, slot[i],
                        (long long)ps.L, (long long)n_new[i], (long long)plan->max_ref);
        }
    }
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = plan->begin(st)) return rc;
    DescStaging& stage = sampled ? plan->samp_desc : plan->desc;
    if (int rc = stage.wait_free()) return rc;
    int nq = 0;
    int64_t max_w = 0;
    for (int i = 0; i < n; ++i) {
        ProgSlot& ps = plan->slots[slot[i]];
        ffsa::ProgSlotDesc& p = ((ffsa::ProgSlotDesc*)stage.host)[i];  // first in either block: all that k_prog_pick reads
        memset(&p, 0, sizeof p);
        p.L = ps.L;  // the length (of a sampled slot: |K|) before this append
        p.n_new = n_new[i];
        p.n_cand = ps.n_cand;
        ps.L += n_new[i];
        if (sampled && n_new[i] > 0) plan->merge_interval(slot[i], position[i], position[i] + n_new[i]);
        max_w = std::max(max_w, ps.W);
        nq = sampled ? prog_fill_sampled(plan, i, slot[i], chunk_dev[i], first_bit[i], position[i], n_new[i], nq)
                     : prog_fill_prefix(plan, p, i, slot[i], chunk_dev[i], first_bit[i], nq);
    }
    // one upload of all the arrays (the later ones are at fixed offsets: copy the whole used span)
    const size_t ms = (size_t)plan->max_slots;
    const size_t used = sampled ? (sizeof(ffsa::ProgSlotDesc) + sizeof(ffsa::SampSlotDesc)) * ms + sizeof(ffsa::SampDesc) * nq
                                : sizeof(ffsa::ProgSlotDesc) * ms + sizeof(ffsa::QualDesc) * nq;
    if (int rc = stage.upload(used, st)) return rc;
    const int mc = plan->max_cand, n_tiles = (int)((2 * max_w + ffsa::PROG_TILE - 1) / ffsa::PROG_TILE);
    const dim3 per_slot((unsigned)n), per_tile((unsigned)((int64_t)n * mc * n_tiles)), per_cand((unsigned)nq);
    const ffsa::ProgSlotDesc* dp = (const ffsa::ProgSlotDesc*)stage.dev;
    ffsa::QualResult* cand_out = (ffsa::QualResult*)cand_out_dev;
    if (sampled) {
        const ffsa::SampSlotDesc* ds = (const ffsa::SampSlotDesc*)(dp + ms);
        const ffsa::SampDesc* dq = (const ffsa::SampDesc*)(ds + ms);
        hipLaunchKernelGGL(ffsa::k_samp_ingest, per_slot, dim3(ffsa::PROG_THREADS), 0, st, ds);
        hipLaunchKernelGGL(ffsa::k_samp_counts, per_tile, dim3(ffsa::PROG_CNT_THREADS), 0, st, ds, dq, n_tiles, mc);
        hipLaunchKernelGGL(ffsa::k_samp_peaks, per_cand, dim3(ffsa::QUAL_PEAK_THREADS), 0, st, dq, top_k, exclusion_samples,
                           cand_out);
    } else {
        const ffsa::QualDesc* dq = (const ffsa::QualDesc*)(dp + ms);
        hipLaunchKernelGGL(ffsa::k_prog_ingest, per_slot, dim3(ffsa::PROG_THREADS), 0, st, dp);
        hipLaunchKernelGGL(ffsa::k_prog_counts, per_tile, dim3(ffsa::PROG_CNT_THREADS), 0, st, dp, dq, n_tiles, mc);
        hipLaunchKernelGGL(ffsa::k_quality_peaks, per_cand, dim3(ffsa::QUAL_PEAK_THREADS), 0, st, dq, top_k,
                           exclusion_samples, cand_out);
    }
    hipLaunchKernelGGL(ffsa::k_prog_pick, per_slot, dim3(ffsa::PROG_PICK_THREADS), 0, st, dp, mc, cand_out,
                       (ffsa::ProgState*)state_out_dev);
    HIP_TRY(hipGetLastError());
    return plan->end(st);
}
}  // namespace

int ffs_prog_open(ffs_prog_plan* plan, int n, const int32_t* slot, const int32_t* n_cand, const void* const* sub_ptr,
                  const int64_t* sub_len, const double* sub_lo, const double* sub_hi, const double* ref_lo,
                  const double* ref_hi, const int64_t* max_offset_samples, void* hip_stream) {
    return prog_open("ffs_prog_open", plan, n, slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi,
                     max_offset_samples, nullptr, false, hip_stream);
}

int ffs_prog_open_sampled(ffs_prog_plan* plan, int n, const int32_t* slot, const int32_t* n_cand, const void* const* sub_ptr,
                          const int64_t* sub_len, const double* sub_lo, const double* sub_hi, const double* ref_lo,
                          const double* ref_hi, const int64_t* max_offset_samples, const int64_t* ref_total,
                          void* hip_stream) {
    return prog_open("ffs_prog_open_sampled", plan, n, slot, n_cand, sub_ptr, sub_len, sub_lo, sub_hi, ref_lo, ref_hi,
                     max_offset_samples, ref_total, true, hip_stream);
}

int64_t ffs_prog_plan_sampled_bytes(const ffs_prog_plan* plan) { return plan ? plan->sampled_bytes : 0; }

int ffs_prog_append(ffs_prog_plan* plan, int n, const int32_t* slot, const void* const* chunk_dev, const int32_t* first_bit,
                    const int64_t* n_new, int top_k, int64_t exclusion_samples, ffs_quality_result* cand_out_dev,
                    ffs_prog_state* state_out_dev, void* hip_stream) {
    return prog_append("ffs_prog_append", plan, n, slot, chunk_dev, first_bit, nullptr, n_new, top_k, exclusion_samples,
                       cand_out_dev, state_out_dev, false, hip_stream);
}

int ffs_prog_append_at(ffs_prog_plan* plan, int n, const int32_t* slot, const void* const* chunk_dev, const int32_t* first_bit,
                       const int64_t* position, const int64_t* n_new, int top_k, int64_t exclusion_samples,
                       ffs_quality_result* cand_out_dev, ffs_prog_state* state_out_dev, void* hip_stream) {
    return prog_append("ffs_prog_append_at", plan, n, slot, chunk_dev, first_bit, position, n_new, top_k, exclusion_samples,
                       cand_out_dev, state_out_dev, true, hip_stream);
}

int ffs_prog_reference(ffs_prog_plan* plan, int slot, const uint32_t** bits_dev, int64_t* len) {
    if (!plan) return fail(FFS_E_INVALID, "null progressive plan");
    if (!bits_dev || !len) return fail(FFS_E_INVALID, "null argument");
    if (int rc = plan->check_slot("ffs_prog_reference", slot, true)) return rc;
    *bits_dev = plan->ref_row(slot);
    *len = plan->slots[slot].sampled ? plan->slots[slot].T : plan->slots[slot].L;
    return FFS_OK;
}

int ffs_prog_known(ffs_prog_plan* plan, int slot, int64_t* bounds_out, int cap, int* n_out) {
    if (!plan) return fail(FFS_E_INVALID, "null progressive plan");
    if (!n_out || cap < 0 || (cap > 0 && !bounds_out)) return fail(FFS_E_INVALID, "null argument");
    if (int rc = plan->check_slot("ffs_prog_known", slot, false)) return rc;
    const ProgSlot& ps = plan->slots[slot];
    if (!ps.open || !ps.sampled) return fail(FFS_E_INVALID, "ffs_prog_known: slot %d is not an open sampled slot", slot);
    if (ps.n_iv > cap) return fail(FFS_E_INVALID, "ffs_prog_known: %d intervals exceed cap=%d", ps.n_iv, cap);
    if (ps.n_iv > 0) memcpy(bounds_out, plan->iv_row(slot), sizeof(int64_t) * 2 * (size_t)ps.n_iv);
    *n_out = ps.n_iv;
    return FFS_OK;
}

int ffs_prog_close(ffs_prog_plan* plan, int n, const int32_t* slot) {
    if (int rc = check_call(plan, "progressive", n, !slot); rc != CALL_GO_ON) return rc;
    if (n > plan->max_slots) return fail(FFS_E_INVALID, "ffs_prog_close: %d slots exceed the plan's max_slots %d", n, plan->max_slots);
    if (int rc = plan->check_slots("ffs_prog_close", n, slot, true)) return rc;
    for (int i = 0; i < n; ++i) plan->slots[slot[i]].open = false;
    return FFS_OK;
}

}  // extern "C"
