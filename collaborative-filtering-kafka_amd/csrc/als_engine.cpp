// als_engine.cpp -- the C ABI of include/als.h: engine lifetime, in-block upload (its work plan: als_plan.h), factor
// buffers, and the half-iteration launch. See include/als.h for the reference interface each entry
// point replaces.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "als.h"
#include "als_internal.h"

using cfk::Path;
using cfk::Task;

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(ALS_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                        __FILE__, __LINE__);                                                       \
    } while (0)

struct Block {
    bool set = false;
    int64_t n_rows = 0, row_offset = 0, n_opp_rows = 0, nnz = 0, nnz_padded = 0;
    int32_t* d_col = nullptr;
    float* d_rat = nullptr;
    uint32_t* d_rat_pk = nullptr;   // pre-split blocks: ratings as fp16 rh / rm pairs (the Gram's RHS operand)
    int32_t* d_col_ps = nullptr;    // pre-split blocks: column indices in the LDS-DMA gather order
    Task* d_tasks = nullptr;        // FULL + PARTIAL, sorted by work (longest first)
    Task* d_reduce = nullptr;       // REDUCE
    int32_t n_tasks = 0, n_reduce = 0, n_slots = 0;
    double* d_task_se = nullptr;    // per-task squared-error partials
    std::vector<Task> h_tasks, h_reduce;   // host copies of the work plan (chunking re-sorts them)
    Task* d_ctasks = nullptr;       // chunk-major FULL + PARTIAL tasks (LPT inside each chunk)
    Task* d_creduce = nullptr;      // chunk-major REDUCE tasks
    std::vector<int32_t> coff, croff;   // chunk c = d_ctasks[coff[c], coff[c+1]), d_creduce[croff[c], ...)
    // short rows solved in entry space (cfk::launch_dual), by entry-tile count cd = 2 (1 block) / 4 (2 blocks)
    Task* d_dual[3] = {nullptr, nullptr, nullptr};
    int32_t n_dual[3] = {0, 0, 0};
    std::vector<Task> h_dual[3];
    Task* d_cdual[3] = {nullptr, nullptr, nullptr};
    std::vector<int32_t> cdoff[3];
    Task* d_sq_tasks = nullptr;     // every FULL + PARTIAL task incl. the short rows (als_sq_error)
    int32_t n_sq = 0;
    cfk::BlockLayout layout;        // the layout the plan was built with (chunk lengths, XCD ranges, pre-split)
    // interleaved split rows: rows longer than layout.ilv entries, blocks permuted chunk-major
    int64_t ilv_rows = 0, ilv_tasks = 0;
    // chunk-major slot layout (als_set_row_layout): local row i -> factor row row_offset + (i / rows_per_chunk) *
    // chunk_stride + i % rows_per_chunk; rows_per_chunk = 0: row_offset + i
    int64_t rows_per_chunk = 0, chunk_stride = 0;
    int64_t factor_row(int64_t i) const {
        return rows_per_chunk > 0 ? row_offset + (i / rows_per_chunk) * chunk_stride + i % rows_per_chunk
                                  : row_offset + i;
    }
};

struct TimingRec {
    int side;
    hipEvent_t ev[3];
};

struct Factors {
    void* ptr = nullptr;
    int64_t n_rows = 0;
    bool owned = false;
};

// What the environment says, read once when an engine is created (read_environment below lists the variables).
struct Settings {
    cfk::PlanKnobs plan;            // ALS_INTERLEAVE, ALS_XCD_RANGES, ALS_PRESPLIT, ALS_DUAL, ALS_CHUNK (+ debug orders)
    bool gram_f32 = false;          // ALS_GRAM=f32
    bool force_valu = false;        // ALS_FORCE_VALU=1
    // ALS_REFINE_MIN_PIVOT (cfk::SolveArgs): 0.45 keeps the worst per-row error ratio to the reference's own fp32
    // path where always refining puts it (0.41, tools/refine_accuracy.py; 0.30 lets it reach 1.2), and skips the
    // step for nearly every Netflix-shape row (k = 128 user half 17.7 -> 14.9 ms); > 1 always refines
    float refine_min_pivot = 0.45f;
    bool dual_side = true;          // ALS_DUAL_SIDE: entry-space launches on a side stream beside the main launch
    int64_t comm_timeout_ms = 120000;   // ALS_COMM_TIMEOUT_S: bound of host waits while a communicator exists
                                        // (als_comm_set_timeout)
    // debug build only (CFK_DEBUG_KNOBS)
    int32_t debug_flags = 0;        // ALS_DEBUG_SKIP_SOLVE / _REFINE
    uint32_t debug_gen_skew = 0;    // ALS_DEBUG_REDUCE_GEN_SKEW=n, REDUCE decodes with generation + n (tests the
                                    // integrity check: every slot reads as written by another launch)
    int32_t debug_extra_lds = 0;    // ALS_DEBUG_EXTRA_LDS=bytes of unused LDS per main-launch workgroup (occupancy
                                    // sweeps of the MFMA kernels)
    bool debug_fixed_gen = false;   // ALS_DEBUG_FIXED_GEN=1, every launch uses generation 1, so partial slots of
                                    // repeated launches are bitwise comparable (diagnostics)
};

}  // namespace

namespace cfk_detail {
void set_last_error(const std::string& s) { g_last_error = s; }
}  // namespace cfk_detail

struct als_engine {
    int device = 0;
    int k = 0, kp = 0;
    int precision = ALS_F32;
    Path path = Path::VALU;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    Block blk[2];
    Factors fac[2];
    void* d_partials = nullptr;
    size_t partial_bytes = 0;
    int64_t generic_slabs = 0;      // generic path: Gram slabs in d_partials
    void* d_split = nullptr;        // pre-split opposite table (launch_presplit_prepare), sized for the larger need
    size_t split_bytes = 0;
    uint32_t* d_prep = nullptr;     // the preparation's device words: two sets of cfk::PREP_SET_WORDS (the range words
                                    //   of the pre-split table, used in turn), then per side the exponent its opposite
                                    //   table was last split at
    int prep_set = 0;               // the set of the last preparation: SolveArgs::amax of the half it served
    void* d_rec = nullptr;          // als_recommend's own grow-only workspace (rows, exclusion CSR, partial and final
    size_t rec_bytes = 0;           //   lists): never d_partials / d_split / d_prep, which a half in progress owns
    void* h_stage = nullptr;        // pinned staging of als_write_factors / als_read_factors (copy kernels)
    size_t stage_bytes = 0;
    uint32_t* d_integrity = nullptr;   // cfk::INTEGRITY_WORDS: partial slots that failed their check
    int cu_count = 0;               // compute units of the device: the range guard's fallback grid
    Settings cfg;                   // what the environment said when the engine was created (read_environment)
    uint32_t gen = 0;               // launch generation of the next PARTIAL/REDUCE pair
    ncclComm_t comm = nullptr;      // RCCL communicator over the G engines (one per GPU) of a sharded run
    int world = 1, rank = 0;
    hipStream_t comm_stream = nullptr;   // all-gathers run here, overlapping the next chunk's solve
    hipEvent_t solved = nullptr;         // recorded on `stream` before each all-gather
    hipEvent_t gathered[2] = {nullptr, nullptr};   // last all-gather of each side, on comm_stream
    bool gather_pending[2] = {false, false};
    int last_gather_side = -1;           // the last all-gather issued (for the timeout's message)
    int64_t last_gather_chunk = -1, last_gather_rows = 0;
    // Entry-space (als_solve_dual) launches run on side_stream, forked from and joined back into `stream`, so
    // they fill the CUs the main launch's tail leaves idle (unless cfg.dual_side is off)
    hipStream_t side_stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<TimingRec> pending;
    size_t elem() const { return precision == ALS_F64 ? 8 : 4; }
};

namespace {

int check_engine(const als_engine* e) {
    if (!e) return fail(ALS_ERR_INVALID_ARGUMENT, "engine is NULL");
    return ALS_OK;
}

// Order the engine's stream after the pending all-gathers of the given sides (comm_stream -> stream).
int wait_gathers(als_engine* e, bool movie, bool user) {
    const bool want[2] = {movie, user};
    for (int s = 0; s < 2; ++s)
        if (want[s] && e->gather_pending[s]) {
            HIP_TRY(hipStreamWaitEvent(e->stream, e->gathered[s], 0));
            e->gather_pending[s] = false;
        }
    return ALS_OK;
}

// Host wait for the engine's stream, bounded while the engine has a communicator: on expiry the communicator is
// aborted (so that its kernels end) and the call fails naming the last all-gather issued.
int stream_wait(als_engine* e, hipStream_t s) {
    if (!e->comm || e->cfg.comm_timeout_ms <= 0) {
        HIP_TRY(hipStreamSynchronize(s));
        return ALS_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        const hipError_t st = hipStreamQuery(s);
        if (st == hipSuccess) return ALS_OK;
        if (st != hipErrorNotReady) return fail(ALS_ERR_DEVICE, "stream wait: %s", hipGetErrorString(st));
        const int64_t ms =
            std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        if (ms > e->cfg.comm_timeout_ms) {
            (void)ncclCommAbort(e->comm);
            e->comm = nullptr;
            return fail(ALS_ERR_COMM,
                        "rank %d of %d: the engine's stream did not complete within %lld ms; the last RCCL all-gather "
                        "issued was side %s chunk %lld (%lld rows per shard); communicator aborted",
                        e->rank, e->world, (long long)e->cfg.comm_timeout_ms,
                        e->last_gather_side == ALS_SIDE_MOVIE ? "movie" : e->last_gather_side == ALS_SIDE_USER ? "user"
                                                                                                              : "none",
                        (long long)e->last_gather_chunk, (long long)e->last_gather_rows);
        }
        if (spin < 1000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// Drain the engine's stream and read the partial-slot integrity record (cfk::SlotCodec): a REDUCE task that
// found a slot it could not see freshly written by this launch's PARTIAL task makes every later synchronising
// call fail until als_integrity_status(..., reset = 1).
int sync_checked(als_engine* e) {
    if (int r = wait_gathers(e, true, true)) return r;
    if (int r = stream_wait(e, e->stream)) return r;
    uint32_t rec[cfk::INTEGRITY_WORDS];
    HIP_TRY(hipMemcpy(rec, e->d_integrity, sizeof(rec), hipMemcpyDeviceToHost));
    if (rec[0] != 0)
        return fail(ALS_ERR_INTEGRITY,
                    "%u REDUCE tasks found partial slots that failed their check (first: launch generation %u, slot "
                    "%u, row %u): partial sums its PARTIAL task's writes had not reached",
                    rec[0], rec[1], rec[2], rec[3]);
    return ALS_OK;
}
int check_side(int side) {
    if (side != ALS_SIDE_MOVIE && side != ALS_SIDE_USER)
        return fail(ALS_ERR_INVALID_ARGUMENT, "side must be ALS_SIDE_MOVIE (0) or ALS_SIDE_USER (1), got %d", side);
    return ALS_OK;
}

void free_block(Block& b) {
    (void)hipFree(b.d_col);
    (void)hipFree(b.d_rat);
    (void)hipFree(b.d_rat_pk);
    (void)hipFree(b.d_col_ps);
    (void)hipFree(b.d_tasks);
    (void)hipFree(b.d_reduce);
    (void)hipFree(b.d_task_se);
    (void)hipFree(b.d_ctasks);
    (void)hipFree(b.d_creduce);
    for (int c = 0; c < 3; ++c) {
        (void)hipFree(b.d_dual[c]);
        (void)hipFree(b.d_cdual[c]);
    }
    (void)hipFree(b.d_sq_tasks);
    b = Block();
}

// The one place the library reads the environment: once per engine, in als_engine_create. A variable changed later
// has no effect on that engine.
//
//   variable              values                                  default
//   ALS_GRAM              f32: the exact-f32 MFMA Gram instead    split-MFMA Gram (fp32, k >= 32)
//                         of the split one
//   ALS_FORCE_VALU        1: the LDS-staged VALU Gram             off
//   ALS_CHUNK             n >= 1: entries per contiguous chunk    nnz_padded / 4096 within [1024, 32768]
//                         of a split row, rounded up to 32
//   ALS_INTERLEAVE        0 off, else on wherever the pre-split   auto (opposite table of 32 MB .. 256 MiB, als_plan.cpp)
//                         Gram exists
//   ALS_XCD_RANGES        0 off, else on for interleaved halves   auto (KP = 64, opposite table within 128 MiB)
//   ALS_PRESPLIT          1 on, anything else off                 auto (KP = 128, small or interleaved table)
//   ALS_DUAL              0 off: no short rows in entry space     on (split path, KP = 64 / 128)
//   ALS_DUAL_SIDE         0: entry-space launches on the main     side stream
//                         stream
//   ALS_REFINE_MIN_PIVOT  x: refine when a scaled pivot < x       0.45 (product build: never below 0.45)
//   ALS_COMM_TIMEOUT_S    seconds (fraction allowed), <= 0 none   120
// Debug build only (CFK_DEBUG_KNOBS, Makefile target `debug`; never in the product library):
//   ALS_DEBUG_SKIP_SOLVE, ALS_DEBUG_SKIP_REFINE   1: drop the k x k solve / the refinement step
//   ALS_DEBUG_REDUCE_GEN_SKEW   n: REDUCE decodes with generation + n       0
//   ALS_DEBUG_FIXED_GEN         1: every launch uses generation 1           off
//   ALS_DEBUG_EXTRA_LDS         bytes of unused LDS per workgroup           0
//   ALS_ILV_CHUNK               n: interleave length (at least 32)          measured lengths (als_plan.cpp)
//   ALS_TASK_ORDER              random | stagger[:W]: main-launch order     longest first
Settings read_environment() {
    Settings c;
    if (const char* env = getenv("ALS_GRAM")) c.gram_f32 = !strcmp(env, "f32");
    if (const char* env = getenv("ALS_FORCE_VALU")) c.force_valu = env[0] == '1';
    if (const char* env = getenv("ALS_CHUNK")) c.plan.chunk = atol(env);
    if (const char* env = getenv("ALS_INTERLEAVE")) c.plan.interleave = env[0] == '0' ? 0 : 1;
    if (const char* env = getenv("ALS_XCD_RANGES")) c.plan.xcd_ranges = env[0] == '0' ? 0 : 1;
    if (const char* env = getenv("ALS_PRESPLIT")) c.plan.presplit = env[0] == '1' ? 1 : 0;
    if (const char* env = getenv("ALS_DUAL")) c.plan.dual = env[0] != '0';
    if (const char* env = getenv("ALS_DUAL_SIDE")) c.dual_side = env[0] != '0';
    if (const char* env = getenv("ALS_REFINE_MIN_PIVOT")) {
        // the product library can only refine MORE often than the validated gate (> 1: every row); thresholds
        // below 0.45 drop accuracy (tools/refine_accuracy.py) and are accepted by the debug build only
        c.refine_min_pivot = (float)atof(env);
#ifndef CFK_DEBUG_KNOBS
        c.refine_min_pivot = std::max(c.refine_min_pivot, 0.45f);
#endif
    }
    if (const char* env = getenv("ALS_COMM_TIMEOUT_S")) c.comm_timeout_ms = (int64_t)(atof(env) * 1000.0);
#ifdef CFK_DEBUG_KNOBS
    // work-dropping diagnostics: compiled only into the tools' debug build, never into the product library
    if (const char* env = getenv("ALS_DEBUG_SKIP_SOLVE"))
        if (env[0] == '1') c.debug_flags |= cfk::SOLVE_FLAG_SKIP_SOLVE;
    if (const char* env = getenv("ALS_DEBUG_SKIP_REFINE"))
        if (env[0] == '1') c.debug_flags |= cfk::SOLVE_FLAG_SKIP_REFINE;
    // integrity fault injection / slot-level diagnostics (tests/test_gpu_integrity.py, tools/split_diag.py): they
    // weaken the partial-slot check, so they exist in the debug build only
    if (const char* env = getenv("ALS_DEBUG_REDUCE_GEN_SKEW")) c.debug_gen_skew = (uint32_t)atoi(env);
    if (const char* env = getenv("ALS_DEBUG_FIXED_GEN")) c.debug_fixed_gen = env[0] == '1';
    if (const char* env = getenv("ALS_DEBUG_EXTRA_LDS")) c.debug_extra_lds = atoi(env);
    // measurement knobs of the plan
    if (const char* env = getenv("ALS_ILV_CHUNK")) c.plan.ilv_chunk = std::max(32L, atol(env));
    if (const char* env = getenv("ALS_TASK_ORDER")) {
        if (std::strncmp(env, "stagger", 7) == 0) {
            c.plan.task_order = cfk::PlanKnobs::STAGGER;
            if (env[7] == ':') c.plan.stagger_window = std::max(1, atoi(env + 8));
        }
        if (std::strcmp(env, "random") == 0) c.plan.task_order = cfk::PlanKnobs::RANDOM;
    }
#endif
    return c;
}
}  // namespace

extern "C" {

int als_abi_version(void) { return ALS_ABI_VERSION; }

int als_device_count(int* n) {
    if (!n) return fail(ALS_ERR_INVALID_ARGUMENT, "n is NULL");
    *n = 0;
    HIP_TRY(hipGetDeviceCount(n));
    return ALS_OK;
}
const char* als_last_error(void) { return g_last_error.c_str(); }

#define CFK_STR2(x) #x
#define CFK_STR(x) CFK_STR2(x)
const char* als_build_source_sha256(void) {
#ifdef CFK_SOURCE_SHA256
    return &CFK_STR(CFK_SOURCE_SHA256)[1];   // "h<digest>": an identifier token, the h dropped
#else
    return "";
#endif
}

int als_engine_create(int device, int num_features, int precision, als_engine** out) {
    if (!out) return fail(ALS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (precision != ALS_F32 && precision != ALS_F64)
        return fail(ALS_ERR_INVALID_ARGUMENT, "precision must be ALS_F32 or ALS_F64");
    if (num_features < 1) return fail(ALS_ERR_INVALID_ARGUMENT, "num_features must be >= 1, got %d", num_features);
    // padded row stride: 16 / 32 / 64 / 128 for the wave-per-row kernels, beyond them (fp32 k > 128, fp64 k > 64:
    // the generic workgroup-per-row path) the next multiple of 16; the reference accepts any NUM_FEATURES
    // (ALSAppRunner.java:18), this build up to 1024
    if (num_features > 1024)
        return fail(ALS_ERR_UNSUPPORTED, "num_features=%d: this build supports 1..1024", num_features);
    const bool generic = num_features > (precision == ALS_F64 ? 64 : 128);
    int kp = num_features <= 16 ? 16 : num_features <= 32 ? 32 : num_features <= 64 ? 64 : 128;
    if (generic) kp = (num_features + 15) / 16 * 16;
    // MFMA Gram only where the accumulation is a real dense contraction (k >= 32, north star); fp64 and
    // small k use the LDS-staged VALU Gram. fp32 Gram products via the exact split (Path::MFMA_SPLIT) by default;
    // ALS_GRAM=f32 selects the v_mfma_f32_16x16x4_f32 path (same accumulator layout, 2.3x the Gram time).
    Path path = generic ? Path::GENERIC : (precision == ALS_F32 && num_features >= 32) ? Path::MFMA_SPLIT : Path::VALU;
    const Settings cfg = read_environment();
    if (path == Path::MFMA_SPLIT && cfg.gram_f32) path = Path::MFMA;
    if (cfg.force_valu && !generic) path = Path::VALU;
    if (!cfk::variant_available(precision, kp, path))
        return fail(ALS_ERR_UNSUPPORTED, "no kernel variant for precision=%d kp=%d", precision, kp);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ALS_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    als_engine* e = new als_engine();
    e->device = device;
    e->k = num_features;
    e->kp = kp;
    e->precision = precision;
    e->path = path;
    e->cfg = cfg;
    hipError_t st = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (st != hipSuccess) {
        delete e;
        return fail(ALS_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(st));
    }
    e->own_stream = true;
    st = hipDeviceGetAttribute(&e->cu_count, hipDeviceAttributeMultiprocessorCount, device);
    if (st == hipSuccess) st = hipMalloc((void**)&e->d_integrity, cfk::INTEGRITY_WORDS * sizeof(uint32_t));
    if (st == hipSuccess) st = hipMemset(e->d_integrity, 0, cfk::INTEGRITY_WORDS * sizeof(uint32_t));
    {   // both sets of range words zero, no side split yet
        uint32_t prep[2 * cfk::PREP_SET_WORDS + 2] = {};
        prep[2 * cfk::PREP_SET_WORDS] = prep[2 * cfk::PREP_SET_WORDS + 1] = cfk::PREP_NO_EXP;
        if (st == hipSuccess) st = hipMalloc((void**)&e->d_prep, sizeof(prep));
        if (st == hipSuccess) st = hipMemcpy(e->d_prep, prep, sizeof(prep), hipMemcpyHostToDevice);
    }
    if (st != hipSuccess) {
        (void)hipStreamDestroy(e->stream);
        (void)hipFree(e->d_integrity);
        (void)hipFree(e->d_prep);
        delete e;
        return fail(ALS_ERR_DEVICE, "integrity record: %s", hipGetErrorString(st));
    }
    *out = e;
    return ALS_OK;
}

int als_engine_destroy(als_engine* e) {
    if (!e) return ALS_OK;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (auto& b : e->blk) free_block(b);
    for (auto& f : e->fac)
        if (f.owned) (void)hipFree(f.ptr);
    (void)hipFree(e->d_partials);
    (void)hipFree(e->d_split);
    (void)hipFree(e->d_rec);
    (void)hipHostFree(e->h_stage);
    (void)hipFree(e->d_integrity);
    (void)hipFree(e->d_prep);
    for (auto& rec : e->pending)
        for (auto ev : rec.ev) (void)hipEventDestroy(ev);
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    if (e->comm_stream) (void)hipStreamDestroy(e->comm_stream);
    for (auto ev : {e->solved, e->gathered[0], e->gathered[1]})
        if (ev) (void)hipEventDestroy(ev);
    if (e->side_stream) {
        (void)hipStreamSynchronize(e->side_stream);
        (void)hipStreamDestroy(e->side_stream);
    }
    for (auto ev : {e->fork, e->join})
        if (ev) (void)hipEventDestroy(ev);
    if (e->own_stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return ALS_OK;
}

int als_engine_set_stream(als_engine* e, void* hip_stream) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    if (e->own_stream) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipStreamDestroy(e->stream));
        e->own_stream = false;
        e->stream = nullptr;
    }
    if (hip_stream) {
        e->stream = (hipStream_t)hip_stream;
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->own_stream = true;
    }
    return ALS_OK;
}

int als_engine_use_default_stream(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    if (e->own_stream) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipStreamDestroy(e->stream));
        e->own_stream = false;
    }
    e->stream = nullptr;   // hipStream_t 0: the legacy default stream
    return ALS_OK;
}

int als_factor_stride(const als_engine* e) { return e ? e->kp : 0; }

}  // extern "C"

namespace {

int ensure_stage(als_engine* e) {
    constexpr size_t STAGE = 32u << 20;
    if (!e->h_stage) {
        HIP_TRY(hipHostMalloc(&e->h_stage, STAGE, hipHostMallocDefault));
        e->stage_bytes = STAGE;
    }
    return ALS_OK;
}

int check_block_shape(als_engine* e, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows) {
    if (n_rows < 0 || row_offset < 0 || n_opp_rows < 0)
        return fail(ALS_ERR_INVALID_ARGUMENT, "negative size (n_rows=%lld row_offset=%lld n_opp_rows=%lld)",
                    (long long)n_rows, (long long)row_offset, (long long)n_opp_rows);
    if (n_rows > INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "n_rows exceeds 2^31-1");
    if (n_opp_rows >= INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "n_opp_rows must be < 2^31-1 (int32 column indices)");
    if ((n_opp_rows + 1) * (int64_t)e->kp * (int64_t)e->elem() > (int64_t)UINT32_MAX)
        return fail(ALS_ERR_UNSUPPORTED, "opposite factor matrix exceeds 4 GiB (32-bit gather offsets)");
    return ALS_OK;
}

// Padded entries of a row of degree d (every row starts on a 32-entry block).
inline int64_t padded(int64_t d) { return (d + cfk::BLOCK_ENTRIES - 1) / cfk::BLOCK_ENTRIES * cfk::BLOCK_ENTRIES; }

// Replace the device copy *dst of a task list (nullptr for an empty list).
int upload_tasks(Task** dst, const std::vector<Task>& src) {
    if (*dst) {
        (void)hipFree(*dst);
        *dst = nullptr;
    }
    const size_t bytes = src.size() * sizeof(Task);
    if (bytes == 0) return ALS_OK;
    hipError_t st = hipMalloc((void**)dst, bytes);
    if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "hipMalloc(%zu): %s", bytes, hipGetErrorString(st));
    st = hipMemcpy(*dst, src.data(), bytes, hipMemcpyHostToDevice);
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "hipMemcpy: %s", hipGetErrorString(st));
    return ALS_OK;
}

// The device side of a block whose padded in-block (d_col / d_rat, device, already laid out) has row degrees deg[]
// and row starts begin[]: plans it (als_plan.h: layout, then the task lists), permutes the interleaved rows' blocks,
// packs the pre-split operands, uploads the plan, takes ownership of d_col / d_rat and sizes the partial and pre-split
// workspaces.
int finish_block(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows, int64_t nnz,
                 const std::vector<int64_t>& deg, const std::vector<int64_t>& begin, int32_t* d_col, float* d_rat) {
    const int64_t nnz_padded = begin[n_rows];
    auto drop = [&]() {
        (void)hipFree(d_col);
        (void)hipFree(d_rat);
    };
    cfk::BlockShape shape;
    shape.path = e->path;
    shape.k = e->k;
    shape.kp = e->kp;
    shape.cu_count = e->cu_count;
    shape.n_opp_rows = n_opp_rows;
    const cfk::BlockLayout layout = cfk::plan_layout(e->cfg.plan, shape, deg);
    std::vector<int32_t> bfirst;   // opposite slot of every block's first entry (physical position 0 of the block)
    if (layout.ranges && nnz_padded > 0) {
        bfirst.resize((size_t)(nnz_padded / cfk::BLOCK_ENTRIES));
        hipError_t st = hipMemcpy2D(bfirst.data(), 4, d_col, cfk::BLOCK_ENTRIES * 4, 4, bfirst.size(),
                                    hipMemcpyDeviceToHost);
        if (st != hipSuccess) {
            drop();
            return fail(ALS_ERR_DEVICE, "set_block: block heads: %s", hipGetErrorString(st));
        }
    }
    cfk::BlockPlan plan = cfk::plan_build(e->cfg.plan, shape, layout, deg, begin, bfirst);
    if (plan.error) {
        drop();
        return fail(ALS_ERR_UNSUPPORTED, "%s", plan.error);
    }

    hipError_t st0 = hipSetDevice(e->device);
    if (st0 == hipSuccess) st0 = hipStreamSynchronize(e->stream);
    if (st0 == hipSuccess && !plan.perm.empty()) {
        // the long rows' blocks chunk-major (before the pre-split packing below derives its arrays from them)
        int32_t *d_perm = nullptr, *col2 = nullptr;
        float* rat2 = nullptr;
        st0 = hipMalloc((void**)&d_perm, plan.perm.size() * 4);
        if (st0 == hipSuccess) st0 = hipMalloc((void**)&col2, (size_t)nnz_padded * 4);
        if (st0 == hipSuccess) st0 = hipMalloc((void**)&rat2, (size_t)nnz_padded * 4);
        if (st0 == hipSuccess) st0 = hipMemcpy(d_perm, plan.perm.data(), plan.perm.size() * 4, hipMemcpyHostToDevice);
        if (st0 == hipSuccess)
            st0 = cfk::launch_permute_blocks(d_col, d_rat, col2, rat2, d_perm, (int64_t)plan.perm.size(), nullptr);
        if (st0 == hipSuccess) st0 = hipDeviceSynchronize();
        (void)hipFree(d_perm);
        if (st0 == hipSuccess) {
            std::swap(d_col, col2);
            std::swap(d_rat, rat2);
        }
        (void)hipFree(col2);
        (void)hipFree(rat2);
    }
    if (st0 != hipSuccess) {
        drop();
        return fail(ALS_ERR_DEVICE, "set_block: %s", hipGetErrorString(st0));
    }
    Block& blk = e->blk[side];
    free_block(blk);
    blk.d_col = d_col;
    blk.d_rat = d_rat;
    blk.n_rows = n_rows;
    blk.row_offset = row_offset;
    blk.n_opp_rows = n_opp_rows;
    blk.nnz = nnz;
    blk.nnz_padded = nnz_padded;
    blk.layout = layout;
    blk.n_tasks = (int32_t)plan.tasks.size();
    blk.n_reduce = (int32_t)plan.reduce.size();
    blk.n_slots = (int32_t)plan.slots;
    blk.ilv_rows = plan.ilv_rows;
    blk.ilv_tasks = plan.ilv_tasks;
    if (layout.presplit) {
        // the pre-split copy of the opposite table (cfk::launch_presplit_prepare, once per half), sized for the
        // larger side
        const int64_t sb = (n_opp_rows + 1) * (int64_t)cfk::presplit_row_bytes(e->kp);
        if ((size_t)sb > e->split_bytes) {
            (void)hipFree(e->d_split);
            e->d_split = nullptr;
            e->split_bytes = 0;
            hipError_t st = hipMalloc(&e->d_split, (size_t)sb);
            if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "pre-split hipMalloc(%lld): %s", (long long)sb,
                                              hipGetErrorString(st));
            e->split_bytes = (size_t)sb;
        }
        if (nnz_padded > 0) {
            // the RHS operand's ratings, packed once (setup time): fp16 rh pairs, then rm pairs
            hipError_t st = hipMalloc((void**)&blk.d_rat_pk, (size_t)nnz_padded * 4);
            if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "hipMalloc(%lld): %s", (long long)nnz_padded * 4,
                                              hipGetErrorString(st));
            st = cfk::launch_pack_ratings(blk.d_rat, blk.d_rat_pk, nnz_padded / 2, nullptr);
            // and the column indices in the order of the LDS-DMA gather (one 16-B load per loader row)
            if (st == hipSuccess) st = hipMalloc((void**)&blk.d_col_ps, (size_t)nnz_padded * 4);
            if (st == hipSuccess) st = cfk::launch_pack_cols_ps(blk.d_col, blk.d_col_ps, nnz_padded, nullptr);
            if (st == hipSuccess) st = hipDeviceSynchronize();
            if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "pack ratings: %s", hipGetErrorString(st));
        }
    }
    if (int r = upload_tasks(&blk.d_tasks, plan.tasks)) return r;
    if (int r = upload_tasks(&blk.d_reduce, plan.reduce)) return r;
    for (int c = 0; c < 3; ++c) {
        if (int r = upload_tasks(&blk.d_dual[c], plan.dual[c])) return r;
        blk.n_dual[c] = (int32_t)plan.dual[c].size();
        blk.h_dual[c] = std::move(plan.dual[c]);
    }
    if (int r = upload_tasks(&blk.d_sq_tasks, plan.sq_all)) return r;
    blk.n_sq = (int32_t)plan.sq_all.size();
    if (blk.n_sq > 0) HIP_TRY(hipMalloc((void**)&blk.d_task_se, plan.sq_all.size() * sizeof(double)));
    blk.h_tasks = std::move(plan.tasks);
    blk.h_reduce = std::move(plan.reduce);
    // Partial workspace sized for the larger side (the generic path: its per-workgroup Gram slabs, when the packed
    // triangle does not fit in LDS -- up to 1024 workgroups within 4 GiB)
    size_t need = (size_t)plan.slots * cfk::partial_words_per_lane(e->precision, e->kp, e->path) * 64 * e->elem();
    if (e->path == Path::GENERIC) {
        const cfk::GenericPlan gp = cfk::generic_plan(e->precision, e->kp);
        if (!gp.g_in_lds) {
            const int64_t slab = gp.slab_elems * (int64_t)e->elem();
            e->generic_slabs = std::max<int64_t>(1, std::min<int64_t>(1024, (4ll << 30) / slab));
            need = (size_t)(e->generic_slabs * slab);
        }
    }
    if (need > e->partial_bytes) {
        (void)hipFree(e->d_partials);
        e->d_partials = nullptr;
        e->partial_bytes = 0;
        hipError_t st = hipMalloc(&e->d_partials, need);
        if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "partials hipMalloc(%zu): %s", need, hipGetErrorString(st));
        e->partial_bytes = need;
    }
    blk.set = true;
    return ALS_OK;
}

}  // namespace

extern "C" {

int als_set_block(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows,
                  const int64_t* row_ptr, const int32_t* col_idx, const int16_t* ratings) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (int r = check_block_shape(e, n_rows, row_offset, n_opp_rows)) return r;
    if (n_rows > 0 && !row_ptr) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr is NULL");
    const int64_t nnz = n_rows > 0 ? row_ptr[n_rows] : 0;
    if (n_rows > 0 && row_ptr[0] != 0) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr[0] must be 0");
    if (nnz > 0 && (!col_idx || !ratings)) return fail(ALS_ERR_INVALID_ARGUMENT, "col_idx/ratings NULL");
    // Validate the block on the host: a bad index would fault the GPU.
    std::vector<int64_t> deg(n_rows), begin(n_rows + 1);
    int64_t o = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t d = row_ptr[i + 1] - row_ptr[i];
        if (d < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "row_ptr not monotone at row %lld", (long long)i);
        if (d > INT32_MAX / 2) return fail(ALS_ERR_UNSUPPORTED, "row %lld has %lld entries", (long long)i, (long long)d);
        deg[i] = d;
        begin[i] = o;
        o += padded(d);
    }
    begin[n_rows] = o;
    for (int64_t t = 0; t < nnz; ++t)
        if (col_idx[t] < 0 || col_idx[t] >= n_opp_rows)
            return fail(ALS_ERR_INVALID_ARGUMENT, "col_idx[%lld]=%d outside [0, %lld)", (long long)t, col_idx[t],
                        (long long)n_opp_rows);
    // Padded, block-interleaved device in-block (see cfk::block_position): every row starts on a
    // 32-entry block; padding entries point at the sentinel zero row (col = n_opp_rows) with rating 0.
    std::vector<int32_t> col(o, (int32_t)n_opp_rows);
    std::vector<float> rat(o, 0.f);
    for (int64_t i = 0; i < n_rows; ++i)
        for (int64_t t = 0; t < deg[i]; ++t) {
            const int64_t pos = begin[i] + cfk::block_position(t);
            col[pos] = col_idx[row_ptr[i] + t];
            rat[pos] = (float)ratings[row_ptr[i] + t];
        }
    HIP_TRY(hipSetDevice(e->device));
    int32_t* d_col = nullptr;
    float* d_rat = nullptr;
    if (o > 0) {
        hipError_t st = hipMalloc((void**)&d_col, o * 4);
        if (st == hipSuccess) st = hipMalloc((void**)&d_rat, o * 4);
        if (st == hipSuccess) st = hipMemcpy(d_col, col.data(), o * 4, hipMemcpyHostToDevice);
        if (st == hipSuccess) st = hipMemcpy(d_rat, rat.data(), o * 4, hipMemcpyHostToDevice);
        if (st != hipSuccess) {
            (void)hipFree(d_col);
            (void)hipFree(d_rat);
            return fail(ALS_ERR_OUT_OF_MEMORY, "in-block upload: %s", hipGetErrorString(st));
        }
    }
    return finish_block(e, side, n_rows, row_offset, n_opp_rows, nnz, deg, begin, d_col, d_rat);
}

int als_set_block_coo(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows, int64_t nnz,
                      const int32_t* rows, const int32_t* cols, const int16_t* ratings) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (int r = check_block_shape(e, n_rows, row_offset, n_opp_rows)) return r;
    if (nnz < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "nnz < 0");
    if (nnz > 0 && (!rows || !cols || !ratings)) return fail(ALS_ERR_INVALID_ARGUMENT, "rows/cols/ratings NULL");
    if (nnz >= INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "nnz per block must be < 2^31-1 (shard the side)");
    HIP_TRY(hipSetDevice(e->device));
    std::vector<int64_t> deg, begin;
    int32_t* d_col = nullptr;
    float* d_rat = nullptr;
    std::string err;
    const int code = cfk::build_block_device(rows, cols, ratings, nnz, n_rows, n_opp_rows, e->stream, deg, begin,
                                             &d_col, &d_rat, err);
    if (code != ALS_OK) return fail(code, "als_set_block_coo: %s", err.c_str());
    return finish_block(e, side, n_rows, row_offset, n_opp_rows, nnz, deg, begin, d_col, d_rat);
}

int als_alloc_factors(als_engine* e, int side, int64_t n_total_rows) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (n_total_rows < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "n_total_rows < 0");
    HIP_TRY(hipSetDevice(e->device));
    Factors& f = e->fac[side];
    if (f.owned) (void)hipFree(f.ptr);
    f = Factors();
    const size_t bytes = (size_t)(n_total_rows + 1) * e->kp * e->elem();   // + sentinel zero row
    hipError_t st = hipMalloc(&f.ptr, bytes);
    if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "factors hipMalloc(%zu): %s", bytes, hipGetErrorString(st));
    f.owned = true;
    f.n_rows = n_total_rows;
    HIP_TRY(hipMemsetAsync(f.ptr, 0, bytes, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ALS_OK;
}

int als_bind_factors(als_engine* e, int side, void* device_ptr, int64_t n_total_rows) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (!device_ptr || n_total_rows < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "bad device buffer");
    Factors& f = e->fac[side];
    if (f.owned) (void)hipFree(f.ptr);
    f.ptr = device_ptr;
    f.n_rows = n_total_rows;
    f.owned = false;
    // the sentinel row after the last factor row must read as zeros (padding entries gather it). The buffer's
    // owner may still have work on it queued on another stream (e.g. torch's zero fill): drain the device first,
    // so the memset and every later engine access are ordered after it.
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync((char*)device_ptr + (size_t)n_total_rows * e->kp * e->elem(), 0, (size_t)e->kp * e->elem(),
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ALS_OK;
}

int als_factors_device_ptr(const als_engine* e, int side, void** device_ptr, int64_t* n_total_rows) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (device_ptr) *device_ptr = e->fac[side].ptr;
    if (n_total_rows) *n_total_rows = e->fac[side].n_rows;
    return ALS_OK;
}

int als_write_factors(als_engine* e, int side, int64_t row0, int64_t n_rows, const void* host_src, int64_t src_ld) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Factors& f = e->fac[side];
    if (!f.ptr) return fail(ALS_ERR_STATE, "factors of side %d not allocated/bound", side);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > f.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "row range out of bounds");
    if (src_ld < e->k) return fail(ALS_ERR_INVALID_ARGUMENT, "src_ld (%lld) < num_features (%d)", (long long)src_ld, e->k);
    if (n_rows == 0) return ALS_OK;
    if (!host_src) return fail(ALS_ERR_INVALID_ARGUMENT, "host_src is NULL");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    const size_t es = e->elem();
    // Rows are packed kp wide (padding columns zero) into pinned staging and written by a copy kernel
    // (cfk::launch_upload) on the engine's stream: see copy16 in als_kernels.hip.
    const size_t row_bytes = (size_t)e->kp * es;
    if (int r = ensure_stage(e)) return r;
    HIP_TRY(hipStreamSynchronize(e->stream));   // the staging buffer may still feed an earlier copy
    const int64_t rows_per = (int64_t)(e->stage_bytes / row_bytes);
    for (int64_t r = 0; r < n_rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, n_rows - r);
        char* stage = (char*)e->h_stage;
        const char* src = (const char*)host_src + (size_t)r * src_ld * es;
        for (int64_t i = 0; i < nr; ++i) {
            std::memcpy(stage + i * row_bytes, src + (size_t)i * src_ld * es, (size_t)e->k * es);
            std::memset(stage + i * row_bytes + (size_t)e->k * es, 0, row_bytes - (size_t)e->k * es);
        }
        HIP_TRY(cfk::launch_upload(stage, (char*)f.ptr + (size_t)(row0 + r) * row_bytes, (size_t)nr * row_bytes,
                                   e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));   // the staging buffer is reused by the next chunk
    }
    return ALS_OK;
}

int als_read_factors(als_engine* e, int side, int64_t row0, int64_t n_rows, void* host_dst, int64_t dst_ld) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Factors& f = e->fac[side];
    if (!f.ptr) return fail(ALS_ERR_STATE, "factors of side %d not allocated/bound", side);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > f.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "row range out of bounds");
    if (dst_ld < e->k) return fail(ALS_ERR_INVALID_ARGUMENT, "dst_ld (%lld) < num_features (%d)", (long long)dst_ld, e->k);
    if (n_rows == 0) return ALS_OK;
    if (!host_dst) return fail(ALS_ERR_INVALID_ARGUMENT, "host_dst is NULL");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = sync_checked(e)) return r;
    const size_t es = e->elem();
    // Read back the way the kernels wrote: a copy kernel (cfk::launch_download) moves whole kp-wide rows into
    // pinned staging, the host keeps the first k columns; the same path as als_write_factors in reverse.
    const size_t row_bytes = (size_t)e->kp * es;
    if (int r = ensure_stage(e)) return r;
    const int64_t rows_per = (int64_t)(e->stage_bytes / row_bytes);
    for (int64_t r = 0; r < n_rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, n_rows - r);
        HIP_TRY(cfk::launch_download((const char*)f.ptr + (size_t)(row0 + r) * row_bytes, e->h_stage,
                                     (size_t)nr * row_bytes, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const char* stage = (const char*)e->h_stage;
        char* dst = (char*)host_dst + (size_t)r * dst_ld * es;
        for (int64_t i = 0; i < nr; ++i)
            std::memcpy(dst + (size_t)i * dst_ld * es, stage + i * row_bytes, (size_t)e->k * es);
    }
    return ALS_OK;
}

namespace {

// One half (or one chunk of it): the FULL + PARTIAL launch, then the REDUCE launch.
struct DualLaunch {
    const Task* t[3] = {nullptr, nullptr, nullptr};
    int32_t n[3] = {0, 0, 0};
};

int launch_half(als_engine* e, int side, float lambda, const Task* tasks, int32_t n_tasks, const Task* reduce,
                int32_t n_reduce, bool first_chunk, const DualLaunch& dl) {
    Block& b = e->blk[side];
    const Factors& self = e->fac[side];
    const Factors& opp = e->fac[1 - side];
    if (!self.ptr || !opp.ptr) return fail(ALS_ERR_STATE, "als_solve_half: factor matrices not allocated/bound");
    if (b.n_rows > 0 && b.factor_row(b.n_rows - 1) >= self.n_rows)
        return fail(ALS_ERR_STATE, "block rows (last at factor row %lld) exceed factor rows %lld",
                    (long long)b.factor_row(b.n_rows - 1), (long long)self.n_rows);
    if (b.n_opp_rows != opp.n_rows)   // the padding entries gather row n_opp_rows: it must be the sentinel
        return fail(ALS_ERR_STATE, "block was set for %lld opposite rows, the opposite factor matrix has %lld",
                    (long long)b.n_opp_rows, (long long)opp.n_rows);
    if (!(lambda >= 0.f)) return fail(ALS_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
    HIP_TRY(hipSetDevice(e->device));
    // the solve reads the opposite replica: wait for its all-gather; a whole half / first chunk also rewrites
    // this side's rows, which an earlier all-gather of this side may still be sending
    if (int r = wait_gathers(e, side == ALS_SIDE_USER || first_chunk, side == ALS_SIDE_MOVIE || first_chunk)) return r;
    cfk::SolveArgs a{};
    a.tasks = tasks;
    a.n_tasks = n_tasks;
    a.k = e->k;
    a.col = b.d_col;
    a.rat = b.d_rat;
    a.opp = opp.ptr;
    a.out = self.ptr;
    a.row_offset = b.row_offset;
    a.rows_per_chunk = (int32_t)b.rows_per_chunk;
    a.chunk_stride = b.chunk_stride;
    a.partials = e->d_partials;
    a.scratch_slabs = e->generic_slabs;
    a.lambda = lambda;
    a.sentinel = (int32_t)b.n_opp_rows;
    a.flags = e->path == Path::VALU ? 0 : e->cfg.debug_flags;
    if (++e->gen == 0) e->gen = 1;
    a.gen = e->cfg.debug_fixed_gen ? 1u : e->gen;
    a.integrity = e->d_integrity;
    a.refine_min_pivot = e->cfg.refine_min_pivot;
    a.extra_lds = e->cfg.debug_extra_lds;
    TimingRec rec{side, {nullptr, nullptr, nullptr}};
    if (e->timing) {
        for (auto& ev : rec.ev) {
            if (!e->ev_pool.empty()) {
                ev = e->ev_pool.back();
                e->ev_pool.pop_back();
            } else {
                HIP_TRY(hipEventCreate(&ev));
            }
        }
        HIP_TRY(hipEventRecord(rec.ev[0], e->stream));
    }
    const bool any_dual = dl.n[0] > 0 || dl.n[1] > 0 || dl.n[2] > 0;
    const bool side_dual = any_dual && e->cfg.dual_side;
    if (side_dual) {   // the dual launches read the fp32 opposite table only: fork before the pre-split
        if (!e->side_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&e->fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&e->join, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(e->fork, e->stream));
    }
    if (b.layout.presplit) {
        // the opposite replica is the half's input and does not change between its chunks (als.h): chunk 0
        // converts it, later chunks reuse the conversion and its range words. The two sets of range words alternate
        // per preparation: each preparation zeroes the other set, which the launches of the half before it read.
        if (first_chunk) {
            e->prep_set ^= 1;
            HIP_TRY(cfk::launch_presplit_prepare(e->kp, (const float*)opp.ptr, e->d_split, b.n_opp_rows + 1,
                                                 e->d_prep + e->prep_set * cfk::PREP_SET_WORDS,
                                                 e->d_prep + (e->prep_set ^ 1) * cfk::PREP_SET_WORDS,
                                                 e->d_prep + 2 * cfk::PREP_SET_WORDS + side, e->cu_count, e->stream));
        }
        a.opp_split = e->d_split;
        a.rat_pk = b.d_rat_pk;
        a.rat_lo_off = b.nnz_padded / 2;
        a.col_ps = b.d_col_ps;
        a.amax = e->d_prep + e->prep_set * cfk::PREP_SET_WORDS;
    }
    HIP_TRY(cfk::launch_solve(e->precision, e->kp, e->path, a, e->stream, b.layout.presplit, false));
    if (b.layout.presplit) {
        // the range guard's fallback: the same tasks on the fp32 table with the on-the-fly split, a launch whose
        // waves exit at once unless the opposite table is out of the pre-split's range (cfk::presplit_ok)
        cfk::SolveArgs f = a;
        f.presplit_fallback = 1;
        f.grid_cap = 4 * e->cu_count;
        // (on the main stream: on the side stream, ahead of the entry-space launches, the step was slower)
        HIP_TRY(cfk::launch_solve(e->precision, e->kp, e->path, f, e->stream, false, false));
    }
    if (side_dual) HIP_TRY(hipStreamWaitEvent(e->side_stream, e->fork, 0));
    for (int c = 0; c < 3; ++c)
        if (dl.n[c] > 0) {
            cfk::SolveArgs d = a;
            d.tasks = dl.t[c];
            d.n_tasks = dl.n[c];
            HIP_TRY(cfk::launch_dual(e->kp, 2 * (c + 1), d, side_dual ? e->side_stream : e->stream));
        }
    if (side_dual) {
        HIP_TRY(hipEventRecord(e->join, e->side_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->join, 0));
    }
    if (e->timing) HIP_TRY(hipEventRecord(rec.ev[1], e->stream));
    if (n_reduce > 0) {
        a.tasks = reduce;
        a.n_tasks = n_reduce;
        a.gen += e->cfg.debug_gen_skew;
        HIP_TRY(cfk::launch_solve(e->precision, e->kp, e->path, a, e->stream, false, true));
    }
    if (e->timing) {
        HIP_TRY(hipEventRecord(rec.ev[2], e->stream));
        e->pending.push_back(rec);
    }
    return ALS_OK;
}

}  // namespace

int als_solve_half(als_engine* e, int side, float lambda) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_solve_half: no block set for side %d", side);
    DualLaunch dl;
    for (int c = 0; c < 3; ++c) {
        dl.t[c] = b.d_dual[c];
        dl.n[c] = b.n_dual[c];
    }
    return launch_half(e, side, lambda, b.d_tasks, b.n_tasks, b.d_reduce, b.n_reduce, true, dl);
}

int als_set_chunks(als_engine* e, int side, int n_chunks, const int64_t* row_bounds) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_set_chunks: no block set for side %d", side);
    if (n_chunks < 1 || !row_bounds) return fail(ALS_ERR_INVALID_ARGUMENT, "n_chunks must be >= 1 with row_bounds");
    if (row_bounds[0] != 0 || row_bounds[n_chunks] != b.n_rows)
        return fail(ALS_ERR_INVALID_ARGUMENT, "row_bounds must run from 0 to n_rows (%lld)", (long long)b.n_rows);
    for (int c = 0; c < n_chunks; ++c)
        if (row_bounds[c + 1] < row_bounds[c]) return fail(ALS_ERR_INVALID_ARGUMENT, "row_bounds not monotone");
    // stable partition by chunk keeps the longest-first order inside every chunk
    std::vector<Task> ct, cr, cdl[3];
    cfk::partition_by_chunk(b.h_tasks, n_chunks, row_bounds, ct, b.coff);
    cfk::partition_by_chunk(b.h_reduce, n_chunks, row_bounds, cr, b.croff);
    for (int c = 0; c < 3; ++c) cfk::partition_by_chunk(b.h_dual[c], n_chunks, row_bounds, cdl[c], b.cdoff[c]);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int r = upload_tasks(&b.d_ctasks, ct)) return r;
    if (int r = upload_tasks(&b.d_creduce, cr)) return r;
    for (int c = 0; c < 3; ++c)
        if (int r = upload_tasks(&b.d_cdual[c], cdl[c])) return r;
    return ALS_OK;
}

int als_solve_half_chunk(als_engine* e, int side, float lambda, int chunk) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set || b.coff.empty()) return fail(ALS_ERR_STATE, "als_solve_half_chunk: no chunks set for side %d", side);
    if (chunk < 0 || chunk + 1 >= (int)b.coff.size())
        return fail(ALS_ERR_INVALID_ARGUMENT, "chunk %d out of range (%d chunks)", chunk, (int)b.coff.size() - 1);
    DualLaunch dl;
    for (int c = 0; c < 3; ++c) {
        dl.t[c] = b.d_cdual[c] + b.cdoff[c][chunk];
        dl.n[c] = b.cdoff[c][chunk + 1] - b.cdoff[c][chunk];
    }
    return launch_half(e, side, lambda, b.d_ctasks + b.coff[chunk], b.coff[chunk + 1] - b.coff[chunk],
                       b.d_creduce + b.croff[chunk], b.croff[chunk + 1] - b.croff[chunk], chunk == 0, dl);
}

int als_predict(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows,
                int64_t n_movies, float* host_out) {
    if (int r = check_engine(e)) return r;
    if (n_users < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (n_users == 0 || n_movies == 0) return ALS_OK;
    if (!user_rows || !movie_rows || !host_out) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    const Factors& U = e->fac[ALS_SIDE_USER];
    const Factors& M = e->fac[ALS_SIDE_MOVIE];
    if (!U.ptr || !M.ptr) return fail(ALS_ERR_STATE, "als_predict: factor matrices not allocated/bound");
    for (int64_t i = 0; i < n_users; ++i)
        if (user_rows[i] < 0 || user_rows[i] >= U.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "user row out of range");
    for (int64_t i = 0; i < n_movies; ++i)
        if (movie_rows[i] < 0 || movie_rows[i] >= M.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "movie row out of range");
    if ((n_users + 15) / 16 > 65535) return fail(ALS_ERR_UNSUPPORTED, "at most 1,048,560 users per call (call per user range)");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    int64_t *d_u = nullptr, *d_m = nullptr;
    float* d_out = nullptr;
    const size_t ob = (size_t)n_users * (size_t)n_movies * sizeof(float);
    auto cleanup = [&]() {
        (void)hipFree(d_u);
        (void)hipFree(d_m);
        (void)hipFree(d_out);
    };
    hipError_t st = hipMalloc((void**)&d_u, n_users * sizeof(int64_t));
    if (st == hipSuccess) st = hipMalloc((void**)&d_m, n_movies * sizeof(int64_t));
    if (st == hipSuccess) st = hipMalloc((void**)&d_out, ob);
    if (st != hipSuccess) {
        cleanup();
        return fail(ALS_ERR_OUT_OF_MEMORY, "als_predict: hipMalloc: %s", hipGetErrorString(st));
    }
    st = hipMemcpyAsync(d_u, user_rows, n_users * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_m, movie_rows, n_movies * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
        st = cfk::launch_predict(e->precision, U.ptr, M.ptr, e->kp, e->k, d_u, n_users, d_m, n_movies, d_out, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(host_out, d_out, ob, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    cleanup();
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "als_predict: %s", hipGetErrorString(st));
    return sync_checked(e);
}

int als_recommend_plan(const als_engine* e, int64_t n_users, int64_t n_movies, int top_n, int64_t info[4]) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n_users < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (top_n < 1 || top_n > cfk::REC_MAX_TOP_N)
        return fail(ALS_ERR_INVALID_ARGUMENT, "top_n must be 1..%d, got %d", cfk::REC_MAX_TOP_N, top_n);
    const cfk::RecommendPlan p = cfk::recommend_plan(n_users, n_movies, top_n, e->kp, e->cu_count);
    info[0] = p.user_tile;
    info[1] = p.segments;
    info[2] = p.seg_len;
    info[3] = p.lds_bytes;
    return ALS_OK;
}

int als_recommend(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                  int top_n, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* host_idx, float* host_score) {
    if (int r = check_engine(e)) return r;
    if (n_users < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (top_n < 1 || top_n > cfk::REC_MAX_TOP_N)
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: top_n must be 1..%d, got %d", cfk::REC_MAX_TOP_N, top_n);
    if ((excl_ptr == nullptr) != (excl_idx == nullptr))
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: excl_ptr and excl_idx must both be given or both be NULL");
    if (n_movies > INT32_MAX) return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: n_movies must be below 2^31");
    const Factors& U = e->fac[ALS_SIDE_USER];
    const Factors& M = e->fac[ALS_SIDE_MOVIE];
    if (!U.ptr || !M.ptr) return fail(ALS_ERR_STATE, "als_recommend: factor matrices not allocated/bound");
    if (n_users == 0 || n_movies == 0) return ALS_OK;
    if (!user_rows || !movie_rows || !host_idx || !host_score) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    for (int64_t i = 0; i < n_users; ++i)
        if (user_rows[i] < 0 || user_rows[i] >= U.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "user row out of range");
    for (int64_t i = 0; i < n_movies; ++i)
        if (movie_rows[i] < 0 || movie_rows[i] >= M.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "movie row out of range");
    int64_t ex0 = 0, ex_nnz = 0;
    if (excl_ptr) {   // O(nnz): ranges in order, positions strictly ascending per user and inside the candidate set
        ex0 = excl_ptr[0];
        if (ex0 < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: excl_ptr[0] is negative");
        for (int64_t u = 0; u < n_users; ++u) {
            const int64_t lo = excl_ptr[u], hi = excl_ptr[u + 1];
            if (hi < lo) return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: excl_ptr decreases at user %lld", (long long)u);
            for (int64_t x = lo; x < hi; ++x) {
                if (excl_idx[x] < 0 || excl_idx[x] >= n_movies)
                    return fail(ALS_ERR_INVALID_ARGUMENT, "als_recommend: excluded position %d of user %lld is outside [0, %lld)",
                                (int)excl_idx[x], (long long)u, (long long)n_movies);
                if (x > lo && excl_idx[x] <= excl_idx[x - 1])
                    return fail(ALS_ERR_INVALID_ARGUMENT,
                                "als_recommend: excluded positions of user %lld are not strictly ascending", (long long)u);
            }
        }
        ex_nnz = excl_ptr[n_users] - ex0;
    }
    const cfk::RecommendPlan p = cfk::recommend_plan(n_users, n_movies, top_n, e->kp, e->cu_count);
    if (p.lds_bytes > cfk::REC_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "als_recommend: launch plan exceeds the LDS");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t off_eptr = p.workspace_bytes;
    const int64_t off_eidx = off_eptr + (excl_ptr ? align((n_users + 1) * 8) : 0);
    const size_t need = (size_t)(off_eidx + (excl_ptr ? align(ex_nnz * 4) : 0));
    if (need > e->rec_bytes) {   // grow-only; the stream may still be reading the old one
        HIP_TRY(hipStreamSynchronize(e->stream));
        (void)hipFree(e->d_rec);
        e->d_rec = nullptr;
        e->rec_bytes = 0;
        const hipError_t st = hipMalloc(&e->d_rec, need);
        if (st != hipSuccess)
            return fail(ALS_ERR_OUT_OF_MEMORY, "als_recommend: hipMalloc(%zu): %s", need, hipGetErrorString(st));
        e->rec_bytes = need;
    }
    char* w = (char*)e->d_rec;
    int64_t* d_u = (int64_t*)(w + p.off_urows);
    int64_t* d_m = (int64_t*)(w + p.off_mrows);
    int32_t* d_idx = (int32_t*)(w + p.off_idx);
    float* d_score = (float*)(w + p.off_score);
    float* d_ps = (float*)(w + p.off_part_score);
    int32_t* d_pp = (int32_t*)(w + p.off_part_pos);
    int64_t* d_eptr = excl_ptr ? (int64_t*)(w + off_eptr) : nullptr;
    int32_t* d_eidx = excl_ptr ? (int32_t*)(w + off_eidx) : nullptr;
    std::vector<int64_t> eptr0;   // the device ranges index the uploaded slice: rebased to 0
    hipError_t st = hipMemcpyAsync(d_u, user_rows, n_users * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_m, movie_rows, n_movies * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess && excl_ptr) {
        const int64_t* src = excl_ptr;
        if (ex0 != 0) {
            eptr0.resize(n_users + 1);
            for (int64_t u = 0; u <= n_users; ++u) eptr0[u] = excl_ptr[u] - ex0;
            src = eptr0.data();
        }
        st = hipMemcpyAsync(d_eptr, src, (n_users + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
        if (st == hipSuccess && ex_nnz > 0)
            st = hipMemcpyAsync(d_eidx, excl_idx + ex0, ex_nnz * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    }
    if (st == hipSuccess)
        st = cfk::launch_recommend(e->precision, U.ptr, M.ptr, e->kp, e->k, d_u, n_users, d_m, n_movies, top_n, p, d_eptr,
                                   d_eidx, d_ps, d_pp, d_score, d_idx, e->stream);
    const size_t ob = (size_t)n_users * (size_t)top_n * 4;
    if (st == hipSuccess) st = hipMemcpyAsync(host_idx, d_idx, ob, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(host_score, d_score, ob, hipMemcpyDeviceToHost, e->stream);
    // the host arrays (eptr0 too) are pageable: the stream has to pass the copies before this call returns
    const hipError_t st2 = hipStreamSynchronize(e->stream);
    if (st == hipSuccess) st = st2;
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "als_recommend: %s", hipGetErrorString(st));
    return sync_checked(e);
}

int als_sq_error(als_engine* e, int side, double* sum_sq_error, int64_t* count) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_sq_error: no block set for side %d", side);
    const Factors& self = e->fac[side];
    const Factors& opp = e->fac[1 - side];
    if (!self.ptr || !opp.ptr) return fail(ALS_ERR_STATE, "als_sq_error: factor matrices not allocated/bound");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    cfk::SqErrArgs a{};
    a.tasks = b.d_sq_tasks;
    a.n_tasks = b.n_sq;
    a.col = b.d_col;
    a.rat = b.d_rat;
    a.opp = opp.ptr;
    a.self = self.ptr;
    a.row_offset = b.row_offset;
    a.rows_per_chunk = (int32_t)b.rows_per_chunk;
    a.chunk_stride = b.chunk_stride;
    a.task_se = b.d_task_se;
    a.sentinel = (int32_t)b.n_opp_rows;
    HIP_TRY(cfk::launch_sq_error(e->precision, e->kp, a, e->stream));
    std::vector<double> se(b.n_sq);
    if (b.n_sq > 0)
        HIP_TRY(hipMemcpyAsync(se.data(), b.d_task_se, se.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (int r = sync_checked(e)) return r;
    double s = 0.0;
    for (double v : se) s += v;   // fixed (task) order: deterministic
    if (sum_sq_error) *sum_sq_error = s;
    if (count) *count = b.nnz;
    return ALS_OK;
}

int als_synchronize(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    return sync_checked(e);
}

int als_integrity_status(als_engine* e, uint32_t* record, int reset) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    if (int r = stream_wait(e, e->stream)) return r;
    uint32_t rec[cfk::INTEGRITY_WORDS];
    HIP_TRY(hipMemcpy(rec, e->d_integrity, sizeof(rec), hipMemcpyDeviceToHost));
    if (record) std::memcpy(record, rec, sizeof(rec));
    if (reset) HIP_TRY(hipMemset(e->d_integrity, 0, sizeof(rec)));
    return ALS_OK;
}

int als_set_timing(als_engine* e, int enabled) {
    if (int r = check_engine(e)) return r;
    e->timing = enabled != 0;
    return ALS_OK;
}

int als_timing_collect(als_engine* e, int side, double* ms_gram, double* ms_reduce, int64_t* n_calls) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    HIP_TRY(hipSetDevice(e->device));
    double g = 0, rd = 0;
    int64_t n = 0;
    std::vector<TimingRec> keep;
    for (auto& rec : e->pending) {
        if (rec.side != side) {
            keep.push_back(rec);
            continue;
        }
        HIP_TRY(hipEventSynchronize(rec.ev[2]));
        float m1 = 0, m2 = 0;
        HIP_TRY(hipEventElapsedTime(&m1, rec.ev[0], rec.ev[1]));
        HIP_TRY(hipEventElapsedTime(&m2, rec.ev[1], rec.ev[2]));
        g += m1;
        rd += m2;
        ++n;
        for (auto ev : rec.ev) e->ev_pool.push_back(ev);
    }
    e->pending.swap(keep);
    if (ms_gram) *ms_gram = g;
    if (ms_reduce) *ms_reduce = rd;
    if (n_calls) *n_calls = n;
    return ALS_OK;
}

int als_debug_copy_partials(als_engine* e, void* host_dst, int64_t max_bytes, int64_t* bytes) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int64_t n = std::min<int64_t>(max_bytes, (int64_t)e->partial_bytes);
    if (bytes) *bytes = (int64_t)e->partial_bytes;
    if (host_dst && n > 0) HIP_TRY(hipMemcpy(host_dst, e->d_partials, (size_t)n, hipMemcpyDeviceToHost));
    return ALS_OK;
}

// ---- multi-GPU exchange (RCCL over xGMI) ---------------------------------------------------------------
#define NCCL_TRY(expr)                                                                                     \
    do {                                                                                                   \
        ncclResult_t _r = (expr);                                                                          \
        if (_r != ncclSuccess)                                                                             \
            return fail(ALS_ERR_COMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(_r), __FILE__,     \
                        __LINE__);                                                                         \
    } while (0)

static int comm_streams(als_engine* e) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamCreateWithFlags(&e->comm_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&e->solved, hipEventDisableTiming));
    for (auto& ev : e->gathered) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return ALS_OK;
}

// Caller-level RCCL groups (als_comm_group_start / _end, one host thread driving several engines): inside a
// group a collective is only placed on its stream at the OUTERMOST ncclGroupEnd, so the "gathered" event of an
// all-gather issued inside a group must be recorded after that end, not at the call (recorded earlier it would
// order nothing). The thread's open-group depth and the (engine, side) pairs whose record is deferred:
thread_local int g_group_depth = 0;
thread_local std::vector<std::pair<als_engine*, int>> g_group_gathers;

static int record_gathered(als_engine* e, int side) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(e->gathered[side], e->comm_stream));
    e->gather_pending[side] = true;
    return ALS_OK;
}

int als_comm_unique_id(void* id_out, int nbytes) {
    if (!id_out || nbytes < (int)sizeof(ncclUniqueId))
        return fail(ALS_ERR_INVALID_ARGUMENT, "unique id buffer must hold %d bytes", (int)sizeof(ncclUniqueId));
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return ALS_OK;
}

int als_comm_init(als_engine* e, int world, int rank, const void* unique_id) {
    if (int r = check_engine(e)) return r;
    if (world < 1 || rank < 0 || rank >= world || !unique_id)
        return fail(ALS_ERR_INVALID_ARGUMENT, "bad world/rank/unique_id (world %d, rank %d)", world, rank);
    if (e->comm) return fail(ALS_ERR_STATE, "engine already has a communicator");
    HIP_TRY(hipSetDevice(e->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    NCCL_TRY(ncclCommInitRank(&e->comm, world, id, rank));
    e->world = world;
    e->rank = rank;
    return comm_streams(e);
}

int als_comm_init_group(als_engine** engines, int n) {
    if (!engines || n < 1) return fail(ALS_ERR_INVALID_ARGUMENT, "need >= 1 engines");
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        if (int r = check_engine(engines[i])) return r;
        if (engines[i]->comm) return fail(ALS_ERR_STATE, "engine %d already has a communicator", i);
        devs[i] = engines[i]->device;
        for (int j = 0; j < i; ++j)
            if (devs[j] == devs[i]) return fail(ALS_ERR_INVALID_ARGUMENT, "engines %d and %d share device %d", j, i, devs[i]);
    }
    std::vector<ncclComm_t> comms(n);
    NCCL_TRY(ncclCommInitAll(comms.data(), n, devs.data()));
    for (int i = 0; i < n; ++i) {
        engines[i]->comm = comms[i];
        engines[i]->world = n;
        engines[i]->rank = i;
        if (int r = comm_streams(engines[i])) return r;
    }
    return ALS_OK;
}

int als_comm_info(const als_engine* e, int* world, int* rank) {
    if (int r = check_engine(e)) return r;
    if (world) *world = e->world;
    if (rank) *rank = e->rank;
    return ALS_OK;
}

int als_comm_group_start(void) {
    NCCL_TRY(ncclGroupStart());
    ++g_group_depth;
    return ALS_OK;
}

int als_comm_group_end(void) {
    if (g_group_depth <= 0) return fail(ALS_ERR_STATE, "als_comm_group_end without als_comm_group_start");
    const ncclResult_t r = ncclGroupEnd();
    if (--g_group_depth > 0) {
        if (r != ncclSuccess) return fail(ALS_ERR_COMM, "ncclGroupEnd failed: %s", ncclGetErrorString(r));
        return ALS_OK;
    }
    // outermost end: the grouped all-gathers are on their streams now; record their events behind them
    std::vector<std::pair<als_engine*, int>> touched;
    touched.swap(g_group_gathers);
    if (r != ncclSuccess) return fail(ALS_ERR_COMM, "ncclGroupEnd failed: %s", ncclGetErrorString(r));
    for (auto& eg : touched)
        if (int rc = record_gathered(eg.first, eg.second)) return rc;
    return ALS_OK;
}

int als_allgather_shard(als_engine* e, int side, int64_t slots_per_chunk, int64_t chunk) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (e->world == 1 && !e->comm) return ALS_OK;   // one shard: the replica is the matrix
    if (!e->comm) return fail(ALS_ERR_STATE, "als_allgather_shard: no communicator (als_comm_init)");
    const Factors& f = e->fac[side];
    if (!f.ptr) return fail(ALS_ERR_STATE, "factors of side %d not allocated/bound", side);
    const int64_t Sc = slots_per_chunk;
    if (Sc < 0 || chunk < 0 || (chunk + 1) * Sc * e->world > f.n_rows)
        return fail(ALS_ERR_INVALID_ARGUMENT, "chunk %lld of %lld slots per shard x %d shards exceeds %lld rows",
                    (long long)chunk, (long long)Sc, e->world, (long long)f.n_rows);
    if (Sc == 0) return ALS_OK;
    HIP_TRY(hipSetDevice(e->device));
    // after this engine's solve (stream) on comm_stream; the next solve that reads this side waits for it
    HIP_TRY(hipEventRecord(e->solved, e->stream));
    HIP_TRY(hipStreamWaitEvent(e->comm_stream, e->solved, 0));
    const ncclDataType_t dt = e->precision == ALS_F64 ? ncclFloat64 : ncclFloat32;
    const size_t row = (size_t)e->kp * e->elem();
    // chunk-major slots: chunk c holds the G shards' Sc-row pieces back to back, so its exchange is ONE
    // contiguous in-place all-gather
    char* cbase = (char*)f.ptr + (size_t)chunk * (size_t)(Sc * e->world) * row;
    e->last_gather_side = side;
    e->last_gather_chunk = chunk;
    e->last_gather_rows = Sc;
    NCCL_TRY(ncclAllGather(cbase + (size_t)e->rank * Sc * row, cbase, (size_t)Sc * e->kp, dt, e->comm,
                           e->comm_stream));
    if (g_group_depth > 0) {   // placed on the stream at the outermost group end: record the event there
        g_group_gathers.emplace_back(e, side);
        return ALS_OK;
    }
    return record_gathered(e, side);
}

int als_set_row_layout(als_engine* e, int side, int64_t rows_per_chunk, int64_t chunk_stride) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_set_row_layout: no block set for side %d", side);
    if (rows_per_chunk < 0 || (rows_per_chunk > 0 && chunk_stride < rows_per_chunk) || rows_per_chunk > INT32_MAX)
        return fail(ALS_ERR_INVALID_ARGUMENT, "rows_per_chunk %lld / chunk_stride %lld", (long long)rows_per_chunk,
                    (long long)chunk_stride);
    b.rows_per_chunk = rows_per_chunk;
    b.chunk_stride = rows_per_chunk > 0 ? chunk_stride : 0;
    return ALS_OK;
}

int als_comm_wait(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    return wait_gathers(e, true, true);
}

int als_comm_set_timeout(als_engine* e, int64_t timeout_ms) {
    if (int r = check_engine(e)) return r;
    e->cfg.comm_timeout_ms = timeout_ms;
    return ALS_OK;
}

int als_block_path(const als_engine* e, int side, int* gram_path, int* presplit, int64_t* chunk, int64_t* n_dual_rows) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Block& b = e->blk[side];
    if (gram_path) *gram_path = (int)e->path;
    if (presplit) *presplit = b.layout.presplit ? 1 : 0;
    if (chunk) *chunk = b.set ? b.layout.chunk : 0;
    if (n_dual_rows)
        for (int c = 0; c < 3; ++c) n_dual_rows[c] = b.n_dual[c];
    return ALS_OK;
}

int als_block_stats(const als_engine* e, int side, int64_t* n_tasks, int64_t* n_reduce, int64_t* nnz_padded) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Block& b = e->blk[side];
    if (n_tasks) *n_tasks = b.n_tasks + b.n_dual[0] + b.n_dual[1] + b.n_dual[2];
    if (n_reduce) *n_reduce = b.n_reduce;
    if (nnz_padded) *nnz_padded = b.nnz_padded;
    return ALS_OK;
}

int als_block_split_info(const als_engine* e, int side, int64_t info[4]) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (!info) return fail(ALS_ERR_INVALID_ARGUMENT, "info is NULL");
    const Block& b = e->blk[side];
    info[0] = b.ilv_rows;
    info[1] = b.ilv_tasks;
    info[2] = b.layout.ilv;
    info[3] = b.layout.presplit ? 1 : 0;
    return ALS_OK;
}

}  // extern "C"

#ifdef CFK_DEBUG_KNOBS
// Debug build only (not in include/als.h): present iff the work-dropping / fault-injection knobs are compiled in
// (bench.py refuses a library that exports it, whatever its path).
extern "C" int als_debug_knobs_compiled(void) { return 1; }
#endif
