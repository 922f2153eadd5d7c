// als_engine.cpp -- the C ABI of include/als.h, first of four units (als_engine_impl.h names the others): engine
// lifetime, the environment, streams, synchronisation and the integrity record, timing, introspection. See
// include/als.h for the reference interface each entry point replaces.
#include <chrono>
#include <cstdlib>
#include <memory>
#include <thread>

#include "als_engine_impl.h"

namespace cfk_detail {

int check_engine(const als_engine* e) {
    if (!e) return fail(ALS_ERR_INVALID_ARGUMENT, "engine is NULL");
    return ALS_OK;
}

int wait_gathers(als_engine* e, bool movie, bool user) {
    const bool want[2] = {movie, user};
    for (int s = 0; s < 2; ++s)
        if (want[s] && e->gather_pending[s]) {
            HIP_TRY(hipStreamWaitEvent(e->stream, e->gathered[s], 0));
            e->gather_pending[s] = false;
        }
    return ALS_OK;
}

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

// Drain the engine's stream (and the all-gathers before it) and read the integrity record.
static int drain_integrity(als_engine* e, uint32_t rec[cfk::INTEGRITY_WORDS]) {
    if (int r = wait_gathers(e, true, true)) return r;
    if (int r = stream_wait(e, e->stream)) return r;
    HIP_TRY(hipMemcpy(rec, e->d_integrity.get(), cfk::INTEGRITY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ALS_OK;
}

int sync_checked(als_engine* e) {
    uint32_t rec[cfk::INTEGRITY_WORDS];
    if (int r = drain_integrity(e, rec)) return r;
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

}  // namespace cfk_detail

using namespace cfk_detail;

namespace {

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
    std::unique_ptr<als_engine> e(new als_engine());
    e->device = device;
    e->k = num_features;
    e->kp = kp;
    e->precision = precision;
    e->path = path;
    e->cfg = cfg;
    hipError_t st = e->stream.create();
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "hipStreamCreate: %s", hipGetErrorString(st));
    st = hipDeviceGetAttribute(&e->cu_count, hipDeviceAttributeMultiprocessorCount, device);
    if (st == hipSuccess) st = e->d_integrity.alloc(cfk::INTEGRITY_WORDS);
    if (st == hipSuccess) st = hipMemset(e->d_integrity.get(), 0, e->d_integrity.bytes());
    {   // both sets of range words zero, no side split yet
        uint32_t prep[2 * cfk::PREP_SET_WORDS + 2] = {};
        prep[2 * cfk::PREP_SET_WORDS] = prep[2 * cfk::PREP_SET_WORDS + 1] = cfk::PREP_NO_EXP;
        if (st == hipSuccess) st = e->d_prep.alloc(2 * cfk::PREP_SET_WORDS + 2);
        if (st == hipSuccess) st = hipMemcpy(e->d_prep.get(), prep, sizeof(prep), hipMemcpyHostToDevice);
    }
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "integrity record: %s", hipGetErrorString(st));
    *out = e.release();
    return ALS_OK;
}

int als_engine_destroy(als_engine* e) {
    if (!e) return ALS_OK;
    (void)hipSetDevice(e->device);
    // every stream drained before anything it uses is freed, the communicator gone before its stream; the members'
    // destructors release the rest (als_engine_impl.h: buffers and events first, the streams last)
    (void)hipStreamSynchronize(e->stream);
    if (e->comm_stream) (void)hipStreamSynchronize(e->comm_stream);
    if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);
    if (e->comm) (void)ncclCommDestroy(e->comm);
    delete e;
    return ALS_OK;
}

int als_engine_set_stream(als_engine* e, void* hip_stream) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    if (hip_stream) HIP_TRY(e->stream.borrow((hipStream_t)hip_stream));
    else HIP_TRY(e->stream.create());
    return ALS_OK;
}

int als_engine_use_default_stream(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(e->stream.borrow(nullptr));   // hipStream_t 0: the legacy default stream
    return ALS_OK;
}

int als_factor_stride(const als_engine* e) { return e ? e->kp : 0; }

int als_synchronize(als_engine* e) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    return sync_checked(e);
}

int als_integrity_status(als_engine* e, uint32_t* record, int reset) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    uint32_t rec[cfk::INTEGRITY_WORDS];
    if (int r = drain_integrity(e, rec)) return r;
    if (record) std::memcpy(record, rec, sizeof(rec));
    if (reset) HIP_TRY(hipMemset(e->d_integrity.get(), 0, sizeof(rec)));
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
    // this side's records to the back, in order; they leave `pending` only once all of them were read
    const auto mine = std::stable_partition(e->pending.begin(), e->pending.end(),
                                            [side](const TimingRec& rec) { return rec.side != side; });
    for (auto rec = mine; rec != e->pending.end(); ++rec) {
        HIP_TRY(hipEventSynchronize(rec->ev[2]));
        float m1 = 0, m2 = 0;
        HIP_TRY(hipEventElapsedTime(&m1, rec->ev[0], rec->ev[1]));
        HIP_TRY(hipEventElapsedTime(&m2, rec->ev[1], rec->ev[2]));
        g += m1;
        rd += m2;
        ++n;
    }
    for (auto rec = mine; rec != e->pending.end(); ++rec)
        for (auto& ev : rec->ev) e->ev_pool.push_back(std::move(ev));
    e->pending.erase(mine, e->pending.end());
    if (ms_gram) *ms_gram = g;
    if (ms_reduce) *ms_reduce = rd;
    if (n_calls) *n_calls = n;
    return ALS_OK;
}

int als_debug_copy_partials(als_engine* e, void* host_dst, int64_t max_bytes, int64_t* bytes) {
    if (int r = check_engine(e)) return r;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const int64_t n = std::min<int64_t>(max_bytes, (int64_t)e->d_partials.size());
    if (bytes) *bytes = (int64_t)e->d_partials.size();
    if (host_dst && n > 0) HIP_TRY(hipMemcpy(host_dst, e->d_partials.get(), (size_t)n, hipMemcpyDeviceToHost));
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
        for (int c = 0; c < 3; ++c) n_dual_rows[c] = b.dual[c].size();
    return ALS_OK;
}

int als_block_stats(const als_engine* e, int side, int64_t* n_tasks, int64_t* n_reduce, int64_t* nnz_padded) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Block& b = e->blk[side];
    if (n_tasks) *n_tasks = (int64_t)b.tasks.size() + b.dual[0].size() + b.dual[1].size() + b.dual[2].size();
    if (n_reduce) *n_reduce = b.reduce.size();
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
