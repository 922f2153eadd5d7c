// als_engine_impl.h -- the engine's state and the helpers its translation units share: als_engine.cpp (lifetime,
// environment, streams, synchronisation, timing, introspection), als_engine_block.cpp (block upload, chunks, row
// layout), als_engine_solve.cpp (factor buffers and their I/O, the half-iteration launch, squared error),
// als_engine_score.cpp (predict, recommend, held-out ranks), als_engine_query.cpp (fold-in, the implicit solve, the
// table Gram) and als_engine_comm.cpp (the RCCL exchange). The synchronous calls of the score and query units share
// one host path, als_engine_call.h, and the checks of their CSR arguments, als_args.h (host-only). Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "als.h"
#include "als_error.h"
#include "als_internal.h"
#include "als_resources.h"

namespace cfk_detail {

using cfk::DeviceBuf;
using cfk::Path;
using cfk::Task;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::cfk_detail::fail(ALS_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr,              \
                                      hipGetErrorString(_e), __FILE__, __LINE__);                  \
    } while (0)

#define NCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t _r = (expr);                                                                  \
        if (_r != ncclSuccess)                                                                     \
            return ::cfk_detail::fail(ALS_ERR_COMM, "%s failed: %s (%s:%d)", #expr,                \
                                      ncclGetErrorString(_r), __FILE__, __LINE__);                 \
    } while (0)

struct TaskSlice {
    const Task* t = nullptr;
    int32_t n = 0;
};

// One task list of a block's work plan in every form the engine uses.
struct TaskList {
    std::vector<Task> host;       // as planned (chunking partitions it)
    DeviceBuf<Task> dev;          // the same, on the device
    DeviceBuf<Task> chunked;      // chunk-major (als_set_chunks; the plan's order inside each chunk)
    std::vector<int32_t> coff;    // chunk c = chunked[coff[c], coff[c + 1]); empty: no chunks set
    int32_t size() const { return (int32_t)host.size(); }
    TaskSlice slice(int chunk) const {   // chunk -1: the whole list
        if (chunk < 0) return {dev.get(), size()};
        return {chunked.get() + coff[chunk], coff[chunk + 1] - coff[chunk]};
    }
};

// The launches of one half, or of one chunk of it.
struct HalfTasks {
    TaskSlice main, reduce, dual[3];
    bool first_chunk = true;   // a whole half, or chunk 0: the launch that prepares the opposite table
};

struct Block {
    bool set = false;
    int64_t n_rows = 0, row_offset = 0, n_opp_rows = 0, nnz = 0, nnz_padded = 0;
    DeviceBuf<int32_t> d_col;
    DeviceBuf<float> d_rat;
    DeviceBuf<uint32_t> d_rat_pk;   // pre-split blocks: ratings as fp16 rh / rm pairs (the Gram's RHS operand)
    DeviceBuf<int32_t> d_col_ps;    // pre-split blocks: column indices in the LDS-DMA gather order
    TaskList tasks;                 // FULL + PARTIAL, sorted by work (longest first)
    TaskList reduce;                // REDUCE
    // short rows solved in entry space (cfk::launch_dual), by entry-tile count cd = 2 (1 block) / 4 (2 blocks) / 6
    TaskList dual[3];
    DeviceBuf<Task> sq_tasks;       // every FULL + PARTIAL task incl. the short rows (als_sq_error)
    DeviceBuf<double> d_task_se;    // per-task squared-error partials
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
    HalfTasks half_tasks(int chunk) const {   // chunk -1: the whole half
        HalfTasks h;
        h.main = tasks.slice(chunk);
        h.reduce = reduce.slice(chunk);
        for (int c = 0; c < 3; ++c) h.dual[c] = dual[c].slice(chunk);
        h.first_chunk = chunk <= 0;
        return h;
    }
};

struct TimingRec {
    int side = 0;
    cfk::Event ev[3];
};

struct Factors {
    void* ptr = nullptr;       // owned.get(), or the caller's buffer (als_bind_factors)
    int64_t n_rows = 0;
    DeviceBuf<char> owned;
};

// What the environment says, read once when an engine is created (read_environment in als_engine.cpp lists the
// variables).
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

}  // namespace cfk_detail

// Members are destroyed in reverse order: everything the streams use is declared after them, so it goes first.
struct als_engine {
    int device = 0;
    int k = 0, kp = 0;
    int precision = ALS_F32;
    cfk::Path path = cfk::Path::VALU;
    cfk::Stream stream;
    cfk::Stream comm_stream;        // all-gathers run here, overlapping the next chunk's solve
    // Entry-space (als_solve_dual) launches run on side_stream, forked from and joined back into `stream`, so
    // they fill the CUs the main launch's tail leaves idle (unless cfg.dual_side is off)
    cfk::Stream side_stream;
    cfk::Event fork, join;
    cfk::Event solved;              // recorded on `stream` before each all-gather
    cfk::Event gathered[2];         // last all-gather of each side, on comm_stream
    cfk_detail::Block blk[2];
    cfk_detail::Factors fac[2];
    cfk::DeviceBuf<char> d_partials;   // partial slots (generic path: its Gram slabs), sized for the larger side
    int64_t generic_slabs = 0;      // generic path: Gram slabs in d_partials
    cfk::DeviceBuf<char> d_split;   // pre-split opposite table (launch_presplit_prepare), sized for the larger need
    cfk::DeviceBuf<uint32_t> d_prep;   // the preparation's device words: two sets of cfk::PREP_SET_WORDS (the range
                                    //   words of the pre-split table, used in turn), then per side the exponent its
                                    //   opposite table was last split at
    int prep_set = 0;               // the set of the last preparation: SolveArgs::amax of the half it served
    cfk::DeviceBuf<char> d_rec;     // the grow-only workspace of the synchronous calls (als_recommend, als_rank_targets,
                                    //   als_fold_in, als_solve_implicit, als_gram_table; als_engine_call.h): none of
                                    //   them is reading it when another starts. Never d_partials / d_split / d_prep,
                                    //   which a half in progress owns
    cfk::PinnedBuf h_stage;         // pinned staging of als_write_factors / als_read_factors (copy kernels)
    cfk::DeviceBuf<uint32_t> d_integrity;   // cfk::INTEGRITY_WORDS: partial slots that failed their check
    int cu_count = 0;               // compute units of the device: the range guard's fallback grid
    cfk_detail::Settings cfg;       // what the environment said when the engine was created (read_environment)
    uint32_t gen = 0;               // launch generation of the next PARTIAL/REDUCE pair
    ncclComm_t comm = nullptr;      // RCCL communicator over the G engines (one per GPU) of a sharded run
    int world = 1, rank = 0;
    bool gather_pending[2] = {false, false};
    int last_gather_side = -1;      // the last all-gather issued (for the timeout's message)
    int64_t last_gather_chunk = -1, last_gather_rows = 0;
    bool timing = false;
    std::vector<cfk::Event> ev_pool;
    std::vector<cfk_detail::TimingRec> pending;
    size_t elem() const { return precision == ALS_F64 ? 8 : 4; }
};

namespace cfk_detail {

int check_engine(const als_engine* e);
int check_side(int side);
// Order the engine's stream after the pending all-gathers of the given sides (comm_stream -> stream).
int wait_gathers(als_engine* e, bool movie, bool user);
// Host wait for a stream of the engine, bounded while the engine has a communicator: on expiry the communicator is
// aborted (so that its kernels end) and the call fails naming the last all-gather issued.
int stream_wait(als_engine* e, hipStream_t s);
// Drain the engine's stream and read the partial-slot integrity record (cfk::SlotCodec): a REDUCE task that
// found a slot it could not see freshly written by this launch's PARTIAL task makes every later synchronising
// call fail until als_integrity_status(..., reset = 1).
int sync_checked(als_engine* e);
// Make sure the pinned staging buffer (h_stage) of the factor I/O and the query read-back exists
// (als_engine_solve.cpp).
int ensure_stage(als_engine* e);
// The first k columns of the nr kp-wide rows in the pinned staging buffer to host_out (row stride out_ld elements).
void unpack_stage(const als_engine* e, int64_t nr, void* host_out, int64_t out_ld);
// The first k columns of n kp-wide device rows to host_out, through the pinned staging buffer in as many passes as it
// takes (als_engine_solve.cpp). Waits for the stream once per pass; `fn` names the call in a failure's message.
int download_rows(als_engine* e, const char* fn, const char* d_rows, int64_t n, void* host_out, int64_t out_ld);

}  // namespace cfk_detail
