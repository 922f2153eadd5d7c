// The work plan of a block: its task types (shared with the kernels) and the host arithmetic that turns row degrees
// into FULL / PARTIAL / REDUCE tasks (als_plan.cpp). Free of HIP and of the environment: the plan is a function of its
// arguments only, so it builds with any host compiler and is tested on a CPU (tests/test_plan_host.py).
#pragma once
#include <cstdint>
#include <vector>

// Functions the kernels call too; a host compiler sees plain functions.
#ifdef __HIPCC__
#define CFK_HOST_DEVICE __host__ __device__
#else
#define CFK_HOST_DEVICE
#endif

namespace cfk {

// One wave-sized unit of work of a half-iteration (host-built once per uploaded block, README.md:146-147:
// the rating blocks never change, so the work plan is fixed for every iteration).
//   kind FULL    : gather rows [begin, begin + 4*nsteps) of the padded in-block, accumulate Gram + RHS,
//                  regularise, Cholesky-solve, store factor row `row`.
//   kind PARTIAL : same gather/accumulate over one chunk of a long row; store the raw per-lane
//                  accumulators into partial slot `slot` (no solve).
//   kind REDUCE  : sum partial slots [slot, slot + nsteps) of row `row` in fixed order, then solve + store.
enum TaskKind : int32_t { TASK_FULL = 0, TASK_PARTIAL = 1, TASK_REDUCE = 2 };

// Device in-block layout: each row is padded to whole blocks of BLOCK_ENTRIES = 32 entries; padding entries
// hold col = n_opp_rows (the sentinel zero row kept after the last factor row) and rating 0, so they add
// nothing and need no masking in the kernels. Entry e of a
// row is consumed by sub-step t = e / 4 (one MFMA K=4 step) in lane group g = e % 4; inside a block the
// entries are stored group-major ([g][t], t < 8) so that one lane fetches the column indices of its 8
// sub-steps with two 16-byte loads.
constexpr int BLOCK_SUBSTEPS = 8;
constexpr int BLOCK_ENTRIES = 4 * BLOCK_SUBSTEPS;
CFK_HOST_DEVICE constexpr int64_t block_position(int64_t e) {
    const int64_t blk = e / BLOCK_ENTRIES, w = e % BLOCK_ENTRIES;
    return blk * BLOCK_ENTRIES + (w % 4) * BLOCK_SUBSTEPS + w / 4;
}

struct alignas(16) Task {
    int64_t begin;   // entry offset into the padded col/rating arrays (multiple of BLOCK_ENTRIES)
    int32_t nsteps;  // FULL/PARTIAL: sub-steps holding real entries (ceil(n/4)); the task spans
                     // ceil(nsteps / BLOCK_SUBSTEPS) blocks. REDUCE: number of partial slots
    int32_t row;     // local row of the block (factor row = row_offset + row)
    int32_t slot;    // PARTIAL: slot written; REDUCE: first slot read; FULL: -1
    int32_t ndeg;    // true in-block size n_j (lambda * n_j * I, MFeatureCalculator.java:92-95)
    int32_t kind;
    int32_t nent;    // FULL/PARTIAL: real entries in this task's range (logical indices [0, nent))
};
static_assert(sizeof(Task) == 32, "Task layout");

// Gram paths: VALU (LDS-staged, fp32 k < 32 and all fp64), MFMA (v_mfma_f32_16x16x4_f32, exact f32
// products), MFMA_SPLIT (fp32 operands split into narrow terms, fp32 accumulation: fp32-accurate products at a
// multiple of the f32 MFMA rate): on the fly into three bf16 terms (six v_mfma_f32_16x16x32_bf16 partial products
// per tile), or -- presplit -- once per half into a scaled two-term fp16 table (three v_mfma_f32_16x16x32_f16).
// GENERIC: any num_features beyond the wave-per-row kernels (fp32 k > 128, fp64 k > 64): one workgroup per row,
// the Gram's packed lower triangle in LDS (or a per-workgroup global slab) and a workgroup Cholesky.
enum class Path : int { VALU = 0, MFMA = 1, MFMA_SPLIT = 2, GENERIC = 3 };

// Bytes of one row of the pre-split opposite table (als_internal.h, launch_presplit_prepare): the fp32 row's size.
CFK_HOST_DEVICE constexpr int presplit_row_bytes(int kp) { return 4 * kp; }

// Everything the environment can say about the plan (read once per engine by the engine's read_environment, which
// documents each variable). The defaults are the product's behaviour with nothing set.
struct PlanKnobs {
    int interleave = -1;    // ALS_INTERLEAVE: -1 auto, 0 off, 1 wherever the pre-split Gram exists
    int xcd_ranges = -1;    // ALS_XCD_RANGES: -1 auto, 0 off, 1 on (for interleaved halves)
    int presplit = -1;      // ALS_PRESPLIT: -1 auto, 0 off, 1 on (where the pre-split Gram exists)
    bool dual = true;       // ALS_DUAL: short rows in entry space
    int64_t chunk = 0;      // ALS_CHUNK: >= 1 overrides the contiguous chunk length (rounded up to whole blocks)
    // debug build only (CFK_DEBUG_KNOBS)
    int64_t ilv_chunk = 0;  // ALS_ILV_CHUNK: > 0 overrides the interleave length
    enum TaskOrder { LPT = 0, STAGGER = 1, RANDOM = 2 };
    int task_order = LPT;   // ALS_TASK_ORDER
    int64_t stagger_window = 1024;   // ALS_TASK_ORDER=stagger:<W>
};

struct BlockShape {
    Path path = Path::VALU;
    int k = 0, kp = 0;      // features, padded row stride
    int cu_count = 0;       // compute units of the device
    int64_t n_opp_rows = 0; // rows of the opposite factor table (its sentinel row not counted)
};

// How a block's long rows are split and which table its half gathers: decided from the row degrees alone, before the
// plan is built (the engine fetches the block heads from the device only when `ranges` asks for them).
struct BlockLayout {
    int64_t chunk = 0;      // entries per contiguous PARTIAL task of a split row (the generic path never splits)
    int64_t ilv = 0;        // > 0: rows longer than this are split into interleaved chunks of this many entries
    bool ranges = false;    // interleaved rows are cut into 8 opposite-slot ranges, one per XCD
    bool presplit = false;  // the half gathers the pre-split (scaled fp16 h/m) copy of the opposite table
};
BlockLayout plan_layout(const PlanKnobs& knobs, const BlockShape& shape, const std::vector<int64_t>& deg);

struct BlockPlan {
    std::vector<Task> tasks;     // main launch: FULL + PARTIAL in launch order
    std::vector<Task> reduce;    // one REDUCE per split row, longest first
    std::vector<Task> dual[3];   // short rows solved in entry space, by padded blocks - 1, longest first
    std::vector<Task> sq_all;    // every FULL + PARTIAL task incl. the short rows (they cover every entry once)
    std::vector<int32_t> perm;   // in-block block permutation, dst block i <- src block perm[i]; empty: identity
    int64_t slots = 0;           // partial slots
    int64_t ilv_rows = 0, ilv_tasks = 0;   // interleaved rows and their chunk tasks
    const char* error = nullptr; // set when the block cannot be planned (the vectors are then unspecified)
};
// deg[i]: entries of row i; begin[i]: its padded start (begin[n_rows] = padded nnz); bfirst[b]: opposite slot of block
// b's first entry, read only when layout.ranges.
BlockPlan plan_build(const PlanKnobs& knobs, const BlockShape& shape, const BlockLayout& layout,
                     const std::vector<int64_t>& deg, const std::vector<int64_t>& begin,
                     const std::vector<int32_t>& bfirst);

// Stable partition of a task list by the row chunk of each task's row (chunk c = rows [row_bounds[c],
// row_bounds[c + 1])): out = the chunks' tasks back to back, chunk c = out[off[c], off[c + 1]). Keeps the
// longest-first order inside every chunk.
void partition_by_chunk(const std::vector<Task>& in, int n_chunks, const int64_t* row_bounds, std::vector<Task>& out,
                        std::vector<int32_t>& off);

// ---- the any-k path (als_generic.h) ---------------------------------------------------------------------------------
// One 256-thread workgroup per row. Its static LDS is three vectors of the engine's element type: the RHS / solution of
// GENERIC_MAX_KP features plus the pivot, and (fp64 only, else one element each) the refinement's residual and the
// per-entry residuals of a batch of at most GENERIC_MAX_BATCH staged rows. The kernel sizes them with the functions
// below and the plan budgets the dynamic LDS (packed triangle + staged rows) against what they leave, so neither can
// change without the other.
constexpr int GENERIC_MAX_KP = 1024;
constexpr int GENERIC_MAX_BATCH = 64;
constexpr int GENERIC_MIN_LDS_BATCH = 8;           // the Gram stays in LDS only while this many rows still fit beside it
constexpr int64_t GENERIC_SLAB_STAGE_BYTES = 64 * 1024;   // staged rows of the slab variant
constexpr int64_t GENERIC_LDS_LIMIT = 160 * 1024;  // LDS of one gfx950 compute unit
constexpr int64_t GENERIC_LDS_ALIGN = 16;          // the dynamic region is 16-byte aligned: the statics round up to it
CFK_HOST_DEVICE constexpr int generic_vec_elems() { return GENERIC_MAX_KP + 1; }
CFK_HOST_DEVICE constexpr int generic_res_elems(bool f64) { return f64 ? GENERIC_MAX_KP : 1; }
CFK_HOST_DEVICE constexpr int generic_tb_elems(bool f64) { return f64 ? GENERIC_MAX_BATCH : 1; }
// Static LDS of als_solve_generic, alignment padding included: 4112 bytes in fp32, 16912 in fp64.
CFK_HOST_DEVICE constexpr int64_t generic_static_lds_bytes(bool f64) {
    return ((generic_vec_elems() + generic_res_elems(f64) + generic_tb_elems(f64)) * (int64_t)(f64 ? 8 : 4) +
            GENERIC_LDS_ALIGN - 1) / GENERIC_LDS_ALIGN * GENERIC_LDS_ALIGN;
}
// Elements of the packed lower triangle of a kp x kp Gram, rounded up to an even count: the staged rows follow it.
CFK_HOST_DEVICE constexpr int64_t generic_tri_elems(int kp) { return (((int64_t)kp * (kp + 1) / 2) + 1) & ~(int64_t)1; }

// Launch geometry of the generic path for (precision, kp): LDS or slab Gram, staged rows per batch, dynamic LDS.
struct GenericPlan {
    bool g_in_lds;
    int batch;
    int64_t lds_bytes;
    int64_t slab_elems;   // elements per workgroup slab of SolveArgs::partials (0 when the Gram is in LDS)
};
// precision: 0 fp32, 1 fp64; kp: the padded row stride, a multiple of 16 up to GENERIC_MAX_KP.
GenericPlan generic_plan(int precision, int kp);

// ---- top-N recommendation (als_recommend.hip) ----------------------------------------------------------------------
// A 256-thread workgroup owns REC_USER_TILE query users and sweeps the REC_CAND_TILE-candidate tiles of one candidate
// segment, REC_FEAT_CHUNK features staged per pass (row pitch REC_PITCH floats: odd, so the 16 rows a wave reads in
// one step fall into 16 banks). Per user: a sorted best-N list, a threshold and a queue of REC_QUEUE survivors.
constexpr int REC_USER_TILE = 64;
constexpr int REC_CAND_TILE = 64;
constexpr int REC_FEAT_CHUNK = 32;
constexpr int REC_PITCH = REC_FEAT_CHUNK + 1;
constexpr int REC_QUEUE = 32;
constexpr int REC_MAX_TOP_N = 64;
constexpr int64_t REC_MAX_SEGMENTS = 65535;   // gridDim.y
constexpr int64_t REC_LDS_LIMIT = 160 * 1024; // LDS of one gfx950 compute unit
// Dynamic LDS of the scoring kernel in 4-byte words: the two staged tiles, the queues (score, position), the lists
// (score, position), then per user threshold score, threshold position, queue count, list count, and the overflow flag.
CFK_HOST_DEVICE constexpr int64_t recommend_lds_bytes(int top_n) {
    return 4 * ((int64_t)(REC_USER_TILE + REC_CAND_TILE) * REC_PITCH + 2 * (int64_t)REC_USER_TILE * REC_QUEUE +
                2 * (int64_t)REC_USER_TILE * top_n + 4 * (int64_t)REC_USER_TILE + 4);
}

struct RecommendPlan {
    int user_tile = REC_USER_TILE, cand_tile = REC_CAND_TILE;
    int64_t user_tiles = 0;     // workgroups along the users (gridDim.x)
    int64_t segments = 1;       // S: candidate segments (gridDim.y); > 1: partial lists + the merge kernel
    int64_t seg_len = 0;        // candidates per segment: whole candidate tiles, the last segment may be short
    int64_t lds_bytes = 0;      // dynamic LDS of one workgroup
    int64_t partial_rows = 0;   // S > 1: (user, segment) partial lists of top_n (score, position) pairs; else 0
    // byte offsets into the call's workspace (256-byte aligned): user rows, candidate rows (int64), final positions
    // (int32) and scores (float) [n_users][top_n], partial scores and positions [partial_rows][top_n]
    int64_t off_urows = 0, off_mrows = 0, off_idx = 0, off_score = 0, off_part_score = 0, off_part_pos = 0;
    int64_t workspace_bytes = 0;   // all of the above (the exclusion CSR comes on top: it depends on the caller's
                                   // data, not on the shape)
};
// Pure function of its arguments. S = 1 when the user tiles alone give every compute unit a workgroup; otherwise the
// candidates are cut so that user tiles x S reaches 4 workgroups per compute unit (the scoring kernel's occupancy at
// top_n <= 16), at least one candidate tile per segment. kp does not enter today (features are staged in chunks of
// REC_FEAT_CHUNK whatever the row length); it is part of the signature so that a kp-dependent tile can come later.
RecommendPlan recommend_plan(int64_t n_users, int64_t n_cand, int top_n, int kp, int cu_count);

// ---- nearest rows of one table (als_similar: als_recommend.hip's sweep, als_similar.hip's norms) --------------------
// The launch shape is recommend_plan's for (n_queries, n_cand, top_n): the sweep is the same kernel with the same LDS.
// The workspace is that plan's (off_urows = the query rows, off_mrows = the candidate rows) with the two arrays of
// inverse norms (float per query, float per candidate) after it.
struct SimilarPlan {
    RecommendPlan sweep;
    int64_t off_inv_q = 0, off_inv_c = 0;   // byte offsets, 256-byte aligned
    int64_t workspace_bytes = 0;            // the sweep's parts and the two arrays
};
// Pure function of its arguments.
SimilarPlan similar_plan(int64_t n_queries, int64_t n_cand, int top_n, int kp, int cu_count);

// ---- held-out evaluation: exact target ranks (als_rank.hip) ---------------------------------------------------------
// The row dimension of a tile is target entries, not users: a 256-thread workgroup owns RANK_TGT_TILE targets (each with
// its user's factor row) and sweeps the RANK_CAND_TILE-candidate tiles of one candidate segment with the recommend
// kernel's staging (RANK_FEAT_CHUNK features per pass, row pitch RANK_PITCH). Nothing but the two staged tiles is in
// LDS: thresholds and counters live in registers.
constexpr int RANK_TGT_TILE = 64;
constexpr int RANK_CAND_TILE = 64;
constexpr int RANK_FEAT_CHUNK = 32;
constexpr int RANK_PITCH = RANK_FEAT_CHUNK + 1;
constexpr int RANK_WG_PER_CU = 5;              // als_rank_count's occupancy: 92 VGPRs, 5 waves per SIMD, 16.5 KiB of LDS
constexpr int64_t RANK_MAX_SEGMENTS = 65535;   // gridDim.y
constexpr int64_t RANK_LDS_LIMIT = 160 * 1024; // LDS of one gfx950 compute unit
CFK_HOST_DEVICE constexpr int64_t rank_lds_bytes() {
    return 4 * (int64_t)(RANK_TGT_TILE + RANK_CAND_TILE) * RANK_PITCH;
}

struct RankPlan {
    int tgt_tile = RANK_TGT_TILE, cand_tile = RANK_CAND_TILE;
    int64_t tgt_tiles = 0;      // workgroups along the targets (gridDim.x: no 65535 limit)
    int64_t segments = 1;       // S: candidate segments (gridDim.y); > 1: one integer atomicAdd per (target, segment)
    int64_t seg_len = 0;        // candidates per segment: whole candidate tiles, the last segment may be short
    int64_t lds_bytes = 0;      // dynamic LDS of one workgroup
    // byte offsets into the call's workspace (256-byte aligned): per target its user's factor row (int64), candidate
    // position, query-user index (int32), score (float) and rank (int32); then the candidate rows (int64)
    int64_t off_trow = 0, off_tpos = 0, off_tuser = 0, off_score = 0, off_rank = 0, off_mrows = 0;
    int64_t workspace_bytes = 0;   // all of the above (the exclusion CSR comes on top, as in als_recommend)
};
// Pure function of its arguments. S = 1 when the target tiles alone give every compute unit a workgroup; otherwise the
// candidate tiles are cut so that target tiles x S reaches RANK_WG_PER_CU workgroups per compute unit, at least one
// candidate tile per segment. kp does not enter today (as in recommend_plan).
RankPlan rank_plan(int64_t n_targets, int64_t n_cand, int kp, int cu_count);

// ---- fold-in: factor rows of ad-hoc queries (als_foldin.hip) --------------------------------------------------------
// One FOLDIN_THREADS workgroup owns one whole query, grid-stride over the queries. Its dynamic LDS, in elements of the
// engine's type: the Gram's lower-triangle 16 x 16 tiles (row pitch FOLDIN_TILE_PITCH: odd, so a column of the
// factorisation falls into 16 banks), `batch` staged opposite rows of foldin_pitch(kp) elements (pitch = 16 mod 32: the
// 4 entries x 16 features one MFMA operand read touches lie in distinct banks), four kp-vectors (Jacobi scale, Cholesky
// diagonal, substitution broadcast, solution) and the batch's ratings / residuals.
constexpr int FOLDIN_THREADS = 256;
constexpr int FOLDIN_MAX_KP = 128;
constexpr int FOLDIN_MAX_BATCH = 64;
constexpr int FOLDIN_TILE_PITCH = 17;
constexpr int FOLDIN_TILE_ELEMS = 16 * FOLDIN_TILE_PITCH;
constexpr int FOLDIN_MAX_WG_PER_CU = 8;
constexpr int64_t FOLDIN_LDS_LIMIT = 160 * 1024;   // LDS of one gfx950 compute unit
// kp + 16 where kp is a multiple of 32, kp itself where it already is 16 mod 32 (16, and the strides 80 and 112 of fp64
// engines on the generic solve path; 96 takes 112)
CFK_HOST_DEVICE constexpr int foldin_pitch(int kp) { return kp % 32 == 16 ? kp : kp + 16; }
CFK_HOST_DEVICE constexpr int foldin_tiles(int kp) { return (kp / 16) * (kp / 16 + 1) / 2; }
CFK_HOST_DEVICE constexpr int64_t foldin_lds_bytes(int kp, int elem_bytes, int batch) {
    return (int64_t)elem_bytes *
           ((int64_t)foldin_tiles(kp) * FOLDIN_TILE_ELEMS + (int64_t)batch * foldin_pitch(kp) + 4 * kp + batch);
}

struct FoldinPlan {
    int threads = FOLDIN_THREADS;
    int64_t grid = 1;        // workgroups launched: every compute unit filled to its LDS, never more than the queries
    int batch = 0;           // opposite rows staged per pass: a multiple of 4 (one MFMA step), at most FOLDIN_MAX_BATCH
    int64_t lds_bytes = 0;   // dynamic LDS of one workgroup
};
// Pure function of its arguments. kp: 16, 32, 64 or 128, in fp64 also 80, 96 or 112; elem_bytes: 4 or 8. The batch is the largest that fits the LDS
// beside the Gram (FOLDIN_MAX_BATCH for every supported shape); the grid is what the compute units hold at that LDS
// size, at most FOLDIN_MAX_WG_PER_CU each. A query's result does not depend on the grid (one workgroup per query).
FoldinPlan foldin_plan(int kp, int elem_bytes, int64_t n_queries, int cu_count);

// ---- implicit feedback: the table Gram and the implicit solve (als_implicit.hip) ------------------------------------
// Table Gram G = Y^T Y of a whole factor table: slab s owns rows [s rows_per_slab, (s + 1) rows_per_slab) and one
// FOLDIN_THREADS workgroup forms its lower-triangle tiles from batches of FOLDIN_MAX_BATCH rows staged at foldin_pitch;
// a second kernel sums the slabs' tiles in ascending slab order. Slab count and length depend on n_rows alone (never on
// the device), so G is bitwise the same everywhere: the length is GRAM_TABLE_MIN_SLAB_ROWS until that would need more
// than GRAM_TABLE_MAX_SLABS slabs, then the smallest multiple of the batch that keeps the count within the cap.
constexpr int64_t GRAM_TABLE_MAX_SLABS = 1024;
constexpr int64_t GRAM_TABLE_MIN_SLAB_ROWS = 256;
CFK_HOST_DEVICE constexpr int64_t gram_table_lds_bytes(int kp, int elem_bytes) {
    return (int64_t)elem_bytes * ((int64_t)FOLDIN_MAX_BATCH * foldin_pitch(kp) + FOLDIN_MAX_BATCH);
}
struct GramTablePlan {
    int threads = FOLDIN_THREADS;
    int64_t slabs = 1;            // workgroups of the first kernel, at most GRAM_TABLE_MAX_SLABS
    int64_t rows_per_slab = 0;    // a multiple of FOLDIN_MAX_BATCH; the last slab may be short
    int64_t lds_bytes = 0;        // dynamic LDS of one workgroup: one staged batch
    int64_t partial_bytes = 0;    // workspace of the slabs' tiles: slabs x foldin_tiles(kp) x 256 elements
};
// Pure function of kp, elem_bytes and n_rows; cu_count is accepted and ignored (the plan must not depend on the device).
GramTablePlan gram_table_plan(int kp, int elem_bytes, int64_t n_rows, int cu_count);
// The implicit solve has fold-in's launch contract and LDS layout: its plan is foldin_plan's.
inline FoldinPlan implicit_plan(int kp, int elem_bytes, int64_t n_queries, int cu_count) {
    return foldin_plan(kp, elem_bytes, n_queries, cu_count);
}

// ---- implicit feedback: the loss without the grid (als_objective.hip) -----------------------------------------------
// One OBJECTIVE_THREADS workgroup owns one whole query, grid-stride over the queries. Its dynamic LDS is double in both
// precisions: x (kp doubles), then the waves' three sums (OBJECTIVE_RED_SLOTS doubles: [wave][3], rounded up so that the
// byte count stays a multiple of 16). The entries are dealt over groups of objective_group_lanes lanes: the 16-byte
// pieces of a row, rounded up to a power of two (the fp64 strides 80, 96 and 112 have 40, 48 and 56 pieces: 64 lanes).
constexpr int OBJECTIVE_THREADS = 256;
constexpr int OBJECTIVE_RED_SLOTS = 16;
constexpr int OBJECTIVE_WG_PER_CU = 5;   // als_objective_kernel's occupancy: 86 / 90 VGPRs, 5 waves per SIMD
CFK_HOST_DEVICE constexpr int objective_group_lanes(int kp, int elem_bytes) {
    int lanes = 1;
    while (lanes * 16 < kp * elem_bytes) lanes *= 2;
    return lanes;
}
CFK_HOST_DEVICE constexpr int64_t objective_lds_bytes(int kp) { return 8 * (int64_t)(kp + OBJECTIVE_RED_SLOTS); }
struct ObjectivePlan {
    int threads = OBJECTIVE_THREADS;
    int64_t grid = 1;        // workgroups launched: OBJECTIVE_WG_PER_CU per compute unit, never more than the queries
    int64_t lds_bytes = 0;   // dynamic LDS of one workgroup
};
// Pure function of its arguments; kp as in foldin_plan. elem_bytes does not enter the LDS (x is staged as double); it is
// part of the signature because the group width depends on it. A query's result does not depend on the grid.
ObjectivePlan objective_plan(int kp, int elem_bytes, int64_t n_queries, int cu_count);

}  // namespace cfk
