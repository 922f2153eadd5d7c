// Internal declarations shared by the engine (als_engine*.cpp, their state: als_engine_impl.h) and the kernels
// (als_kernels.hip, als_recommend.hip, als_similar.hip, als_rank.hip, als_foldin.hip, als_implicit.hip, als_objective.hip, als_build.hip).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "als_plan.h"   // Task, Path, the block layout constants: the HIP-free part
#include "als_resources.h"

namespace cfk {

struct SolveArgs {
    const Task* tasks;
    int32_t n_tasks;
    int32_t k;              // true number of features (<= KP)
    const int32_t* col;     // padded in-block opposite indices (-1 = padding)
    const float* rat;       // padded ratings (0 = padding)
    const void* opp;        // opposite factor matrix [n_opp][KP]
    void* out;              // this side's factor matrix [n_total][KP]
    int64_t row_offset;     // first factor row of this block
    void* partials;         // partial-slot workspace
    float lambda;
    int32_t sentinel;       // index of the opposite side's all-zero sentinel row (= n_opp_rows)
    int32_t flags;          // SOLVE_FLAG_* (diagnostics only; 0 in production)
    const void* opp_split;  // MFMA_SPLIT + presplit: the opposite table as fp16 h/m planes (launch_presplit_prepare)
    uint32_t gen;           // launch generation (PARTIAL and its REDUCE share it): keys the partial-slot encoding
    uint32_t* integrity;    // device record of partial slots that failed their check (see als_slots.h)
    float refine_min_pivot; // MFMA tile solve: skip the refinement step when every scaled pivot >= this (> 1: never)
    const uint32_t* rat_pk; // presplit: the padded ratings r = rh + rm as fp16 pairs (entries 2i, 2i+1): the rh pairs,
                            //   then (at rat_lo_off words) the rm pairs; both exact for every Java short
    const int32_t* col_ps;  // presplit: the padded column indices permuted per block for the LDS-DMA gather
                            //   (launch_pack_cols_ps: lane group r of a block loads its 4 rows with one 16-B load)
    int32_t rows_per_chunk; // chunk-major slots (als_set_row_layout): 0 = factor row row_offset + row, else
    int64_t chunk_stride;   //   row_offset + (row / rows_per_chunk) * chunk_stride + row % rows_per_chunk
    int64_t rat_lo_off;     // presplit: words from the rh pairs to the rm pairs (nnz_padded / 2)
    const uint32_t* amax;   // presplit: range statistics of the opposite table (als_presplit_scan): [0] bits of its largest
                            //   |x| (the split scale), [1] ~bits of its smallest nonzero row maximum
    int32_t presplit_fallback;  // the on-the-fly split launch guarding a pre-split half: it runs only when the table
                                //   is out of the pre-split's range (presplit_ok(amax) false), else exits at once
    int64_t scratch_slabs;  // generic path: workgroup slabs in `partials` (its Gram when it does not fit in LDS)
    int32_t grid_cap;       // workgroups of a grid-stride launch (the range guard's fallback): CUs x 4
    int32_t extra_lds;      // diagnostics (debug build's ALS_DEBUG_EXTRA_LDS, else 0): unused dynamic LDS per workgroup
};
// Cache policy of the buffers a solve launch touches exactly once (load_stream, als_device.h): true = the access
// carries the streaming (non-temporal) policy. One constant per buffer that measured faster with it; every other
// buffer -- the gathered opposite rows, which a launch reuses, and every one-touch stream that measured no gain or a
// loss -- keeps the default policy and has no entry here.
struct CachePolicy {
    static constexpr bool slot_loads = true;   // the REDUCE launch's loads of the partial slots (als_slots.h)
};
// Factor row of local row `row` under the block's slot layout (wave-uniform: scalar arithmetic, once per task).
__host__ __device__ inline int64_t factor_row(int64_t row_offset, int32_t rows_per_chunk, int64_t chunk_stride,
                                              int32_t row) {
    if (rows_per_chunk <= 0) return row_offset + row;
    const int32_t q = row / rows_per_chunk;
    return row_offset + (int64_t)q * chunk_stride + (row - q * rows_per_chunk);
}
// Partial-slot integrity record (device, 4 words): [0] REDUCE tasks that found a bad slot, [1] generation, [2] slot,
// [3] row of the first failure. Read back by every synchronising call of the engine.
constexpr int INTEGRITY_WORDS = 4;
// Diagnostic: skip the k x k solve after the Gram (stores the Gram diagonal instead) -- used by
// tools/kbench.py to split a launch's time into Gram and solve. Only the debug build (CFK_DEBUG_KNOBS) can set
// these flags; the product library never does.
constexpr int32_t SOLVE_FLAG_SKIP_SOLVE = 1;
constexpr int32_t SOLVE_FLAG_SKIP_REFINE = 2;   // diagnostic: no refinement step (accuracy experiments)

struct SqErrArgs {
    const Task* tasks;      // FULL + PARTIAL tasks (they cover every entry exactly once)
    int32_t n_tasks;
    const int32_t* col;
    const float* rat;
    const void* opp;
    const void* self;
    int64_t row_offset;
    double* task_se;        // [n_tasks]
    int32_t sentinel;
    int32_t rows_per_chunk; // slot layout as SolveArgs
    int64_t chunk_stride;
};

// The generic path (als_generic.h) at the geometry of generic_plan(precision, kp) (als_plan.h).
hipError_t launch_generic(int precision, int kp, const SolveArgs& a, hipStream_t s);

// Launch helpers (defined in als_kernels.hip). Return hipSuccess or the launch error.
// The variant (and its occupancy) follows from (precision, kp, path, presplit). presplit: the Gram reads the pre-split
// opposite table (a.opp_split). reduce: `a.tasks` are REDUCE tasks (launched after the FULL/PARTIAL launch of the
// same half).
hipError_t launch_solve(int precision, int kp, Path path, const SolveArgs& a, hipStream_t s, bool presplit,
                        bool reduce);
// Block permutation of the in-block (32-entry blocks): dst block i <- src block perm[i] (cols and ratings).
hipError_t launch_permute_blocks(const int32_t* col, const float* rat, int32_t* col_out, float* rat_out,
                                 const int32_t* perm, int64_t n_blocks, hipStream_t s);
// Short rows in entry space (als_solve_dual): fp32 split path, kp 64 with cd 2, kp 128 with cd 2, 4 or 6 (rows of
// 16 * cd padded entries, i.e. cd / 2 blocks); `a.tasks` are FULL tasks of such rows.
hipError_t launch_dual(int kp, int cd, const SolveArgs& a, hipStream_t s);
// Pre-split of an fp32 [n_rows][kp] factor table (kp = 64 or 128, sentinel row included) into the two fp16 terms
// the presplit Gram stages in LDS: row r = presplit_row_bytes(kp) = 4 kp bytes (the fp32 row's size) at r * 4 kp =
// two planes (h, m) of 2 kp bytes, plane position 16 b + j (b = 0..kp/16-1, j = 0..15) holding feature (kp/16) j + b
// scaled by 2^s, so the 16 values one transposed LDS read hands to a 16-lane group (features (kp/16) j + b,
// j = 0..15) are 32 contiguous bytes, with s = split_exp (als_mfma.h) of the table's largest |x|.
// One preparation is two launches on `s`. als_presplit_scan reads the table once: it splits it at the exponent *pred
// (the one this side's table was last split at) and accumulates the table's range words into set[0..1] (as
// SolveArgs::amax reads them). als_presplit_confirm then compares split_exp(set[0]) with the exponent used; only when
// they differ (or *pred was PREP_NO_EXP) it splits the table again, at the true exponent. It stores that exponent to
// *pred and zeroes next_set[0..1], the set of the next preparation. So dst is always the table split at the
// split_exp of its own maximum, and nothing is read back to the host. set, next_set: PREP_SET_WORDS device words each,
// zeroed once when allocated and then only through next_set, used in turn; cu_count caps both grids.
constexpr int PREP_SET_WORDS = 4;            // [0], [1] the range words, [PREP_EXP] the exponent the scan split at
constexpr int PREP_EXP = 2;
constexpr uint32_t PREP_NO_EXP = 0x7fffffffu;   // *pred before a side's first preparation (no split_exp value)
hipError_t launch_presplit_prepare(int kp, const float* src, void* dst, int64_t n_rows, uint32_t* set,
                                   uint32_t* next_set, uint32_t* pred, int cu_count, hipStream_t s);
// padded column indices -> the per-block order of the presplit gather (n_entries = nnz_padded)
hipError_t launch_pack_cols_ps(const int32_t* col, int32_t* dst, int64_t n_entries, hipStream_t s);
// padded fp32 ratings r -> fp16 pairs of rh = f16(r) at dst[0, n_pairs) and of rm = r - rh at dst[n_pairs, 2 n_pairs)
// (n_pairs = nnz_padded / 2; exact for every integer |r| <= 2^22, so for every Java short)
hipError_t launch_pack_ratings(const float* rat, uint32_t* dst, int64_t n_pairs, hipStream_t s);
// bytes % 16 == 0; host_pinned must stay valid until the stream has passed the copy
hipError_t launch_upload(const void* host_pinned, void* dst, size_t bytes, hipStream_t s);
hipError_t launch_download(const void* src, void* host_pinned, size_t bytes, hipStream_t s);
// out[u][m] = Java-float dot of U row urows[u] and M row mrows[m] (device arrays; out row-major n_u x n_m).
hipError_t launch_predict(int precision, const void* U, const void* M, int kp, int k, const int64_t* urows,
                          int64_t n_u, const int64_t* mrows, int64_t n_m, float* out, hipStream_t s);
// Top-N of the same dots per query user (als_recommend.hip): the scoring kernel sweeps plan.segments candidate
// segments per user tile; one segment writes out_pos / out_score [n_u][top_n] itself, several write the partial lists
// (part_*, [n_u * segments][top_n]) that the merge kernel reduces. excl_ptr / excl_idx: device CSR of excluded
// candidate positions per query user (ascending), or both NULL.
hipError_t launch_recommend(int precision, const void* U, const void* M, int kp, int k, const int64_t* urows,
                            int64_t n_users, const int64_t* mrows, int64_t n_cand, int top_n,
                            const RecommendPlan& plan, const int64_t* excl_ptr, const int32_t* excl_idx,
                            float* part_score, int32_t* part_pos, float* out_score, int32_t* out_pos, hipStream_t s);
// Nearest rows of one factor table (als_similar), all arrays on the device. launch_similar_norms (als_similar.hip):
// inv_q[i] / inv_c[i] = 1 / sqrt(dot of row qrows[i] / crows[i] with itself), 0 for a zero row. launch_similar_sweep
// (als_recommend.hip): launch_recommend's sweep with both row lists in `table`, every score scaled by the two inverse
// norms (both NULL: the plain dot), and -- exclude_self -- without the candidate positions that hold the query's slot.
hipError_t launch_similar_norms(int precision, const void* table, int kp, int k, const int64_t* qrows, int64_t n_queries,
                                const int64_t* crows, int64_t n_cand, float* inv_q, float* inv_c, hipStream_t s);
hipError_t launch_similar_sweep(int precision, const void* table, int kp, int k, const int64_t* qrows, int64_t n_queries,
                                const int64_t* crows, int64_t n_cand, int top_n, const RecommendPlan& plan,
                                const float* inv_q, const float* inv_c, bool exclude_self, float* part_score,
                                int32_t* part_pos, float* out_score, int32_t* out_pos, hipStream_t s);
// Held-out evaluation (als_rank.hip), all arrays on the device. Target entry t = (factor row trow[t] of its user,
// candidate position tpos[t], query-user index tuser[t]). launch_score_pairs: score[t] = the same dot for the pair.
// launch_rank: rank[t] = candidates that come before the target under als_recommend's order (tscore = the scores just
// computed), minus the excluded ones among them (excl_ptr / excl_idx: device CSR per query user, or both NULL; tuser
// is read only with exclusions).
hipError_t launch_score_pairs(int precision, const void* U, const void* M, int kp, int k, const int64_t* trow,
                              const int32_t* tpos, const int64_t* mrows, int64_t n_tgt, float* score, hipStream_t s);
hipError_t launch_rank(int precision, const void* U, const void* M, int kp, int k, const int64_t* trow,
                       const int32_t* tpos, const int32_t* tuser, const float* tscore, int64_t n_tgt,
                       const int64_t* mrows, int64_t n_cand, const RankPlan& plan, const int64_t* excl_ptr,
                       const int32_t* excl_idx, int32_t* rank, hipStream_t s);
// Fold-in (als_foldin.hip), all arrays on the device: query q solves x = (Y^T Y + lambda n I)^-1 Y^T r over the opposite
// rows q_idx[q_ptr[q] .. q_ptr[q + 1]) (q_ptr[0] = 0) with the ratings q_rat, n their count; n = 0 gives zeros. Row q of
// `out` ([n_queries][kp], columns >= k zero) always receives it, and so does row dst_rows[q] of `self` when dst_rows is
// not NULL. kp: 16, 32, 64 or 128, and in fp64 also 80, 96 or 112; the geometry is foldin_plan's (als_plan.h).
struct FoldinArgs {
    const void* opp;          // opposite factor matrix [n_opp][kp], the plain table
    void* self;               // this side's factor matrix (read only with dst_rows)
    void* out;                // [n_queries][kp]
    const int64_t* q_ptr;     // [n_queries + 1]
    const int32_t* q_idx;
    const int16_t* q_rat;
    const int64_t* dst_rows;  // [n_queries] or NULL
    int64_t n_queries;
    int32_t k;
    float lambda;
};
hipError_t launch_fold_in(int precision, int kp, const FoldinArgs& a, const FoldinPlan& plan, hipStream_t s);
// Table Gram (als_implicit.hip): G = Y^T Y of table [n_rows][kp] into the dense symmetric gram [kp][kp] (both triangles,
// padding zero), through `partial` (plan.partial_bytes): the slabs' tiles, summed in ascending slab order (fp32 in
// double, rounded once). The geometry is gram_table_plan's; G does not depend on the device.
hipError_t launch_gram_table(int precision, int kp, const void* table, int64_t n_rows, const GramTablePlan& plan,
                             void* partial, void* gram, hipStream_t s);
// Implicit-feedback solve (als_implicit.hip), arrays as in FoldinArgs: query q solves
// x = (G + alpha sum_e r_e y_e y_e^T + lambda I)^-1 sum_{e: r_e > 0} (1 + alpha r_e) y_e, G the opposite table's Gram
// from launch_gram_table. order[i] is the query the i-th step of the grid-stride loop takes (longest first).
struct ImplicitArgs {
    FoldinArgs f;             // lambda is the plain lambda of the model (not lambda n)
    const void* gram;         // [kp][kp]
    const int64_t* order;     // [n_queries]: a permutation of the queries
    float alpha;
};
hipError_t launch_implicit(int precision, int kp, const ImplicitArgs& a, const FoldinPlan& plan, hipStream_t s);
// The implicit-feedback objective (als_objective.hip), all arrays on the device, q_ptr / q_idx / q_rat / order as in
// ImplicitArgs: parts[q] = {x^T G x, sum_e [(1 + alpha r_e)(p_e - y_e . x)^2 - (y_e . x)^2], lambda x^T x} for x = row
// rows[q] of `self`, in double, and parts[n_queries][0] = lambda tr(G); both over the k true features. The geometry is
// objective_plan's (als_plan.h). Nothing but `parts` is written.
struct ObjectiveArgs {
    const void* opp;          // opposite factor matrix [n_opp][kp], the plain table
    const void* self;         // this side's factor matrix: the rows x are read from
    const void* gram;         // [kp][kp], launch_gram_table's
    const int64_t* q_ptr;     // [n_queries + 1]
    const int32_t* q_idx;
    const int16_t* q_rat;
    const int64_t* rows;      // [n_queries]: factor row of `self` per query (repeats allowed)
    const int64_t* order;     // [n_queries]: a permutation of the queries
    double* parts;            // [3 n_queries + 1]
    int64_t n_queries;
    int32_t k;
    float lambda, alpha;
};
hipError_t launch_objective(int precision, int kp, const ObjectiveArgs& a, const ObjectivePlan& plan, hipStream_t s);
hipError_t launch_sq_error(int precision, int kp, const SqErrArgs& a, hipStream_t s);
// Per-lane accumulator words (elements of the engine precision) of one partial slot: nacc * 64.
int partial_words_per_lane(int precision, int kp, Path path);
// In-block build on the device (als_build.hip): host COO (local row, opposite slot, rating) in arrival order ->
// stable radix sort by row -> the padded block-interleaved d_col / d_rat of als_set_block, row degrees and
// padded row starts back on the host (for the work plan). Returns an als_status; on failure `err` says why and
// d_col / d_rat are empty.
int build_block_device(const int32_t* rows, const int32_t* cols, const int16_t* ratings, int64_t nnz, int64_t n_rows,
                       int64_t n_opp_rows, hipStream_t s, std::vector<int64_t>& deg, std::vector<int64_t>& begin,
                       DeviceBuf<int32_t>& d_col, DeviceBuf<float>& d_rat, std::string& err);
// Host-side check that a (precision, kp, path) variant is compiled in.
bool variant_available(int precision, int kp, Path path);

}  // namespace cfk
