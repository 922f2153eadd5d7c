/*
 * als.h -- C ABI of the MI355X-native ALS engine (libcfk_als.so).
 *
 * Drop-in boundary for the reference's one hot path: the per-movie / per-user regularised least-squares
 * feature update that the Kafka Streams processors run
 *     MFeatureCalculator.process   src/main/java/de/hpi/collaborativefilteringkafka/processors/MFeatureCalculator.java:49-136
 *     UFeatureCalculator.process   .../processors/UFeatureCalculator.java:49-136
 * whose arithmetic sits behind EJML CommonOps_FDRM (multTransA / scale / identity / add / invert / mult,
 * MFeatureCalculator.java:85-99). A re-plumbed processor buffers its partition's half-iteration (the EOF
 * barrier, UFeatureInitializer.java:37-41) and makes ONE als_solve_half() call instead of one EJML solve per
 * entity. The JNI / Panama binding a maintainer adds on the Java side is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Plain C types only; every function returns an als_status (0 = ALS_OK) and never throws or longjmps
 *    across the ABI. als_last_error() returns the calling thread's last message. (The reference ignores
 *    EJML invert's boolean, MFeatureCalculator.java:98; this ABI reports failures instead.)
 *  - One engine = one (device, num_features, precision). Engines are independent; one engine must not be
 *    used from two threads at once (the reference runs each task's process() single-threaded,
 *    BaseKafkaApp.java:51, so one engine per stream task / GPU is the intended use).
 *  - "side" selects the entity type whose rows are recomputed: ALS_SIDE_MOVIE rows are solved from user
 *    factors (MFeatureCalculator), ALS_SIDE_USER rows from movie factors (UFeatureCalculator).
 *  - Factor matrices live in device memory with a padded row stride (als_factor_stride(): 16, 32, 64 or
 *    128 elements, or num_features rounded up to 16 beyond that); columns >= num_features are kept at zero.
 */
#ifndef CFK_ALS_H
#define CFK_ALS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALS_ABI_VERSION 3

typedef enum {
    ALS_OK = 0,
    ALS_ERR_INVALID_ARGUMENT = 1,
    ALS_ERR_UNSUPPORTED = 2,
    ALS_ERR_DEVICE = 3,        /* HIP runtime error */
    ALS_ERR_OUT_OF_MEMORY = 4,
    ALS_ERR_STATE = 5,         /* call order violated (e.g. solve before a block was set) */
    ALS_ERR_IO = 6,
    ALS_ERR_PARSE = 7,
    ALS_ERR_DATA = 8,          /* input that hangs the reference (duplicate pair, count mismatch) */
    ALS_ERR_INTEGRITY = 9,     /* a split row's REDUCE task read a partial slot this launch had not written
                                  (als_integrity_status); the results of that half are not trustworthy */
    ALS_ERR_COMM = 10          /* RCCL error (als_comm_*, als_allgather_shard) */
} als_status;

typedef enum { ALS_SIDE_MOVIE = 0, ALS_SIDE_USER = 1 } als_side;
typedef enum { ALS_F32 = 0, ALS_F64 = 1 } als_precision;

typedef struct als_engine als_engine;

/* ---- version / errors --------------------------------------------------------------------------- */
int         als_abi_version(void);
const char* als_last_error(void);
/* sha256 of the sources (csrc/, include/) the library was compiled from, as stamped by the build
 * (__graft_entry__.build); "" for an unstamped developer build. */
const char* als_build_source_sha256(void);
int         als_device_count(int* n);

/* ---- engine lifetime ---------------------------------------------------------------------------- */
/* Replaces the per-task processor state of MFeatureCalculator/UFeatureCalculator.init (:29-46).
 * num_features = ALSApp.NUM_FEATURES (ALSApp.java:18), 1..1024: up to 128 (f64: 64) on the wave-per-row kernels,
 * beyond that on the generic workgroup-per-row path (ALSAppRunner.java:18 accepts any value). */
int als_engine_create(int device, int num_features, int precision, als_engine** out);
int als_engine_destroy(als_engine* e);
/* Launch on a caller-provided hipStream_t (e.g. torch's current stream); NULL = engine-owned stream.
 * Ordering contract: the engine orders its own work on its stream only. A caller that reads or writes a bound
 * factor buffer (als_bind_factors) from other work -- torch ops, RCCL collectives -- must issue that work on
 * the engine's stream or synchronise (als_synchronize) in between. */
int als_engine_set_stream(als_engine* e, void* hip_stream);
/* Launch on the device's NULL (legacy default) stream: the stream torch launches on when no other stream is
 * current (its handle is 0, which als_engine_set_stream would read as "engine-owned"). The engine's kernels are
 * then ordered with torch's work and with RCCL collectives issued against that stream. */
int als_engine_use_default_stream(als_engine* e);
int als_factor_stride(const als_engine* e);

/* ---- in-block upload (constant over all iterations, README.md:146-147) ---------------------------- */
/* Replaces the state stores m-inblocks-uid / m-inblocks-ratings (resp. u-*) that
 * MRatings2BlocksProcessor.java:48-69 / URatings2BlocksProcessor.java:72-92 fill: one CSR row per entity
 * of this partition, entries in in-block order. Row i is solved into factor row (row_offset + i) of
 * `side`; col_idx[] are rows of the opposite side's factor matrix (0 <= col < n_opp_rows).
 * Host pointers; copied to the device once. A failed als_set_block / als_set_block_coo leaves the side's previous
 * block, chunks and row layout set and usable (only ALS_ERR_OUT_OF_MEMORY may unset the blocks of both sides). */
int als_set_block(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows,
                  const int64_t* row_ptr, const int32_t* col_idx, const int16_t* ratings);

/* The same block from COO triples in arrival order (rows[t] = local row, cols[t] = opposite row, ratings[t]):
 * the stable sort into in-block order (= arrival order per row, MRatings2BlocksProcessor.java:53-69) and the
 * padded layout are done on the GPU (radix sort by row), replacing the host-side CSR build for large data.
 * Host pointers; results identical to als_set_block on the equivalent CSR. nnz < 2^31 per call. */
int als_set_block_coo(als_engine* e, int side, int64_t n_rows, int64_t row_offset, int64_t n_opp_rows, int64_t nnz,
                      const int32_t* rows, const int32_t* cols, const int16_t* ratings);

/* ---- factor matrices (device resident) ---------------------------------------------------------- */
/* Engine-owned buffer of n_total_rows x stride elements (zeroed), plus one hidden all-zero sentinel row
 * after the last row (in-block padding entries gather it instead of being masked). */
int als_alloc_factors(als_engine* e, int side, int64_t n_total_rows);
/* Caller-owned device buffer (e.g. a torch tensor) of n_total_rows + 1 rows, row stride =
 * als_factor_stride(e), padding columns zero; the engine zeroes row n_total_rows (the sentinel) here and
 * never writes it, so callers must not either. Lets a collective (RCCL all-gather) write straight into the
 * matrix the engine reads. */
int als_bind_factors(als_engine* e, int side, void* device_ptr, int64_t n_total_rows);
int als_factors_device_ptr(const als_engine* e, int side, void** device_ptr, int64_t* n_total_rows);
/* Host <-> device copies of rows [row0, row0+n_rows) with a host row stride of src_ld/dst_ld elements
 * (>= num_features); element type = float (ALS_F32) or double (ALS_F64). */
int als_write_factors(als_engine* e, int side, int64_t row0, int64_t n_rows, const void* host_src, int64_t src_ld);
int als_read_factors(als_engine* e, int side, int64_t row0, int64_t n_rows, void* host_dst, int64_t dst_ld);

/* ---- THE HOT PATH ------------------------------------------------------------------------------- */
/* For every row j of `side`'s block: gather Y_S = opposite factor rows of its in-block, form
 * A = Y_S^T Y_S + lambda * n_j * I and V = Y_S^T r, solve A m_j = V and store m_j. A is SPD because lambda * n_j > 0:
 * the MFMA paths (fp32 k <= 128, fp64 k <= 64) factor it as a Jacobi-scaled block LDL^T on the 16 x 16 Gram tiles
 * with a pivot-gated refinement step, the generic path (wider k) by Cholesky; EJML's LU inverse (the reference,
 * CommonOps_FDRM.invert) is restated in the oracle. == MFeatureCalculator.java:66-104 / UFeatureCalculator.java:66-104
 * for the whole partition. Asynchronous on the engine's stream. */
int als_solve_half(als_engine* e, int side, float lambda);

/* Row-range chunks of a half (multi-GPU overlap). als_set_chunks splits `side`'s block into n_chunks
 * ranges of its local rows, row_bounds[0] = 0 <= ... <= row_bounds[n_chunks] = n_rows; the union of the
 * chunk launches is exactly als_solve_half. Lets the caller all-gather chunk c of the updated shard over
 * RCCL while chunk c+1 is solved -- the per-partition fan-out of the reference's feature topics
 * (ALSApp.java:105-148) overlapped with compute. Replaces any previous chunking of that side. The chunks of
 * one half are solved in ascending order starting with chunk 0, and the opposite factor replica (the half's
 * input) does not change between them: chunk 0 prepares it (the pre-split copy), later chunks reuse that. A failed
 * als_set_chunks leaves the side's previous chunking as it was. */
int als_set_chunks(als_engine* e, int side, int n_chunks, const int64_t* row_bounds);
int als_solve_half_chunk(als_engine* e, int side, float lambda, int chunk);
/* Chunk-major slot layout of `side`'s rows (after als_set_block, which resets it): local row i is solved into
 * factor row row_offset + (i / rows_per_chunk) * chunk_stride + i % rows_per_chunk (rows_per_chunk = 0: the
 * contiguous row_offset + i). With Sc = rows_per_chunk and chunk_stride = G Sc, the rows of chunk c of every
 * shard are contiguous (als_host.h "Slot layout"). */
int als_set_row_layout(als_engine* e, int side, int64_t rows_per_chunk, int64_t chunk_stride);

/* ---- multi-GPU: shards + RCCL all-gather over xGMI ------------------------------------------------
 * Replaces the per-iteration feature topics (ALSApp.java:105-151): entities are sharded by raw id % G
 * (PureModStreamPartitioner.java:9-10) into chunk-major slots (als_host.h "Slot layout": slot = (r / Sc) G Sc +
 * shard Sc + r % Sc for rank r in the shard, Sc = slots per shard and chunk; one chunk: slot = shard S + r), every
 * engine holds its shard's in-blocks and a full replica of both factor matrices, and each half ends with one
 * all-gather per chunk of the updated shard. One engine per GPU; either one process per GPU (unique id from
 * als_comm_unique_id on one process, shared by the caller, then als_comm_init on every process) or one process
 * driving G GPUs (als_comm_init_group). The exchange is enqueued on the engine's stream after its solve. */
int als_comm_unique_id(void* id_out, int nbytes);   /* nbytes >= 128 */
int als_comm_init(als_engine* e, int world, int rank, const void* unique_id);
int als_comm_init_group(als_engine** engines, int n);
int als_comm_info(const als_engine* e, int* world, int* rank);
/* Gather chunk `chunk` of `side` -- factor rows [chunk G Sc, (chunk + 1) G Sc), this engine's Sc rows at
 * chunk G Sc + rank Sc -- into every engine's replica: one in-place ncclAllGather (Sc = slots_per_chunk; an
 * unchunked side passes its S slots per shard and chunk 0). A single host thread driving several engines
 * wraps its per-engine calls in als_comm_group_start / als_comm_group_end; the engines' completion events are
 * then recorded at the outermost group end, where RCCL places the grouped collectives on their streams. A no-op
 * for an engine without a communicator (G = 1). */
int als_allgather_shard(als_engine* e, int side, int64_t slots_per_chunk, int64_t chunk);
int als_comm_group_start(void);
int als_comm_group_end(void);
/* The all-gathers run on the engine's own communication stream, after the solve that produced the shard and
 * overlapping any later solve that does not depend on them (e.g. the next user-half chunk); the engine orders
 * its next solve of the other side, and every synchronising call, after them. Work issued by the caller on
 * the engine's stream that reads the gathered replicas (e.g. torch ops) must call als_comm_wait first. */
int als_comm_wait(als_engine* e);
/* Bound on every host wait of an engine with a communicator (default 120 000 ms, or ALS_COMM_TIMEOUT_S): a collective
 * that never completes (a peer gone, mismatched calls) would hang the caller of a synchronising call. On expiry the
 * communicator is aborted and the call fails with ALS_ERR_COMM naming the last all-gather issued (side, chunk); the
 * engine is then unusable for the exchange. timeout_ms <= 0: unbounded. (No reference counterpart: the reference's
 * lost messages hang silently, README.md:241; SURVEY.md section 5 asks for a timeout on collectives.) */
int als_comm_set_timeout(als_engine* e, int64_t timeout_ms);

/* FeatureCollector's prediction matrix (FeatureCollector.java:90-101) from the resident factors:
 * host_out[u * n_movies + m] = U[user_rows[u]] . M[movie_rows[m]] as a Java float dot (fp32 products and
 * sums rounded separately, features in order -- EJML multTransB), so the CSV written from it carries the
 * reference's digits. Rows are factor-matrix rows (slots); pass them in ascending-id order for the
 * collector's layout (FeatureCollector.java:72-88). Synchronous. */
int als_predict(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows,
                int64_t n_movies, float* host_out);

/* Top-N recommendation from the resident factors (no reference counterpart: the reference can only write the dense
 * matrix): per query user the top_n best-scoring candidates that are not excluded. Scoring and selection are fused on
 * the GPU; the users x movies matrix is never materialised, and n_users is not limited as in als_predict.
 *  - user_rows / movie_rows: factor rows (slots) of U / M, any order, repeats allowed; n_movies < 2^31.
 *  - Score of (u, c) = exactly als_predict's cell for (user_rows[u], movie_rows[c]), bit for bit.
 *  - Order (total): higher score first, compared as floats (-0.0 == +0.0); equal scores by the smaller candidate
 *    position c (the index into movie_rows). The result is deterministic.
 *  - host_idx[u * top_n + j] = candidate position of the j-th best, host_score its score; a user with fewer than top_n
 *    eligible candidates gets idx -1 / score -INFINITY in the remaining entries. top_n: 1..64.
 *  - excl_idx[excl_ptr[u] .. excl_ptr[u + 1]) = candidate positions excluded for query user u: strictly ascending per
 *    user, in [0, n_movies) (checked on the host, ALS_ERR_INVALID_ARGUMENT). Both NULL: nothing excluded; exactly one
 *    NULL is an error.
 *  - NaN factors are out of contract (no fault; the order among NaN scores is unspecified).
 * Synchronous, on the engine's stream, after pending all-gathers. n_users == 0 or n_movies == 0: ALS_OK, outputs
 * untouched. Uses a grow-only workspace of its own: a call between two chunks of one half leaves the half's prepared
 * pre-split table and partial slots intact. */
int als_recommend(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                  int top_n, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* host_idx, float* host_score);
/* Launch shape als_recommend would choose: info[0] = users per workgroup tile, [1] = candidate segments S (> 1: partial
 * lists per segment, merged by a second kernel), [2] = candidates per segment, [3] = dynamic LDS bytes per workgroup. */
int als_recommend_plan(const als_engine* e, int64_t n_users, int64_t n_movies, int top_n, int64_t info[4]);

/* Nearest rows of ONE factor table (no reference counterpart): "more like this movie", "users like this user". Per query
 * row the top_n best-scoring candidate rows of the same table, by cosine or by dot product, scored and selected in one
 * sweep on the GPU like als_recommend; no n_queries x n_cand matrix is written.
 *  - side: ALS_SIDE_MOVIE or ALS_SIDE_USER, the table both lists index. query_rows / cand_rows: factor rows (slots) of
 *    it, any order, repeats allowed; n_cand < 2^31.
 *  - cell(a, b) = als_predict's cell formula on rows a and b of that table: f64 factors narrowed to float first,
 *    features 0..k-1 in order, every product and every partial sum rounded separately.
 *  - ALS_SIM_DOT:    score(q, c) = cell(q, c).
 *    ALS_SIM_COSINE: score(q, c) = (cell(q, c) * inv(q)) * inv(c) with inv(r) = 1.0f / sqrtf(cell(r, r)), and inv(r) = 0
 *    when cell(r, r) == 0: the square root, the division and the two products are each one correctly rounded fp32
 *    operation, in that order, never contracted. A zero row therefore scores 0 against everything. Being rounded five
 *    times, |score| may exceed 1 by a few ulp and a row's score with itself need not be exactly 1.
 *  - Order and output are als_recommend's: higher score first, compared as floats; equal scores by the smaller
 *    candidate position; deterministic, independent of tiles and segments. host_idx[q * top_n + j] = candidate position
 *    (index into cand_rows) of the j-th best, host_score its score; missing entries are -1 / -INFINITY. top_n: 1..64.
 *  - exclude_self != 0: every candidate position c with cand_rows[c] == query_rows[q] is ineligible for query q (a slot
 *    listed several times among the candidates is left out at all of its positions), under als_recommend's rule for
 *    exclusions: such a cell never competes. Another row with equal factors is not "self".
 *  - NaN or overflowing factors are out of contract (no fault; the order is unspecified).
 * Synchronous, on the engine's stream, after that side's pending all-gathers. n_queries == 0 or n_cand == 0: ALS_OK,
 * outputs untouched. Uses als_recommend's grow-only workspace, never a half's partial slots or pre-split table.
 * ALS_ERR_INVALID_ARGUMENT: bad side, metric or top_n, negative counts, NULL pointers, a row outside [0, rows of the
 * table) (the message names the array and the index). ALS_ERR_STATE: the side's table is not allocated or bound. */
enum { ALS_SIM_COSINE = 0, ALS_SIM_DOT = 1 };
int als_similar(als_engine* e, int side, int metric, const int64_t* query_rows, int64_t n_queries, const int64_t* cand_rows,
                int64_t n_cand, int top_n, int exclude_self, int32_t* host_idx, float* host_score);
/* Launch shape als_similar would choose, as als_recommend_plan reports it: info[0] = queries per workgroup tile, [1] =
 * candidate segments S, [2] = candidates per segment, [3] = dynamic LDS bytes per workgroup. */
int als_similar_plan(const als_engine* e, int64_t n_queries, int64_t n_cand, int top_n, int64_t info[4]);

/* Held-out evaluation from the resident factors (no reference counterpart): for given (user, candidate) pairs -- the
 * targets -- the exact score and the exact rank of the target among the user's candidates. One candidate sweep on the
 * GPU counts what comes before each target; nothing dense is written and nothing is sorted. The rank gives HR@N,
 * NDCG@N, MRR and the percentile rank for every N at once.
 *  - user_rows, movie_rows, excl_ptr, excl_idx: exactly as in als_recommend (n_movies < 2^31; exclusions strictly
 *    ascending per user, in [0, n_movies), checked on the host in O(nnz); both NULL: nothing excluded; exactly one NULL
 *    is an error).
 *  - tgt_idx[tgt_ptr[u] .. tgt_ptr[u + 1]) = the candidate positions (indices into movie_rows) to evaluate for query
 *    user u: any order, repeats allowed, possibly none. Both pointers are required. T = tgt_ptr[n_users] - tgt_ptr[0]
 *    must be below 2^31; a tgt_ptr[0] != 0 is rebased, and the outputs are indexed by the rebased entry t in [0, T).
 *    A decreasing tgt_ptr or a position outside [0, n_movies) is ALS_ERR_INVALID_ARGUMENT, naming the user.
 *  - host_score[t] = exactly als_predict's cell for (user row, movie_rows[target]), bit for bit: the number als_recommend
 *    reports for that cell.
 *  - host_rank[t] = the number of candidate positions c in [0, n_movies) that are not excluded for that user and come
 *    before the target under als_recommend's order: score(c) > score(target) as floats, or equal scores and c < target.
 *    The rank is 0-based. The target never counts itself. The other targets of the same user count like any candidate:
 *    each held-out item is ranked against everything the user has not seen. A target that is itself excluded is still
 *    ranked against the non-excluded candidates.
 *  - host_rank == NULL: scores only -- no candidate sweep, T dots (the held-out RMSE path).
 *  - NaN factors are out of contract, as in als_recommend.
 * Synchronous, on the engine's stream, after pending all-gathers. n_users == 0, T == 0, or n_movies == 0 with ranks
 * requested: ALS_OK, outputs untouched. Uses als_recommend's grow-only workspace (both calls are synchronous): a call
 * between two chunks of one half leaves the half's prepared pre-split table and partial slots intact. */
int als_rank_targets(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                     const int64_t* tgt_ptr, const int32_t* tgt_idx, const int64_t* excl_ptr, const int32_t* excl_idx,
                     float* host_score, int32_t* host_rank);
/* Launch shape als_rank_targets would choose for n_targets target entries: info[0] = targets per workgroup tile, [1] =
 * candidate segments S (> 1: one integer atomic add per target and segment), [2] = candidates per segment, [3] = dynamic
 * LDS bytes per workgroup. */
int als_rank_plan(const als_engine* e, int64_t n_targets, int64_t n_movies, int64_t info[4]);

/* Fold-in: the factor rows of entities that were not in the training block (a user who turns up after training, or
 * whose ratings have changed), from their ratings and the opposite side's resident factors, without retraining:
 * x = (Y^T Y + lambda (float) n I)^-1 Y^T r over the query's n entries -- the normal equation of als_solve_half
 * (MFeatureCalculator.java:85-99) over ad-hoc rows. No block, no work plan, no per-engine state.
 *  - side: the entity type being solved (ALS_SIDE_USER: each query is a user). q_idx[q_ptr[q] .. q_ptr[q + 1]) are
 *    factor rows (slots) of the OPPOSITE side's resident matrix, q_ratings the ratings, typed as in als_set_block.
 *    Entries are used in the order given; a repeated index counts twice, as als_set_block would count it. A
 *    q_ptr[0] != 0 is rebased. The total entry count must be below 2^31.
 *  - A query without entries gives the zero vector, like every other path. lambda as in als_solve_half.
 *  - host_out, if not NULL: row q at host_out + q * out_ld elements (float for ALS_F32, double for ALS_F64),
 *    out_ld >= num_features.
 *  - dst_rows, if not NULL: the result is also stored into factor row dst_rows[q] of `side`'s resident matrix, columns
 *    >= num_features up to the stride zero, bit for bit the host result. No other row and never the sentinel row is
 *    touched. Entries lie in [0, n_total_rows) and do not repeat within a call. Intended use: allocate `side` with
 *    spare rows beyond the trained entities and fold new users into them; als_recommend, als_rank_targets and
 *    als_predict then work on those rows unchanged. The caller must not point dst_rows at rows a half in progress solves.
 *  - At least one of host_out and dst_rows must be given.
 *  - Every num_features whose factor stride is <= 128, in both precisions; wider: ALS_ERR_UNSUPPORTED.
 *  - Checked on the host in O(n_queries + entries), ALS_ERR_INVALID_ARGUMENT naming the query: a decreasing q_ptr, an
 *    index outside [0, opposite n_total_rows), a bad or repeated dst_rows entry. Opposite factors (or, with dst_rows,
 *    `side`'s) not allocated/bound: ALS_ERR_STATE. n_queries == 0: ALS_OK, nothing touched.
 *  - A query's result is bitwise repeatable and does not depend on the other queries of the call, on its position
 *    in the call or on the launch shape: one workgroup owns one whole query and sums in one fixed order.
 * Synchronous, on the engine's stream, after pending all-gathers. Reads the opposite side's plain factor table, never the
 * pre-split copy, and uses als_recommend's grow-only workspace: a call between two chunks of one half leaves that half
 * bitwise unchanged. */
int als_fold_in(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                const int16_t* q_ratings, float lambda, const int64_t* dst_rows, void* host_out, int64_t out_ld);
/* Launch shape als_fold_in would choose: info[0] = threads per workgroup, [1] = workgroups launched, [2] = entries staged
 * per batch, [3] = dynamic LDS bytes per workgroup. */
int als_fold_in_plan(const als_engine* e, int64_t n_queries, int64_t info[4]);

/* Implicit-feedback ALS (Hu, Koren, Volinsky 2008; no reference counterpart: the reference trains on explicit ratings
 * only). Every unobserved pair counts as a weak negative, so a query's system holds the Gram of the whole opposite table:
 *     G = Y^T Y                                      (k x k, all n_total_rows rows of the opposite side's matrix)
 *     A = G + alpha sum_e r_e y_e y_e^T + lambda I   (plain lambda, as in the paper: not lambda n)
 *     b = sum_{e: r_e > 0} (1 + alpha r_e) y_e
 *     x = A^-1 b
 * over the query's entries (i_e, r_e): confidence c = 1 + alpha r, preference p = [r > 0].
 *
 * als_gram_table: Y^T Y of `side`'s own resident table, its k x k leading block to host_out (float for ALS_F32, double
 * for ALS_F64; row stride out_ld >= num_features elements). Row slabs whose count and length depend on the row count
 * alone are multiplied on the matrix pipe at full input precision and summed in ascending slab order (fp32 in double,
 * rounded once), so G is exactly symmetric, bitwise repeatable and the same on every device. Synchronous and diagnostic:
 * it is what als_solve_implicit computes for the opposite side on every call. Factors of `side` not allocated/bound:
 * ALS_ERR_STATE. Factor stride > 128: ALS_ERR_UNSUPPORTED. Uses als_recommend's grow-only workspace. */
int als_gram_table(als_engine* e, int side, void* host_out, int64_t out_ld);
/* Launch shape als_gram_table would choose for a table of n_rows rows: info[0] = threads per workgroup, [1] = slabs
 * (at most 1024), [2] = rows per slab, [3] = dynamic LDS bytes per workgroup. */
int als_gram_table_plan(const als_engine* e, int64_t n_rows, int64_t info[4]);
/* als_solve_implicit: the factor rows x of the model above, for ad-hoc queries or for a whole training half.
 *  - side, n_queries, q_ptr, q_idx, q_ratings, dst_rows, host_out, out_ld: exactly as in als_fold_in (entries used in the
 *    order given, q_ptr[0] != 0 rebased, fewer than 2^31 entries, at least one of host_out and dst_rows, dst_rows bit for
 *    bit the host result with the columns >= num_features zero, no other row and never the sentinel touched).
 *    dst_rows names rows of `side`; the Gram is the OPPOSITE side's, so a call never writes the table it sums.
 *  - Ratings are >= 0; a negative one is ALS_ERR_INVALID_ARGUMENT naming the query. r_e = 0 is allowed and contributes
 *    nothing: the result is bit for bit that of the query without the entry. A repeated index counts twice.
 *  - A query without entries gives the zero vector, written directly with no solve.
 *  - lambda > 0 and alpha > 0, both finite; anything else is ALS_ERR_INVALID_ARGUMENT.
 *  - G of the opposite table is recomputed on every call (als_gram_table's kernels): the engine keeps no state that a
 *    later change of the factors could leave stale.
 *  - Checked on the host in O(n_queries + entries), ALS_ERR_INVALID_ARGUMENT naming the query: a decreasing q_ptr, an
 *    index outside [0, opposite n_total_rows), a bad or repeated dst_rows entry, a negative rating. Factor stride > 128:
 *    ALS_ERR_UNSUPPORTED. Opposite factors (or, with dst_rows, `side`'s) not allocated/bound: ALS_ERR_STATE.
 *    n_queries == 0: ALS_OK, nothing touched.
 *  - A query's result is bitwise repeatable and depends on its own entries, G, lambda and alpha only: not on the other
 *    queries, its position in the call or the launch shape (one workgroup owns one whole query and sums in one fixed
 *    order; the workgroups take the queries longest first).
 * Synchronous, on the engine's stream, after pending all-gathers. Reads the plain factor tables and uses als_recommend's
 * grow-only workspace only: a call between two chunks of an explicit half leaves that half bitwise unchanged. */
int als_solve_implicit(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                       const int16_t* q_ratings, float lambda, float alpha, const int64_t* dst_rows, void* host_out,
                       int64_t out_ld);
/* Launch shape als_solve_implicit would choose: info[] as in als_fold_in_plan. */
int als_solve_implicit_plan(const als_engine* e, int64_t n_queries, int64_t info[4]);
/* als_implicit_objective: the implicit-feedback loss of resident factor rows, without the dense grid. For query q, x =
 * factor row rows[q] of `side`, entries (y_e, r_e) as in als_solve_implicit, G the opposite table's Gram:
 *     f(x) = x^T G x  +  sum_e [ (1 + alpha r_e)(p_e - s_e)^2 - s_e^2 ]  +  lambda x^T x,    s_e = y_e . x,  p_e = [r_e > 0]
 * which is x^T A x - 2 b^T x + sum_{r_e > 0} (1 + alpha r_e) with the A and b of als_solve_implicit: the function whose
 * minimiser that call returns, duplicate entries included. The sum of f over all rows of `side`, plus lambda tr(G), is
 * the loss sum_{u,i} c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2) over the full grid.
 *  - q_ptr, q_idx, q_ratings: exactly als_solve_implicit's, with the same checks (ratings >= 0, lambda and alpha positive
 *    and finite; every message names the query). rows[q] is required and names a row of `side` in [0, n_total_rows); a
 *    row may be listed twice. Nothing is written to either factor table.
 *  - host_parts (NULL, or [n_queries][3] doubles): {x^T G x, sum_e [...], lambda x^T x} per query, the quadratic form and
 *    the ridge over the num_features true features. A query without entries has a middle part of exactly 0; an entry with
 *    r_e = 0 contributes exactly 0; a repeated index counts twice.
 *  - totals[0..2]: the column sums over the queries in ascending query order, summed on the host in double.
 *    totals[3] = lambda tr(G) over the true features, G bit for bit what als_gram_table returns for the opposite side
 *    (recomputed on every call: no per-engine state). totals[0] + [1] + [2] + [3] is the loss over the grid when the
 *    queries are all rows of `side`.
 *  - All device arithmetic after the loads is double in both precisions, in one fixed order without atomics: a query's
 *    three doubles are bitwise repeatable and depend on its entries, x, G, lambda and alpha only.
 *  - n_queries == 0: ALS_OK, totals all zero, no launch. Factor stride > 128: ALS_ERR_UNSUPPORTED. Either factor table
 *    not allocated/bound: ALS_ERR_STATE.
 * Synchronous, on the engine's stream, after pending all-gathers of both sides. Uses als_recommend's grow-only workspace
 * only: a call between two chunks of an explicit half leaves that half bitwise unchanged. */
int als_implicit_objective(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                           const int16_t* q_ratings, const int64_t* rows, float lambda, float alpha, double* host_parts,
                           double totals[4]);
/* Launch shape als_implicit_objective would choose: info[0] = threads per workgroup, [1] = workgroups launched, [2] = 0,
 * [3] = dynamic LDS bytes per workgroup. */
int als_implicit_objective_plan(const als_engine* e, int64_t n_queries, int64_t info[4]);

/* Sum of (r - x_row . y_col)^2 over the block's observed ratings and their count (the RMSE/MSE
 * reduction of scripts/calculate_mse.py:78-90 computed on the device from the factors). Synchronous. */
int als_sq_error(als_engine* e, int side, double* sum_sq_error, int64_t* count);

/* Waits for the engine's stream. Like every synchronising call (als_read_factors, als_sq_error, als_predict)
 * it returns ALS_ERR_INTEGRITY once a REDUCE task has found a partial slot that its PARTIAL task's writes had
 * not reached (each slot is stored keyed by the launch generation with a check word). */
int als_synchronize(als_engine* e);
/* The integrity record: record[0] = REDUCE tasks that found a bad slot so far, record[1..3] = launch generation, slot
 * and local row of the first; reset != 0 clears it. Synchronising. */
int als_integrity_status(als_engine* e, uint32_t* record, int reset);
/* Device-time accounting with HIP events on the engine's stream (non-blocking while enabled): every
 * als_solve_half records its gram/solve launch and its reduce launch; als_timing_collect waits for the
 * recorded events of `side`, returns their summed milliseconds and call count, and clears them. */
int als_set_timing(als_engine* e, int enabled);
int als_timing_collect(als_engine* e, int side, double* ms_gram, double* ms_reduce, int64_t* n_calls);
/* Diagnostics: copies up to max_bytes of the partial-slot workspace (the PARTIAL tasks' encoded sums of the
 * last half) to host memory and reports its size. Synchronising. */
int als_debug_copy_partials(als_engine* e, void* host_dst, int64_t max_bytes, int64_t* bytes);
/* Gram variant of `side`'s block: gram_path 0 = LDS-staged VALU (fp64, fp32 k < 32), 1 = fp32 MFMA
 * (v_mfma_f32_16x16x4_f32), 2 = split MFMA (fp32 operands split exactly into narrow terms); presplit = 1 when the
 * opposite table is gathered as the pre-split scaled two-term fp16 copy (h + m per value, RHS on the MFMAs too),
 * 0 when each gathered fp32 row is split on the fly into three bf16 terms; chunk = entries per contiguous PARTIAL
 * task of a split row (interleaved split rows: als_block_split_info); n_dual_rows[3] = short rows
 * of 1, 2 and 3 padded blocks solved in entry space, (Y Y^T + lambda n I) alpha = r, m = Y^T alpha (the same
 * solution as the k x k system). */
int als_block_path(const als_engine* e, int side, int* gram_path, int* presplit, int64_t* chunk, int64_t* n_dual_rows);
/* Work-plan statistics of the uploaded block (tasks, partial slots, padded nnz). */
int als_block_stats(const als_engine* e, int side, int64_t* n_tasks, int64_t* n_reduce, int64_t* nnz_padded);
/* Split-row plan of the uploaded block (a launch-shape query with no reference counterpart):
 * info[0] = rows split into interleaved chunks (0: contiguous chunks, the plan of halves whose opposite table fits the
 * L2s), [1] their chunk tasks, [2] the chunk length in entries, [3] 1 when the half gathers the pre-split table. */
int als_block_split_info(const als_engine* e, int side, int64_t info[4]);

#ifdef __cplusplus
}
#endif
#endif /* CFK_ALS_H */
