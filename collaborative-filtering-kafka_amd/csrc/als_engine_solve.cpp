// als_engine_solve.cpp -- what runs on the resident factors: factor buffers and their I/O, the half-iteration launch,
// squared error, predict, recommend and held-out ranks (the calls that solve ad-hoc queries are in
// als_engine_query.cpp). The steady-state half (launch_half) allocates nothing and creates no stream or event: the side
// stream and its two events are made by the first half that needs them, timing events come from the engine's pool.
#include "als_engine_impl.h"

using namespace cfk_detail;

namespace cfk_detail {

int ensure_stage(als_engine* e) {
    HIP_TRY(e->h_stage.reserve(32u << 20));
    return ALS_OK;
}

}  // namespace cfk_detail

namespace {

// The engine, side, row range and leading dimension (named `ld`) of als_write_factors / als_read_factors.
int check_factor_range(als_engine* e, int side, int64_t row0, int64_t n_rows, const char* ld, int64_t ld_value) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Factors& f = e->fac[side];
    if (!f.ptr) return fail(ALS_ERR_STATE, "factors of side %d not allocated/bound", side);
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > f.n_rows) return fail(ALS_ERR_INVALID_ARGUMENT, "row range out of bounds");
    if (ld_value < e->k) return fail(ALS_ERR_INVALID_ARGUMENT, "%s (%lld) < num_features (%d)", ld, (long long)ld_value, e->k);
    return ALS_OK;
}

// The query rows of als_predict / als_recommend lie inside the factor matrices.
int check_query_rows(const als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows,
                     int64_t n_movies) {
    const int64_t nu = e->fac[ALS_SIDE_USER].n_rows, nm = e->fac[ALS_SIDE_MOVIE].n_rows;
    for (int64_t i = 0; i < n_users; ++i)
        if (user_rows[i] < 0 || user_rows[i] >= nu) return fail(ALS_ERR_INVALID_ARGUMENT, "user row out of range");
    for (int64_t i = 0; i < n_movies; ++i)
        if (movie_rows[i] < 0 || movie_rows[i] >= nm) return fail(ALS_ERR_INVALID_ARGUMENT, "movie row out of range");
    return ALS_OK;
}

// The exclusion CSR of als_recommend / als_rank_targets (`fn` names the call in the message), O(nnz): ranges in order,
// positions strictly ascending per user and inside the candidate set.
int check_exclusions(const char* fn, const int64_t* excl_ptr, const int32_t* excl_idx, int64_t n_users, int64_t n_movies) {
    if (excl_ptr[0] < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: excl_ptr[0] is negative", fn);
    for (int64_t u = 0; u < n_users; ++u) {
        const int64_t lo = excl_ptr[u], hi = excl_ptr[u + 1];
        if (hi < lo) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: excl_ptr decreases at user %lld", fn, (long long)u);
        for (int64_t x = lo; x < hi; ++x) {
            if (excl_idx[x] < 0 || excl_idx[x] >= n_movies)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: excluded position %d of user %lld is outside [0, %lld)", fn,
                            (int)excl_idx[x], (long long)u, (long long)n_movies);
            if (x > lo && excl_idx[x] <= excl_idx[x - 1])
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: excluded positions of user %lld are not strictly ascending", fn,
                            (long long)u);
        }
    }
    return ALS_OK;
}

// The three events of a timed half: taken from the engine's pool, handed to e->pending by commit(), and back in the
// pool when the half returns early.
struct TimingGuard {
    als_engine* e;
    TimingRec rec;
    ~TimingGuard() {
        for (auto& ev : rec.ev)
            if (ev) e->ev_pool.push_back(std::move(ev));
    }
    int take() {
        for (auto& ev : rec.ev) {
            if (!e->ev_pool.empty()) {
                ev = std::move(e->ev_pool.back());
                e->ev_pool.pop_back();
            } else {
                HIP_TRY(ev.create());
            }
        }
        return ALS_OK;
    }
    void commit() { e->pending.push_back(std::move(rec)); }
};

// One half (or one chunk of it): the FULL + PARTIAL launch, then the REDUCE launch.
int launch_half(als_engine* e, int side, float lambda, const HalfTasks& h) {
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
    if (int r = wait_gathers(e, side == ALS_SIDE_USER || h.first_chunk, side == ALS_SIDE_MOVIE || h.first_chunk)) return r;
    cfk::SolveArgs a{};
    a.tasks = h.main.t;
    a.n_tasks = h.main.n;
    a.k = e->k;
    a.col = b.d_col.get();
    a.rat = b.d_rat.get();
    a.opp = opp.ptr;
    a.out = self.ptr;
    a.row_offset = b.row_offset;
    a.rows_per_chunk = (int32_t)b.rows_per_chunk;
    a.chunk_stride = b.chunk_stride;
    a.partials = e->d_partials.get();
    a.scratch_slabs = e->generic_slabs;
    a.lambda = lambda;
    a.sentinel = (int32_t)b.n_opp_rows;
    a.flags = e->path == Path::VALU ? 0 : e->cfg.debug_flags;
    if (++e->gen == 0) e->gen = 1;
    a.gen = e->cfg.debug_fixed_gen ? 1u : e->gen;
    a.integrity = e->d_integrity.get();
    a.refine_min_pivot = e->cfg.refine_min_pivot;
    a.extra_lds = e->cfg.debug_extra_lds;
    TimingGuard timed{e, {}};
    timed.rec.side = side;
    if (e->timing) {
        if (int r = timed.take()) return r;
        HIP_TRY(hipEventRecord(timed.rec.ev[0], e->stream));
    }
    const bool any_dual = h.dual[0].n > 0 || h.dual[1].n > 0 || h.dual[2].n > 0;
    const bool side_dual = any_dual && e->cfg.dual_side;
    if (side_dual) {   // the dual launches read the fp32 opposite table only: fork before the pre-split
        if (!e->join) {   // (the last of the three to be made)
            HIP_TRY(e->side_stream.create());
            HIP_TRY(e->fork.create(hipEventDisableTiming));
            HIP_TRY(e->join.create(hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(e->fork, e->stream));
    }
    uint32_t* const prep = e->d_prep.get();
    if (b.layout.presplit) {
        // the opposite replica is the half's input and does not change between its chunks (als.h): chunk 0
        // converts it, later chunks reuse the conversion and its range words. The two sets of range words alternate
        // per preparation: each preparation zeroes the other set, which the launches of the half before it read.
        if (h.first_chunk) {
            e->prep_set ^= 1;
            HIP_TRY(cfk::launch_presplit_prepare(e->kp, (const float*)opp.ptr, e->d_split.get(), b.n_opp_rows + 1,
                                                 prep + e->prep_set * cfk::PREP_SET_WORDS,
                                                 prep + (e->prep_set ^ 1) * cfk::PREP_SET_WORDS,
                                                 prep + 2 * cfk::PREP_SET_WORDS + side, e->cu_count, e->stream));
        }
        a.opp_split = e->d_split.get();
        a.rat_pk = b.d_rat_pk.get();
        a.rat_lo_off = b.nnz_padded / 2;
        a.col_ps = b.d_col_ps.get();
        a.amax = prep + e->prep_set * cfk::PREP_SET_WORDS;
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
        if (h.dual[c].n > 0) {
            cfk::SolveArgs d = a;
            d.tasks = h.dual[c].t;
            d.n_tasks = h.dual[c].n;
            HIP_TRY(cfk::launch_dual(e->kp, 2 * (c + 1), d, side_dual ? e->side_stream : e->stream));
        }
    if (side_dual) {
        HIP_TRY(hipEventRecord(e->join, e->side_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->join, 0));
    }
    if (e->timing) HIP_TRY(hipEventRecord(timed.rec.ev[1], e->stream));
    if (h.reduce.n > 0) {
        a.tasks = h.reduce.t;
        a.n_tasks = h.reduce.n;
        a.gen += e->cfg.debug_gen_skew;
        HIP_TRY(cfk::launch_solve(e->precision, e->kp, e->path, a, e->stream, false, true));
    }
    if (e->timing) {
        HIP_TRY(hipEventRecord(timed.rec.ev[2], e->stream));
        timed.commit();
    }
    return ALS_OK;
}

}  // namespace

extern "C" {

int als_alloc_factors(als_engine* e, int side, int64_t n_total_rows) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (n_total_rows < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "n_total_rows < 0");
    HIP_TRY(hipSetDevice(e->device));
    Factors& f = e->fac[side];
    f = Factors();
    const size_t bytes = (size_t)(n_total_rows + 1) * e->kp * e->elem();   // + sentinel zero row
    hipError_t st = f.owned.alloc(bytes);
    if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "factors device allocation (%zu bytes): %s", bytes, hipGetErrorString(st));
    f.ptr = f.owned.get();
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
    f = Factors();
    f.ptr = device_ptr;
    f.n_rows = n_total_rows;
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
    if (int r = check_factor_range(e, side, row0, n_rows, "src_ld", src_ld)) return r;
    if (n_rows == 0) return ALS_OK;
    if (!host_src) return fail(ALS_ERR_INVALID_ARGUMENT, "host_src is NULL");
    const Factors& f = e->fac[side];
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    const size_t es = e->elem();
    // Rows are packed kp wide (padding columns zero) into pinned staging and written by a copy kernel
    // (cfk::launch_upload) on the engine's stream: see copy16 in als_kernels.hip.
    const size_t row_bytes = (size_t)e->kp * es;
    if (int r = ensure_stage(e)) return r;
    HIP_TRY(hipStreamSynchronize(e->stream));   // the staging buffer may still feed an earlier copy
    const int64_t rows_per = (int64_t)(e->h_stage.bytes() / row_bytes);
    for (int64_t r = 0; r < n_rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, n_rows - r);
        char* stage = (char*)e->h_stage.get();
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
    if (int r = check_factor_range(e, side, row0, n_rows, "dst_ld", dst_ld)) return r;
    if (n_rows == 0) return ALS_OK;
    if (!host_dst) return fail(ALS_ERR_INVALID_ARGUMENT, "host_dst is NULL");
    const Factors& f = e->fac[side];
    HIP_TRY(hipSetDevice(e->device));
    if (int r = sync_checked(e)) return r;
    const size_t es = e->elem();
    // Read back the way the kernels wrote: a copy kernel (cfk::launch_download) moves whole kp-wide rows into
    // pinned staging, the host keeps the first k columns; the same path as als_write_factors in reverse.
    const size_t row_bytes = (size_t)e->kp * es;
    if (int r = ensure_stage(e)) return r;
    const int64_t rows_per = (int64_t)(e->h_stage.bytes() / row_bytes);
    for (int64_t r = 0; r < n_rows; r += rows_per) {
        const int64_t nr = std::min(rows_per, n_rows - r);
        HIP_TRY(cfk::launch_download((const char*)f.ptr + (size_t)(row0 + r) * row_bytes, e->h_stage.get(),
                                     (size_t)nr * row_bytes, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        const char* stage = (const char*)e->h_stage.get();
        char* dst = (char*)host_dst + (size_t)r * dst_ld * es;
        for (int64_t i = 0; i < nr; ++i)
            std::memcpy(dst + (size_t)i * dst_ld * es, stage + i * row_bytes, (size_t)e->k * es);
    }
    return ALS_OK;
}

int als_solve_half(als_engine* e, int side, float lambda) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Block& b = e->blk[side];
    if (!b.set) return fail(ALS_ERR_STATE, "als_solve_half: no block set for side %d", side);
    return launch_half(e, side, lambda, b.half_tasks(-1));
}

int als_solve_half_chunk(als_engine* e, int side, float lambda, int chunk) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    const Block& b = e->blk[side];
    const int n_chunks = (int)b.tasks.coff.size() - 1;
    if (!b.set || n_chunks < 0) return fail(ALS_ERR_STATE, "als_solve_half_chunk: no chunks set for side %d", side);
    if (chunk < 0 || chunk >= n_chunks)
        return fail(ALS_ERR_INVALID_ARGUMENT, "chunk %d out of range (%d chunks)", chunk, n_chunks);
    return launch_half(e, side, lambda, b.half_tasks(chunk));
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
    if (int r = check_query_rows(e, user_rows, n_users, movie_rows, n_movies)) return r;
    if ((n_users + 15) / 16 > 65535) return fail(ALS_ERR_UNSUPPORTED, "at most 1,048,560 users per call (call per user range)");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    DeviceBuf<int64_t> d_u, d_m;
    DeviceBuf<float> d_out;
    hipError_t st = d_u.alloc((size_t)n_users);
    if (st == hipSuccess) st = d_m.alloc((size_t)n_movies);
    if (st == hipSuccess) st = d_out.alloc((size_t)n_users * (size_t)n_movies);
    if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "als_predict: device allocation: %s", hipGetErrorString(st));
    st = hipMemcpyAsync(d_u.get(), user_rows, d_u.bytes(), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_m.get(), movie_rows, d_m.bytes(), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
        st = cfk::launch_predict(e->precision, U.ptr, M.ptr, e->kp, e->k, d_u.get(), n_users, d_m.get(), n_movies,
                                 d_out.get(), e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(host_out, d_out.get(), d_out.bytes(), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
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
    if (int r = check_query_rows(e, user_rows, n_users, movie_rows, n_movies)) return r;
    int64_t ex0 = 0, ex_nnz = 0;
    if (excl_ptr) {
        if (int r = check_exclusions("als_recommend", excl_ptr, excl_idx, n_users, n_movies)) return r;
        ex0 = excl_ptr[0];
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
    if (need > e->d_rec.size()) {   // grow-only; the stream may still be reading the old one
        HIP_TRY(hipStreamSynchronize(e->stream));
        const hipError_t st = e->d_rec.reserve(need);
        if (st != hipSuccess)
            return fail(ALS_ERR_OUT_OF_MEMORY, "als_recommend: device allocation (%zu bytes): %s", need, hipGetErrorString(st));
    }
    char* w = e->d_rec.get();
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

int als_rank_plan(const als_engine* e, int64_t n_targets, int64_t n_movies, int64_t info[4]) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n_targets < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    const cfk::RankPlan p = cfk::rank_plan(n_targets, n_movies, e->kp, e->cu_count);
    info[0] = p.tgt_tile;
    info[1] = p.segments;
    info[2] = p.seg_len;
    info[3] = p.lds_bytes;
    return ALS_OK;
}

int als_rank_targets(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                     const int64_t* tgt_ptr, const int32_t* tgt_idx, const int64_t* excl_ptr, const int32_t* excl_idx,
                     float* host_score, int32_t* host_rank) {
    if (int r = check_engine(e)) return r;
    if (n_users < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (!tgt_ptr || !tgt_idx) return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: tgt_ptr and tgt_idx must both be given");
    if ((excl_ptr == nullptr) != (excl_idx == nullptr))
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: excl_ptr and excl_idx must both be given or both be NULL");
    if (n_movies > INT32_MAX) return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: n_movies must be below 2^31");
    if (n_users > INT32_MAX) return fail(ALS_ERR_UNSUPPORTED, "als_rank_targets: at most 2^31 - 1 query users per call");
    const Factors& U = e->fac[ALS_SIDE_USER];
    const Factors& M = e->fac[ALS_SIDE_MOVIE];
    if (!U.ptr || !M.ptr) return fail(ALS_ERR_STATE, "als_rank_targets: factor matrices not allocated/bound");
    if (n_users == 0) return ALS_OK;
    const int64_t t0 = tgt_ptr[0];
    if (t0 < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: tgt_ptr[0] is negative");
    for (int64_t u = 0; u < n_users; ++u)
        if (tgt_ptr[u + 1] < tgt_ptr[u])
            return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: tgt_ptr decreases at user %lld", (long long)u);
    const int64_t T = tgt_ptr[n_users] - t0;
    if (T > INT32_MAX) return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: the number of targets must be below 2^31");
    if (T == 0 || (host_rank && n_movies == 0)) return ALS_OK;
    if (!user_rows || !movie_rows || !host_score) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (int r = check_query_rows(e, user_rows, n_users, movie_rows, n_movies)) return r;
    // per target entry: its user's factor row and its query-user index (the exclusion range)
    std::vector<int64_t> trow((size_t)T);
    std::vector<int32_t> tuser((size_t)T);
    for (int64_t u = 0; u < n_users; ++u)
        for (int64_t x = tgt_ptr[u]; x < tgt_ptr[u + 1]; ++x) {
            if (tgt_idx[x] < 0 || tgt_idx[x] >= n_movies)
                return fail(ALS_ERR_INVALID_ARGUMENT, "als_rank_targets: target position %d of user %lld is outside [0, %lld)",
                            (int)tgt_idx[x], (long long)u, (long long)n_movies);
            trow[(size_t)(x - t0)] = user_rows[u];
            tuser[(size_t)(x - t0)] = (int32_t)u;
        }
    const bool with_excl = excl_ptr && host_rank;   // the scores do not depend on the exclusions
    int64_t ex0 = 0, ex_nnz = 0;
    if (excl_ptr) {
        if (int r = check_exclusions("als_rank_targets", excl_ptr, excl_idx, n_users, n_movies)) return r;
        ex0 = excl_ptr[0];
        ex_nnz = excl_ptr[n_users] - ex0;
    }
    const cfk::RankPlan p = cfk::rank_plan(T, n_movies, e->kp, e->cu_count);
    if (p.lds_bytes > cfk::RANK_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "als_rank_targets: launch plan exceeds the LDS");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
    const int64_t off_eptr = p.workspace_bytes;
    const int64_t off_eidx = off_eptr + (with_excl ? align((n_users + 1) * 8) : 0);
    const size_t need = (size_t)(off_eidx + (with_excl ? align(ex_nnz * 4) : 0));
    // als_recommend's workspace: both calls are synchronous, so neither is reading it when the other starts
    if (need > e->d_rec.size()) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        const hipError_t st = e->d_rec.reserve(need);
        if (st != hipSuccess)
            return fail(ALS_ERR_OUT_OF_MEMORY, "als_rank_targets: device allocation (%zu bytes): %s", need, hipGetErrorString(st));
    }
    char* w = e->d_rec.get();
    int64_t* d_trow = (int64_t*)(w + p.off_trow);
    int32_t* d_tpos = (int32_t*)(w + p.off_tpos);
    int32_t* d_tuser = (int32_t*)(w + p.off_tuser);
    float* d_score = (float*)(w + p.off_score);
    int32_t* d_rank = (int32_t*)(w + p.off_rank);
    int64_t* d_m = (int64_t*)(w + p.off_mrows);
    int64_t* d_eptr = with_excl ? (int64_t*)(w + off_eptr) : nullptr;
    int32_t* d_eidx = with_excl ? (int32_t*)(w + off_eidx) : nullptr;
    std::vector<int64_t> eptr0;   // the device ranges index the uploaded slice: rebased to 0
    hipError_t st = hipMemcpyAsync(d_trow, trow.data(), T * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_tpos, tgt_idx + t0, T * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_m, movie_rows, n_movies * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess && with_excl) {
        st = hipMemcpyAsync(d_tuser, tuser.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        const int64_t* src = excl_ptr;
        if (ex0 != 0) {
            eptr0.resize(n_users + 1);
            for (int64_t u = 0; u <= n_users; ++u) eptr0[u] = excl_ptr[u] - ex0;
            src = eptr0.data();
        }
        if (st == hipSuccess) st = hipMemcpyAsync(d_eptr, src, (n_users + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e->stream);
        if (st == hipSuccess && ex_nnz > 0)
            st = hipMemcpyAsync(d_eidx, excl_idx + ex0, ex_nnz * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    }
    if (st == hipSuccess)
        st = cfk::launch_score_pairs(e->precision, U.ptr, M.ptr, e->kp, e->k, d_trow, d_tpos, d_m, T, d_score, e->stream);
    if (st == hipSuccess && host_rank)
        st = cfk::launch_rank(e->precision, U.ptr, M.ptr, e->kp, e->k, d_trow, d_tpos, d_tuser, d_score, T, d_m, n_movies, p,
                              d_eptr, d_eidx, d_rank, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(host_score, d_score, T * sizeof(float), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess && host_rank)
        st = hipMemcpyAsync(host_rank, d_rank, T * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    // the host arrays are pageable: the stream has to pass the copies before this call returns
    const hipError_t st2 = hipStreamSynchronize(e->stream);
    if (st == hipSuccess) st = st2;
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "als_rank_targets: %s", hipGetErrorString(st));
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
    a.tasks = b.sq_tasks.get();
    a.n_tasks = (int32_t)b.sq_tasks.size();
    a.col = b.d_col.get();
    a.rat = b.d_rat.get();
    a.opp = opp.ptr;
    a.self = self.ptr;
    a.row_offset = b.row_offset;
    a.rows_per_chunk = (int32_t)b.rows_per_chunk;
    a.chunk_stride = b.chunk_stride;
    a.task_se = b.d_task_se.get();
    a.sentinel = (int32_t)b.n_opp_rows;
    HIP_TRY(cfk::launch_sq_error(e->precision, e->kp, a, e->stream));
    std::vector<double> se(b.sq_tasks.size());
    if (!se.empty())
        HIP_TRY(hipMemcpyAsync(se.data(), b.d_task_se.get(), se.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (int r = sync_checked(e)) return r;
    double s = 0.0;
    for (double v : se) s += v;   // fixed (task) order: deterministic
    if (sum_sq_error) *sum_sq_error = s;
    if (count) *count = b.nnz;
    return ALS_OK;
}

}  // extern "C"
