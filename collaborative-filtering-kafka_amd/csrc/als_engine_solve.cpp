// als_engine_solve.cpp -- the resident factors and what the training loop runs on them: factor buffers and their I/O
// (with the staged read-back every call shares), the half-iteration launch and squared error. The calls that score the
// factors are in als_engine_score.cpp, those that solve ad-hoc queries in als_engine_query.cpp. The steady-state half
// (launch_half) allocates nothing and creates no stream or event: the side stream and its two events are made by the
// first half that needs them, timing events come from the engine's pool.
#include "als_engine_impl.h"

using namespace cfk_detail;

namespace cfk_detail {

int ensure_stage(als_engine* e) {
    HIP_TRY(e->h_stage.reserve(32u << 20));
    return ALS_OK;
}

void unpack_stage(const als_engine* e, int64_t nr, void* host_out, int64_t out_ld) {
    const size_t es = e->elem(), row_bytes = (size_t)e->kp * es;
    const char* stage = (const char*)e->h_stage.get();
    for (int64_t i = 0; i < nr; ++i)
        std::memcpy((char*)host_out + (size_t)i * out_ld * es, stage + i * row_bytes, (size_t)e->k * es);
}

// Read back the way the kernels wrote: a copy kernel (cfk::launch_download) moves whole kp-wide rows into pinned
// staging, the host keeps the first k columns; the path of als_write_factors in reverse.
int download_rows(als_engine* e, const char* fn, const char* d_rows, int64_t n, void* host_out, int64_t out_ld) {
    if (int r = ensure_stage(e)) return r;
    const size_t es = e->elem(), row_bytes = (size_t)e->kp * es;
    const int64_t rows_per = (int64_t)(e->h_stage.bytes() / row_bytes);
    for (int64_t r = 0; r < n; r += rows_per) {
        const int64_t nr = std::min(rows_per, n - r);
        hipError_t st = cfk::launch_download(d_rows + (size_t)r * row_bytes, e->h_stage.get(), (size_t)nr * row_bytes, e->stream);
        if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
        if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(st));
        unpack_stage(e, nr, (char*)host_out + (size_t)r * out_ld * es, out_ld);
    }
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
    HIP_TRY(hipSetDevice(e->device));
    if (int r = sync_checked(e)) return r;
    const char* rows = (const char*)e->fac[side].ptr + (size_t)row0 * e->kp * e->elem();
    return download_rows(e, "als_read_factors", rows, n_rows, host_dst, dst_ld);
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
