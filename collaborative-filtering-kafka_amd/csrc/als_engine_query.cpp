// als_engine_query.cpp -- the calls that solve ad-hoc queries against the resident factors: als_fold_in (the explicit
// normal equation) and als_solve_implicit (implicit feedback) over one host path, solve_queries, with als_gram_table,
// als_implicit_objective (the implicit loss of resident rows, objective_queries) and the four *_plan calls. All of them
// are synchronous, on the host path of als_engine_call.h, and keep no
// per-engine state.
#include "als_engine_call.h"

#include <cmath>

using namespace cfk_detail;

namespace {

int check_stride(const als_engine* e, const char* fn) {
    if (e->kp > cfk::FOLDIN_MAX_KP)
        return fail(ALS_ERR_UNSUPPORTED, "%s: factor stride %d exceeds the supported %d", fn, e->kp, cfk::FOLDIN_MAX_KP);
    return ALS_OK;
}

// What the *_plan calls check: `fn` is the call the plan is of, `count` the name of its count argument.
int check_plan_call(const als_engine* e, const int64_t* info, const char* fn, const char* count, int64_t n) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "%s_plan: %s < 0", fn, count);
    return check_stride(e, fn);
}

// The implicit model's parameters, ratings and query order: what als_solve_implicit and als_implicit_objective share.
int check_model(const char* fn, float lambda, float alpha) {
    if (!(lambda > 0.f) || !std::isfinite(lambda))
        return fail(ALS_ERR_INVALID_ARGUMENT, "%s: lambda must be positive and finite", fn);
    if (!(alpha > 0.f) || !std::isfinite(alpha))
        return fail(ALS_ERR_INVALID_ARGUMENT, "%s: alpha must be positive and finite", fn);
    return ALS_OK;
}

int check_ratings(const char* fn, int64_t n_queries, const int64_t* q_ptr, const int16_t* q_ratings) {
    for (int64_t q = 0; q < n_queries; ++q)
        for (int64_t x = q_ptr[q]; x < q_ptr[q + 1]; ++x)
            if (q_ratings[x] < 0)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: rating %d of query %lld is negative", fn, (int)q_ratings[x],
                            (long long)q);
    return ALS_OK;
}

// The order the workgroups take the queries in: longest first (stable).
void longest_first(const int64_t* ptr, int64_t n_queries, std::vector<int64_t>& order) {
    order.resize(n_queries);
    for (int64_t q = 0; q < n_queries; ++q) order[q] = q;
    std::stable_sort(order.begin(), order.end(),
                     [&](int64_t x, int64_t y) { return ptr[x + 1] - ptr[x] > ptr[y + 1] - ptr[y]; });
}

// One call of als_fold_in or als_solve_implicit.
struct QueryCall {
    const char* fn;
    int side;
    int64_t n_queries;
    const int64_t* q_ptr;
    const int32_t* q_idx;
    const int16_t* q_ratings;
    float lambda;
    const float* alpha;   // NULL: the explicit model (lambda n, any lambda >= 0); else the implicit one
    const int64_t* dst_rows;
    void* host_out;
    int64_t out_ld;
};

int solve_queries(als_engine* e, const QueryCall& c) {
    const char* fn = c.fn;
    const bool implicit = c.alpha != nullptr;
    const int64_t n_queries = c.n_queries;
    if (int r = check_engine(e)) return r;
    if (int r = check_side(c.side)) return r;
    if (n_queries < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: n_queries < 0", fn);
    if (int r = check_stride(e, fn)) return r;
    const Factors& self = e->fac[c.side];
    const Factors& opp = e->fac[1 - c.side];
    if (!opp.ptr) return fail(ALS_ERR_STATE, "%s: factors of side %d (the opposite side) not allocated/bound", fn, 1 - c.side);
    if (c.dst_rows && !self.ptr)
        return fail(ALS_ERR_STATE, "%s: dst_rows given but factors of side %d not allocated/bound", fn, c.side);
    if (implicit)
        if (int r = check_model(fn, c.lambda, *c.alpha)) return r;
    if (n_queries == 0) return ALS_OK;
    if (!c.q_ptr || !c.q_idx || !c.q_ratings)
        return fail(ALS_ERR_INVALID_ARGUMENT, "%s: q_ptr, q_idx and q_ratings must be given", fn);
    if (!c.dst_rows && !c.host_out) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: dst_rows and host_out are both NULL", fn);
    if (c.host_out && c.out_ld < e->k)
        return fail(ALS_ERR_INVALID_ARGUMENT, "%s: out_ld (%lld) < num_features (%d)", fn, (long long)c.out_ld, e->k);
    if (!implicit && !(c.lambda >= 0.f)) return fail(ALS_ERR_INVALID_ARGUMENT, "lambda must be >= 0");
    int64_t nnz = 0;
    if (int r = check_queries(fn, n_queries, c.q_ptr, c.q_idx, c.dst_rows, self.n_rows, opp.n_rows, &nnz)) return r;
    const int64_t p0 = c.q_ptr[0];
    if (implicit)
        if (int r = check_ratings(fn, n_queries, c.q_ptr, c.q_ratings)) return r;
    const cfk::FoldinPlan p = implicit ? cfk::implicit_plan(e->kp, (int)e->elem(), n_queries, e->cu_count)
                                       : cfk::foldin_plan(e->kp, (int)e->elem(), n_queries, e->cu_count);
    if (p.lds_bytes > cfk::FOLDIN_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "%s: launch plan exceeds the LDS", fn);
    cfk::GramTablePlan gp;
    if (implicit) gp = cfk::gram_table_plan(e->kp, (int)e->elem(), opp.n_rows, e->cu_count);
    // the device ranges index the uploaded slice: rebased to 0. Implicit: the order the workgroups take the queries in,
    // longest first (stable), so that the one long query of a training half starts first instead of last. Results do
    // not depend on it.
    std::vector<int64_t> ptr0, order;
    const int64_t* ptr = rebase_ptr(c.q_ptr, n_queries, ptr0);
    if (implicit) longest_first(ptr, n_queries, order);
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    // workspace, every part 256-byte aligned: ranges, order, indices, ratings, destination rows, the opposite table's
    // Gram and its slabs' tiles, the kp-wide result rows
    const size_t row_bytes = (size_t)e->kp * e->elem();
    Workspace ws;
    const int64_t off_ptr = ws.part(true, (n_queries + 1) * 8);
    const int64_t off_ord = ws.part(implicit, n_queries * 8);
    const int64_t off_idx = ws.part(true, nnz * 4);
    const int64_t off_rat = ws.part(true, nnz * 2);
    const int64_t off_dst = ws.part(c.dst_rows != nullptr, n_queries * 8);
    const int64_t off_gram = ws.part(implicit, (int64_t)e->kp * (int64_t)row_bytes);
    const int64_t off_part = ws.part(implicit, gp.partial_bytes);
    const int64_t off_out = ws.part(true, n_queries * (int64_t)row_bytes);
    if (int r = reserve_workspace(e, fn, ws.need)) return r;
    // a result that fits the pinned staging buffer is queued behind the kernel, so the call waits for the stream once
    bool one_pass = false;
    if (c.host_out) {
        if (int r = ensure_stage(e)) return r;
        one_pass = n_queries <= (int64_t)(e->h_stage.bytes() / row_bytes);
    }
    char* w = e->d_rec.get();
    cfk::ImplicitArgs a{};
    a.f.opp = opp.ptr;
    a.f.self = self.ptr;
    a.f.out = w + off_out;
    a.f.q_ptr = (const int64_t*)(w + off_ptr);
    a.f.q_idx = (const int32_t*)(w + off_idx);
    a.f.q_rat = (const int16_t*)(w + off_rat);
    a.f.dst_rows = c.dst_rows ? (const int64_t*)(w + off_dst) : nullptr;
    a.f.n_queries = n_queries;
    a.f.k = e->k;
    a.f.lambda = c.lambda;
    StreamChain ch{e};
    ch.upload(w + off_ptr, ptr, (n_queries + 1) * sizeof(int64_t));
    if (nnz > 0) {
        ch.upload(w + off_idx, c.q_idx + p0, nnz * sizeof(int32_t));
        ch.upload(w + off_rat, c.q_ratings + p0, nnz * sizeof(int16_t));
    }
    if (c.dst_rows) ch.upload(w + off_dst, c.dst_rows, n_queries * sizeof(int64_t));
    if (implicit) {
        a.gram = w + off_gram;
        a.order = (const int64_t*)(w + off_ord);
        a.alpha = *c.alpha;
        ch.upload(w + off_ord, order.data(), n_queries * sizeof(int64_t));
        // G of the opposite table, recomputed on every call: no per-engine state that could go stale
        ch.run(cfk::launch_gram_table, e->precision, e->kp, opp.ptr, opp.n_rows, gp, w + off_part, w + off_gram);
        ch.run(cfk::launch_implicit, e->precision, e->kp, a, p);
    } else {
        ch.run(cfk::launch_fold_in, e->precision, e->kp, a.f, p);
    }
    if (one_pass) ch.run(cfk::launch_download, w + off_out, e->h_stage.get(), (size_t)n_queries * row_bytes);
    if (int r = ch.wait(fn)) return r;
    if (one_pass) {
        unpack_stage(e, n_queries, c.host_out, c.out_ld);
    } else if (c.host_out) {
        if (int r = download_rows(e, fn, w + off_out, n_queries, c.host_out, c.out_ld)) return r;
    }
    return sync_checked(e);
}

// als_implicit_objective: solve_queries' checks, rebasing, order and uploads with `rows` read instead of dst_rows
// written, the objective kernel in place of the solve, and 3 n + 1 doubles read back instead of n factor rows.
int objective_queries(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                      const int16_t* q_ratings, const int64_t* rows, float lambda, float alpha, double* host_parts,
                      double* totals) {
    const char* fn = "als_implicit_objective";
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (n_queries < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: n_queries < 0", fn);
    if (int r = check_stride(e, fn)) return r;
    const Factors& self = e->fac[side];
    const Factors& opp = e->fac[1 - side];
    if (!opp.ptr) return fail(ALS_ERR_STATE, "%s: factors of side %d (the opposite side) not allocated/bound", fn, 1 - side);
    if (!self.ptr) return fail(ALS_ERR_STATE, "%s: factors of side %d not allocated/bound", fn, side);
    if (int r = check_model(fn, lambda, alpha)) return r;
    if (!totals) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: totals is NULL", fn);
    if (n_queries == 0) {
        for (int i = 0; i < 4; ++i) totals[i] = 0.0;
        return ALS_OK;
    }
    if (!q_ptr || !q_idx || !q_ratings || !rows)
        return fail(ALS_ERR_INVALID_ARGUMENT, "%s: q_ptr, q_idx, q_ratings and rows must be given", fn);
    int64_t nnz = 0;
    if (int r = check_queries(fn, n_queries, q_ptr, q_idx, nullptr, self.n_rows, opp.n_rows, &nnz)) return r;
    if (int r = check_query_rows(fn, rows, n_queries, self.n_rows)) return r;
    if (int r = check_ratings(fn, n_queries, q_ptr, q_ratings)) return r;
    const int64_t p0 = q_ptr[0];
    const cfk::ObjectivePlan p = cfk::objective_plan(e->kp, (int)e->elem(), n_queries, e->cu_count);
    const cfk::GramTablePlan gp = cfk::gram_table_plan(e->kp, (int)e->elem(), opp.n_rows, e->cu_count);
    std::vector<int64_t> ptr0, order;
    const int64_t* ptr = rebase_ptr(q_ptr, n_queries, ptr0);
    longest_first(ptr, n_queries, order);
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    // workspace, every part 256-byte aligned: ranges, order, indices, ratings, rows, the opposite table's Gram and its
    // slabs' tiles, the queries' three doubles followed by lambda tr(G)
    const int64_t n_out = 3 * n_queries + 1;
    Workspace ws;
    const int64_t off_ptr = ws.part(true, (n_queries + 1) * 8);
    const int64_t off_ord = ws.part(true, n_queries * 8);
    const int64_t off_idx = ws.part(true, nnz * 4);
    const int64_t off_rat = ws.part(true, nnz * 2);
    const int64_t off_rows = ws.part(true, n_queries * 8);
    const int64_t off_gram = ws.part(true, (int64_t)e->kp * e->kp * (int64_t)e->elem());
    const int64_t off_part = ws.part(true, gp.partial_bytes);
    const int64_t off_out = ws.part(true, n_out * 8);
    if (int r = reserve_workspace(e, fn, ws.need)) return r;
    if (int r = ensure_stage(e)) return r;
    char* w = e->d_rec.get();
    cfk::ObjectiveArgs a{};
    a.opp = opp.ptr;
    a.self = self.ptr;
    a.gram = w + off_gram;
    a.q_ptr = (const int64_t*)(w + off_ptr);
    a.q_idx = (const int32_t*)(w + off_idx);
    a.q_rat = (const int16_t*)(w + off_rat);
    a.rows = (const int64_t*)(w + off_rows);
    a.order = (const int64_t*)(w + off_ord);
    a.parts = (double*)(w + off_out);
    a.n_queries = n_queries;
    a.k = e->k;
    a.lambda = lambda;
    a.alpha = alpha;
    StreamChain ch{e};
    ch.upload(w + off_ptr, ptr, (n_queries + 1) * sizeof(int64_t));
    ch.upload(w + off_ord, order.data(), n_queries * sizeof(int64_t));
    if (nnz > 0) {
        ch.upload(w + off_idx, q_idx + p0, nnz * sizeof(int32_t));
        ch.upload(w + off_rat, q_ratings + p0, nnz * sizeof(int16_t));
    }
    ch.upload(w + off_rows, rows, n_queries * sizeof(int64_t));
    // G of the opposite table, recomputed on every call as in solve_queries: no per-engine state
    ch.run(cfk::launch_gram_table, e->precision, e->kp, opp.ptr, opp.n_rows, gp, w + off_part, w + off_gram);
    ch.run(cfk::launch_objective, e->precision, e->kp, a, p);
    // Read back through the pinned staging buffer in passes of whole 16-byte pieces (an even count of doubles; the last
    // pass is rounded up inside the part's 256-byte padding). The first pass is queued behind the kernel. The column
    // sums run over the queries in ascending order, in double, on the host.
    const int64_t per_pass = (int64_t)(e->h_stage.bytes() / 16) * 2;
    const double* stage = (const double*)e->h_stage.get();
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t d0 = 0; d0 < n_out; d0 += per_pass) {
        const int64_t nd = std::min(per_pass, n_out - d0);
        ch.run(cfk::launch_download, w + off_out + d0 * 8, e->h_stage.get(), (size_t)((nd + 1) / 2 * 16));
        if (int r = ch.wait(fn)) return r;
        for (int64_t i = 0; i < nd; ++i) {
            const int64_t d = d0 + i;
            if (d == n_out - 1) {
                totals[3] = stage[i];
            } else {
                sum[d % 3] += stage[i];
                if (host_parts) host_parts[d] = stage[i];
            }
        }
    }
    for (int i = 0; i < 3; ++i) totals[i] = sum[i];
    return sync_checked(e);
}

}  // namespace

extern "C" {

int als_fold_in_plan(const als_engine* e, int64_t n_queries, int64_t info[4]) {
    if (int r = check_plan_call(e, info, "als_fold_in", "n_queries", n_queries)) return r;
    const cfk::FoldinPlan p = cfk::foldin_plan(e->kp, (int)e->elem(), n_queries, e->cu_count);
    return plan_info(info, p.threads, p.grid, p.batch, p.lds_bytes);
}

int als_fold_in(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                const int16_t* q_ratings, float lambda, const int64_t* dst_rows, void* host_out, int64_t out_ld) {
    return solve_queries(e, {"als_fold_in", side, n_queries, q_ptr, q_idx, q_ratings, lambda, nullptr, dst_rows, host_out,
                             out_ld});
}

int als_gram_table_plan(const als_engine* e, int64_t n_rows, int64_t info[4]) {
    if (int r = check_plan_call(e, info, "als_gram_table", "n_rows", n_rows)) return r;
    const cfk::GramTablePlan p = cfk::gram_table_plan(e->kp, (int)e->elem(), n_rows, e->cu_count);
    return plan_info(info, p.threads, p.slabs, p.rows_per_slab, p.lds_bytes);
}

int als_gram_table(als_engine* e, int side, void* host_out, int64_t out_ld) {
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (int r = check_stride(e, "als_gram_table")) return r;
    const Factors& tab = e->fac[side];
    if (!tab.ptr) return fail(ALS_ERR_STATE, "als_gram_table: factors of side %d not allocated/bound", side);
    if (!host_out) return fail(ALS_ERR_INVALID_ARGUMENT, "als_gram_table: host_out is NULL");
    if (out_ld < e->k)
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_gram_table: out_ld (%lld) < num_features (%d)", (long long)out_ld, e->k);
    const cfk::GramTablePlan p = cfk::gram_table_plan(e->kp, (int)e->elem(), tab.n_rows, e->cu_count);
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    // workspace: the kp x kp result, then the slabs' tiles
    Workspace ws;
    const int64_t off_gram = ws.part(true, (int64_t)e->kp * e->kp * (int64_t)e->elem());
    const int64_t off_part = ws.part(true, p.partial_bytes);
    if (int r = reserve_workspace(e, "als_gram_table", ws.need)) return r;
    char* w = e->d_rec.get();
    // one launch and download_rows' own wait, no chain: a failed launch has enqueued nothing to wait for
    const hipError_t st =
        cfk::launch_gram_table(e->precision, e->kp, tab.ptr, tab.n_rows, p, w + off_part, w + off_gram, e->stream);
    if (st != hipSuccess) return fail(ALS_ERR_DEVICE, "als_gram_table: %s", hipGetErrorString(st));
    if (int r = download_rows(e, "als_gram_table", w + off_gram, e->k, host_out, out_ld)) return r;
    return sync_checked(e);
}

int als_solve_implicit_plan(const als_engine* e, int64_t n_queries, int64_t info[4]) {
    if (int r = check_plan_call(e, info, "als_solve_implicit", "n_queries", n_queries)) return r;
    const cfk::FoldinPlan p = cfk::implicit_plan(e->kp, (int)e->elem(), n_queries, e->cu_count);
    return plan_info(info, p.threads, p.grid, p.batch, p.lds_bytes);
}

int als_solve_implicit(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                       const int16_t* q_ratings, float lambda, float alpha, const int64_t* dst_rows, void* host_out,
                       int64_t out_ld) {
    return solve_queries(e, {"als_solve_implicit", side, n_queries, q_ptr, q_idx, q_ratings, lambda, &alpha, dst_rows,
                             host_out, out_ld});
}

int als_implicit_objective_plan(const als_engine* e, int64_t n_queries, int64_t info[4]) {
    if (int r = check_plan_call(e, info, "als_implicit_objective", "n_queries", n_queries)) return r;
    const cfk::ObjectivePlan p = cfk::objective_plan(e->kp, (int)e->elem(), n_queries, e->cu_count);
    return plan_info(info, p.threads, p.grid, 0, p.lds_bytes);
}

int als_implicit_objective(als_engine* e, int side, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx,
                           const int16_t* q_ratings, const int64_t* rows, float lambda, float alpha, double* host_parts,
                           double totals[4]) {
    return objective_queries(e, side, n_queries, q_ptr, q_idx, q_ratings, rows, lambda, alpha, host_parts, totals);
}

}  // extern "C"
