// als_engine_score.cpp -- the calls that score the resident factors: als_predict, als_recommend, als_similar and
// als_rank_targets with their *_plan calls. All four are synchronous, on the host path of als_engine_call.h; each keeps its own order
// of checks.
#include "als_engine_call.h"

using namespace cfk_detail;

namespace {

// The query rows of the three calls lie inside the factor matrices.
int check_query_rows(const als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows,
                     int64_t n_movies) {
    const int64_t nu = e->fac[ALS_SIDE_USER].n_rows, nm = e->fac[ALS_SIDE_MOVIE].n_rows;
    for (int64_t i = 0; i < n_users; ++i)
        if (user_rows[i] < 0 || user_rows[i] >= nu) return fail(ALS_ERR_INVALID_ARGUMENT, "user row out of range");
    for (int64_t i = 0; i < n_movies; ++i)
        if (movie_rows[i] < 0 || movie_rows[i] >= nm) return fail(ALS_ERR_INVALID_ARGUMENT, "movie row out of range");
    return ALS_OK;
}

}  // namespace

extern "C" {

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
    // per-call buffers, not d_rec: the engine would keep the dense n_users x n_movies output for good
    DeviceBuf<int64_t> d_u, d_m;
    DeviceBuf<float> d_out;
    hipError_t st = d_u.alloc((size_t)n_users);
    if (st == hipSuccess) st = d_m.alloc((size_t)n_movies);
    if (st == hipSuccess) st = d_out.alloc((size_t)n_users * (size_t)n_movies);
    if (st != hipSuccess) return fail(ALS_ERR_OUT_OF_MEMORY, "als_predict: device allocation: %s", hipGetErrorString(st));
    StreamChain c{e};
    c.upload(d_u.get(), user_rows, d_u.bytes());
    c.upload(d_m.get(), movie_rows, d_m.bytes());
    c.run(cfk::launch_predict, e->precision, U.ptr, M.ptr, e->kp, e->k, d_u.get(), n_users, d_m.get(), n_movies,
          d_out.get());
    c.download(host_out, d_out.get(), d_out.bytes());
    return c.finish("als_predict");
}

int als_recommend_plan(const als_engine* e, int64_t n_users, int64_t n_movies, int top_n, int64_t info[4]) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n_users < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (top_n < 1 || top_n > cfk::REC_MAX_TOP_N)
        return fail(ALS_ERR_INVALID_ARGUMENT, "top_n must be 1..%d, got %d", cfk::REC_MAX_TOP_N, top_n);
    const cfk::RecommendPlan p = cfk::recommend_plan(n_users, n_movies, top_n, e->kp, e->cu_count);
    return plan_info(info, p.user_tile, p.segments, p.seg_len, p.lds_bytes);
}

int als_recommend(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                  int top_n, const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* host_idx, float* host_score) {
    const char* fn = "als_recommend";
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
    if (excl_ptr)
        if (int r = check_exclusions(fn, excl_ptr, excl_idx, n_users, n_movies)) return r;
    const cfk::RecommendPlan p = cfk::recommend_plan(n_users, n_movies, top_n, e->kp, e->cu_count);
    if (p.lds_bytes > cfk::REC_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "als_recommend: launch plan exceeds the LDS");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    Workspace ws{p.workspace_bytes};   // the plan's parts, then the exclusion CSR
    const int64_t off_eptr = ws.part(excl_ptr != nullptr, (n_users + 1) * 8);
    const int64_t off_eidx = ws.part(excl_ptr != nullptr, excl_ptr ? (excl_ptr[n_users] - excl_ptr[0]) * 4 : 0);
    if (int r = reserve_workspace(e, fn, ws.need)) return r;
    char* w = e->d_rec.get();
    int64_t* d_u = (int64_t*)(w + p.off_urows);
    int64_t* d_m = (int64_t*)(w + p.off_mrows);
    int32_t* d_idx = (int32_t*)(w + p.off_idx);
    float* d_score = (float*)(w + p.off_score);
    float* d_ps = (float*)(w + p.off_part_score);
    int32_t* d_pp = (int32_t*)(w + p.off_part_pos);
    int64_t* d_eptr = excl_ptr ? (int64_t*)(w + off_eptr) : nullptr;
    int32_t* d_eidx = excl_ptr ? (int32_t*)(w + off_eidx) : nullptr;
    std::vector<int64_t> eptr0;
    StreamChain c{e};
    c.upload(d_u, user_rows, n_users * sizeof(int64_t));
    c.upload(d_m, movie_rows, n_movies * sizeof(int64_t));
    if (excl_ptr) upload_exclusions(c, excl_ptr, excl_idx, n_users, d_eptr, d_eidx, eptr0);
    c.run(cfk::launch_recommend, e->precision, U.ptr, M.ptr, e->kp, e->k, d_u, n_users, d_m, n_movies, top_n, p, d_eptr,
          d_eidx, d_ps, d_pp, d_score, d_idx);
    const size_t ob = (size_t)n_users * (size_t)top_n * 4;
    c.download(host_idx, d_idx, ob);
    c.download(host_score, d_score, ob);
    return c.finish(fn);
}

int als_similar_plan(const als_engine* e, int64_t n_queries, int64_t n_cand, int top_n, int64_t info[4]) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n_queries < 0 || n_cand < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (top_n < 1 || top_n > cfk::REC_MAX_TOP_N)
        return fail(ALS_ERR_INVALID_ARGUMENT, "top_n must be 1..%d, got %d", cfk::REC_MAX_TOP_N, top_n);
    const cfk::RecommendPlan p = cfk::similar_plan(n_queries, n_cand, top_n, e->kp, e->cu_count).sweep;
    return plan_info(info, p.user_tile, p.segments, p.seg_len, p.lds_bytes);
}

int als_similar(als_engine* e, int side, int metric, const int64_t* query_rows, int64_t n_queries, const int64_t* cand_rows,
                int64_t n_cand, int top_n, int exclude_self, int32_t* host_idx, float* host_score) {
    const char* fn = "als_similar";
    if (int r = check_engine(e)) return r;
    if (int r = check_side(side)) return r;
    if (metric != ALS_SIM_COSINE && metric != ALS_SIM_DOT)
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_similar: metric must be ALS_SIM_COSINE or ALS_SIM_DOT, got %d", metric);
    if (n_queries < 0 || n_cand < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    if (top_n < 1 || top_n > cfk::REC_MAX_TOP_N)
        return fail(ALS_ERR_INVALID_ARGUMENT, "als_similar: top_n must be 1..%d, got %d", cfk::REC_MAX_TOP_N, top_n);
    if (n_cand > INT32_MAX) return fail(ALS_ERR_INVALID_ARGUMENT, "als_similar: n_cand must be below 2^31");
    const Factors& F = e->fac[side];
    if (!F.ptr) return fail(ALS_ERR_STATE, "als_similar: factor matrix not allocated/bound");
    if (n_queries == 0 || n_cand == 0) return ALS_OK;
    if (!query_rows || !cand_rows || !host_idx || !host_score) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (int r = check_table_rows(fn, query_rows, n_queries, cand_rows, n_cand, F.n_rows)) return r;
    const cfk::SimilarPlan p = cfk::similar_plan(n_queries, n_cand, top_n, e->kp, e->cu_count);
    if (p.sweep.lds_bytes > cfk::REC_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "als_similar: launch plan exceeds the LDS");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, side == ALS_SIDE_MOVIE, side == ALS_SIDE_USER)) return r;
    if (int r = reserve_workspace(e, fn, p.workspace_bytes)) return r;
    char* w = e->d_rec.get();
    int64_t* d_q = (int64_t*)(w + p.sweep.off_urows);
    int64_t* d_c = (int64_t*)(w + p.sweep.off_mrows);
    int32_t* d_idx = (int32_t*)(w + p.sweep.off_idx);
    float* d_score = (float*)(w + p.sweep.off_score);
    float* d_ps = (float*)(w + p.sweep.off_part_score);
    int32_t* d_pp = (int32_t*)(w + p.sweep.off_part_pos);
    const bool cosine = metric == ALS_SIM_COSINE;
    float* d_inv_q = cosine ? (float*)(w + p.off_inv_q) : nullptr;
    float* d_inv_c = cosine ? (float*)(w + p.off_inv_c) : nullptr;
    StreamChain c{e};
    c.upload(d_q, query_rows, n_queries * sizeof(int64_t));
    c.upload(d_c, cand_rows, n_cand * sizeof(int64_t));
    if (cosine) c.run(cfk::launch_similar_norms, e->precision, F.ptr, e->kp, e->k, d_q, n_queries, d_c, n_cand, d_inv_q, d_inv_c);
    c.run(cfk::launch_similar_sweep, e->precision, F.ptr, e->kp, e->k, d_q, n_queries, d_c, n_cand, top_n, p.sweep, d_inv_q,
          d_inv_c, exclude_self != 0, d_ps, d_pp, d_score, d_idx);
    const size_t ob = (size_t)n_queries * (size_t)top_n * 4;
    c.download(host_idx, d_idx, ob);
    c.download(host_score, d_score, ob);
    return c.finish(fn);
}

int als_rank_plan(const als_engine* e, int64_t n_targets, int64_t n_movies, int64_t info[4]) {
    if (!e || !info) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (n_targets < 0 || n_movies < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "negative counts");
    const cfk::RankPlan p = cfk::rank_plan(n_targets, n_movies, e->kp, e->cu_count);
    return plan_info(info, p.tgt_tile, p.segments, p.seg_len, p.lds_bytes);
}

int als_rank_targets(als_engine* e, const int64_t* user_rows, int64_t n_users, const int64_t* movie_rows, int64_t n_movies,
                     const int64_t* tgt_ptr, const int32_t* tgt_idx, const int64_t* excl_ptr, const int32_t* excl_idx,
                     float* host_score, int32_t* host_rank) {
    const char* fn = "als_rank_targets";
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
    int64_t T = 0;
    if (int r = check_csr_ptr(fn, "tgt_ptr", "user", "targets", tgt_ptr, n_users, &T)) return r;
    if (T == 0 || (host_rank && n_movies == 0)) return ALS_OK;
    if (!user_rows || !movie_rows || !host_score) return fail(ALS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (int r = check_query_rows(e, user_rows, n_users, movie_rows, n_movies)) return r;
    // per target entry: its user's factor row and its query-user index (the exclusion range)
    const int64_t t0 = tgt_ptr[0];
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
    if (excl_ptr)
        if (int r = check_exclusions(fn, excl_ptr, excl_idx, n_users, n_movies)) return r;
    const bool with_excl = excl_ptr && host_rank;   // the scores do not depend on the exclusions
    const cfk::RankPlan p = cfk::rank_plan(T, n_movies, e->kp, e->cu_count);
    if (p.lds_bytes > cfk::RANK_LDS_LIMIT) return fail(ALS_ERR_UNSUPPORTED, "als_rank_targets: launch plan exceeds the LDS");
    HIP_TRY(hipSetDevice(e->device));
    if (int r = wait_gathers(e, true, true)) return r;
    Workspace ws{p.workspace_bytes};   // the plan's parts, then the exclusion CSR
    const int64_t off_eptr = ws.part(with_excl, (n_users + 1) * 8);
    const int64_t off_eidx = ws.part(with_excl, with_excl ? (excl_ptr[n_users] - excl_ptr[0]) * 4 : 0);
    if (int r = reserve_workspace(e, fn, ws.need)) return r;
    char* w = e->d_rec.get();
    int64_t* d_trow = (int64_t*)(w + p.off_trow);
    int32_t* d_tpos = (int32_t*)(w + p.off_tpos);
    int32_t* d_tuser = (int32_t*)(w + p.off_tuser);
    float* d_score = (float*)(w + p.off_score);
    int32_t* d_rank = (int32_t*)(w + p.off_rank);
    int64_t* d_m = (int64_t*)(w + p.off_mrows);
    int64_t* d_eptr = with_excl ? (int64_t*)(w + off_eptr) : nullptr;
    int32_t* d_eidx = with_excl ? (int32_t*)(w + off_eidx) : nullptr;
    std::vector<int64_t> eptr0;
    StreamChain c{e};
    c.upload(d_trow, trow.data(), T * sizeof(int64_t));
    c.upload(d_tpos, tgt_idx + t0, T * sizeof(int32_t));
    c.upload(d_m, movie_rows, n_movies * sizeof(int64_t));
    if (with_excl) {
        c.upload(d_tuser, tuser.data(), T * sizeof(int32_t));
        upload_exclusions(c, excl_ptr, excl_idx, n_users, d_eptr, d_eidx, eptr0);
    }
    c.run(cfk::launch_score_pairs, e->precision, U.ptr, M.ptr, e->kp, e->k, d_trow, d_tpos, d_m, T, d_score);
    if (host_rank)
        c.run(cfk::launch_rank, e->precision, U.ptr, M.ptr, e->kp, e->k, d_trow, d_tpos, d_tuser, d_score, T, d_m, n_movies, p,
              d_eptr, d_eidx, d_rank);
    c.download(host_score, d_score, T * sizeof(float));
    if (host_rank) c.download(host_rank, d_rank, T * sizeof(int32_t));
    return c.finish(fn);
}

}  // extern "C"
