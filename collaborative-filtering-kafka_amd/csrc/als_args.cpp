// als_args.cpp -- the shared checks of the caller's CSR arrays (als_args.h). No HIP header.
#include "als_args.h"

#include <cstddef>
#include <unordered_set>

#include "als.h"
#include "als_error.h"

namespace cfk_detail {

int check_csr_ptr(const char* fn, const char* name, const char* owner, const char* what, const int64_t* ptr, int64_t n,
                  int64_t* count) {
    if (ptr[0] < 0) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: %s[0] is negative", fn, name);
    for (int64_t i = 0; i < n; ++i)
        if (ptr[i + 1] < ptr[i])
            return fail(ALS_ERR_INVALID_ARGUMENT, "%s: %s decreases at %s %lld", fn, name, owner, (long long)i);
    *count = ptr[n] - ptr[0];
    if (*count > INT32_MAX) return fail(ALS_ERR_INVALID_ARGUMENT, "%s: the number of %s must be below 2^31", fn, what);
    return ALS_OK;
}

// Not check_csr_ptr: this walk checks a user's positions before the next user's pointer, so of a bad position of
// user 0 and a decrease at user 1 it reports the position, and it has no bound on the count.
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

int check_queries(const char* fn, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx, const int64_t* dst_rows,
                  int64_t self_rows, int64_t opp_rows, int64_t* nnz_out) {
    if (int r = check_csr_ptr(fn, "q_ptr", "query", "entries", q_ptr, n_queries, nnz_out)) return r;
    for (int64_t q = 0; q < n_queries; ++q)
        for (int64_t x = q_ptr[q]; x < q_ptr[q + 1]; ++x)
            if (q_idx[x] < 0 || q_idx[x] >= opp_rows)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: index %d of query %lld is outside [0, %lld)", fn, (int)q_idx[x],
                            (long long)q, (long long)opp_rows);
    if (dst_rows) {
        std::unordered_set<int64_t> seen;
        seen.reserve((size_t)n_queries * 2);
        for (int64_t q = 0; q < n_queries; ++q) {
            if (dst_rows[q] < 0 || dst_rows[q] >= self_rows)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: dst_rows[%lld] = %lld of query %lld is outside [0, %lld)", fn,
                            (long long)q, (long long)dst_rows[q], (long long)q, (long long)self_rows);
            if (!seen.insert(dst_rows[q]).second)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: dst_rows repeats row %lld at query %lld", fn,
                            (long long)dst_rows[q], (long long)q);
        }
    }
    return ALS_OK;
}

int check_query_rows(const char* fn, const int64_t* rows, int64_t n_queries, int64_t self_rows) {
    for (int64_t q = 0; q < n_queries; ++q)
        if (rows[q] < 0 || rows[q] >= self_rows)
            return fail(ALS_ERR_INVALID_ARGUMENT, "%s: rows[%lld] = %lld of query %lld is outside [0, %lld)", fn, (long long)q,
                        (long long)rows[q], (long long)q, (long long)self_rows);
    return ALS_OK;
}

int check_table_rows(const char* fn, const int64_t* query_rows, int64_t n_queries, const int64_t* cand_rows, int64_t n_cand,
                     int64_t n_rows) {
    const struct {
        const char* name;
        const int64_t* rows;
        int64_t n;
    } lists[2] = {{"query_rows", query_rows, n_queries}, {"cand_rows", cand_rows, n_cand}};
    for (const auto& l : lists)
        for (int64_t i = 0; i < l.n; ++i)
            if (l.rows[i] < 0 || l.rows[i] >= n_rows)
                return fail(ALS_ERR_INVALID_ARGUMENT, "%s: %s[%lld] = %lld is outside [0, %lld)", fn, l.name, (long long)i,
                            (long long)l.rows[i], (long long)n_rows);
    return ALS_OK;
}

const int64_t* rebase_ptr(const int64_t* ptr, int64_t n, std::vector<int64_t>& store) {
    if (ptr[0] == 0) return ptr;
    store.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) store[(size_t)i] = ptr[i] - ptr[0];
    return store.data();
}

}  // namespace cfk_detail
