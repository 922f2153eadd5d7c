// als_args.h -- the checks of the caller's CSR arrays and row lists that the synchronous engine calls share
// (als_args.cpp): pure host arithmetic with no HIP header, so that tests/host/args_check.cpp and
// tests/host/similar_args_check.cpp run them under the sanitizers without a GPU.
// Every check sets als_last_error() and returns the status. Private to csrc/.
#pragma once
#include <cstdint>
#include <vector>

namespace cfk_detail {

// A CSR pointer array of n owners ("query", "user") named `name` in the messages of call `fn`: ptr[0] >= 0, no
// decrease, and fewer than 2^31 entries (`what`: "entries", "targets"). *count = ptr[n] - ptr[0]. O(n): reads ptr only.
int check_csr_ptr(const char* fn, const char* name, const char* owner, const char* what, const int64_t* ptr, int64_t n,
                  int64_t* count);

// The exclusion CSR of als_recommend / als_rank_targets, O(nnz): ranges in order, positions strictly ascending per
// user and inside [0, n_movies). Reads excl_idx in [excl_ptr[0], excl_ptr[n_users]) only.
int check_exclusions(const char* fn, const int64_t* excl_ptr, const int32_t* excl_idx, int64_t n_users, int64_t n_movies);

// The query CSR and destination rows (may be NULL) of als_fold_in / als_solve_implicit, O(n_queries + entries): the
// pointers (check_csr_ptr), then every index inside [0, opp_rows), then every destination row inside [0, self_rows)
// and given once. *nnz_out = the entry count.
int check_queries(const char* fn, int64_t n_queries, const int64_t* q_ptr, const int32_t* q_idx, const int64_t* dst_rows,
                  int64_t self_rows, int64_t opp_rows, int64_t* nnz_out);

// The factor rows als_implicit_objective reads its x from, one per query, O(n_queries): every rows[q] inside
// [0, self_rows). A row may be listed twice (nothing is written). The message names the query and the value.
int check_query_rows(const char* fn, const int64_t* rows, int64_t n_queries, int64_t self_rows);

// The two row lists of als_similar against the one table they index, O(n_queries + n_cand): every query_rows[i], then
// every cand_rows[i], inside [0, n_rows). The message names the array, the index and the value.
int check_table_rows(const char* fn, const int64_t* query_rows, int64_t n_queries, const int64_t* cand_rows, int64_t n_cand,
                     int64_t n_rows);

// The n + 1 pointers as the device wants them, starting at 0 (it indexes the uploaded slice): `ptr` itself when
// ptr[0] == 0, else the differences, kept in `store`.
const int64_t* rebase_ptr(const int64_t* ptr, int64_t n, std::vector<int64_t>& store);

}  // namespace cfk_detail
