// Stand-alone check of the argument unit (csrc/als_args.h): the CSR pointer walk, the exclusion and query checks and
// the pointer rebase, each driven with the smallest input that reaches a branch. tests/test_args_host.py compiles this
// file with als_args.cpp and als_error.cpp under -fsanitize=address,undefined and runs it as its own process. It
// prints one JSON line per case: the status, the als_last_error() text and, where a case has one, a result; the test
// holds what each must be.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "als.h"
#include "als_args.h"

#if defined(__SANITIZE_ADDRESS__)
#define ARGS_CHECK_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define ARGS_CHECK_ASAN 1
#endif
#endif
#ifdef ARGS_CHECK_ASAN
#include <sanitizer/asan_interface.h>
#endif

using namespace cfk_detail;

namespace {

void report(const char* name, int status, const std::string& extra = "") {
    std::string msg;
    if (status != ALS_OK)
        for (const char* c = als_last_error(); *c; ++c) {
            if (*c == '"' || *c == '\\') msg.push_back('\\');
            msg.push_back(*c);
        }
    printf("{\"case\": \"%s\", \"status\": %d, \"message\": \"%s\"%s}\n", name, status, msg.c_str(), extra.c_str());
}

std::string result(const char* key, int64_t v) { return ", \"" + std::string(key) + "\": " + std::to_string(v); }

std::string list(const char* key, const int64_t* v, size_t n) {
    std::string s = ", \"" + std::string(key) + "\": [";
    for (size_t i = 0; i < n; ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}

void walk(const char* name, std::vector<int64_t> ptr, int64_t n) {
    int64_t count = -1;
    const int st = check_csr_ptr("als_fold_in", "q_ptr", "query", "entries", ptr.data(), n, &count);
    report(name, st, st == ALS_OK ? result("count", count) : "");
}

void exclusions(const char* name, std::vector<int64_t> ptr, std::vector<int32_t> idx, int64_t n_movies) {
    report(name, check_exclusions("als_recommend", ptr.data(), idx.data(), (int64_t)ptr.size() - 1, n_movies));
}

void queries(const char* name, std::vector<int64_t> ptr, std::vector<int32_t> idx, std::vector<int64_t> dst,
             int64_t self_rows, int64_t opp_rows) {
    int64_t nnz = -1;
    const int st = check_queries("als_solve_implicit", (int64_t)ptr.size() - 1, ptr.data(), idx.data(),
                                 dst.empty() ? nullptr : dst.data(), self_rows, opp_rows, &nnz);
    report(name, st, st == ALS_OK ? result("count", nnz) : "");
}

}  // namespace

int main() {
    // the pointer walk
    walk("walk_ok", {2, 2, 5, 9}, 3);
    walk("walk_negative_first", {-1, 0, 1, 2}, 3);
    walk("walk_decrease_at_1", {0, 4, 3, 6}, 3);
    walk("walk_no_owners", {5}, 0);
    // 2^31 entries by the pointer array alone: no index array of that size exists, none is read
    walk("walk_count_2p31_minus_1", {7, 7 + (int64_t)INT32_MAX}, 1);
    walk("walk_count_2p31", {7, 7 + (int64_t)INT32_MAX + 1}, 1);
    {
        const int64_t ptr[2] = {0, (int64_t)1 << 31};
        int64_t nnz = -1;
        report("queries_count_2p31", check_queries("als_fold_in", 1, ptr, nullptr, nullptr, 10, 10, &nnz));
        int64_t T = -1;
        report("targets_count_2p31", check_csr_ptr("als_rank_targets", "tgt_ptr", "user", "targets", ptr, 1, &T));
        const int64_t bad[4] = {0, 4, 3, 6};
        report("targets_decrease_at_1", check_csr_ptr("als_rank_targets", "tgt_ptr", "user", "targets", bad, 3, &T));
    }

    // the query indices and destination rows
    queries("queries_ok", {1, 3, 3, 4}, {99, 0, 6, 3}, {4, 0, 2}, 5, 7);
    queries("queries_no_dst", {0, 1}, {6}, {}, 0, 7);
    queries("index_negative", {0, 2, 3}, {0, 1, -1}, {}, 5, 7);
    queries("index_at_limit", {0, 2, 3}, {0, 7, 1}, {}, 5, 7);
    queries("dst_negative", {0, 1, 2}, {0, 1}, {0, -1}, 5, 7);
    queries("dst_at_limit", {0, 1, 2}, {0, 1}, {5, 1}, 5, 7);
    queries("dst_repeat", {0, 1, 2, 3}, {0, 1, 2}, {3, 1, 3}, 5, 7);
    // two faults: q_ptr decreases at query 1 and query 0 has a bad index. All pointers are checked first.
    queries("order_pointer_before_index", {0, 2, 1}, {0, 7}, {}, 5, 7);

    // the exclusions
    exclusions("excl_ok", {0, 2, 2, 5}, {1, 4, 0, 2, 49}, 50);
    exclusions("excl_empty_ranges", {4, 4, 4, 4}, {}, 50);
    exclusions("excl_negative_first", {-2, 0, 1}, {1, 2, 3}, 50);
    exclusions("excl_decrease", {0, 2, 1}, {1, 2}, 50);
    exclusions("excl_unsorted", {0, 1, 4}, {9, 3, 8, 5}, 50);
    exclusions("excl_duplicate", {0, 3}, {3, 8, 8}, 50);
    exclusions("excl_position_negative", {0, 1, 2}, {0, -1}, 50);
    exclusions("excl_position_at_limit", {0, 1, 2}, {50, 0}, 50);
    // two faults: user 0 has a bad position and excl_ptr decreases at user 1. Each user's positions come before the
    // next pointer.
    exclusions("order_position_before_pointer", {0, 2, 1}, {0, 50}, 50);
    {
        // a slice with excl_ptr[0] = 3: the three entries before it are not the call's to read. A separate heap block
        // cannot lie under the same array, so they are three entries of the one block, poisoned by hand: the address
        // sanitizer reports any read of them as it would a read of a freed block. The live entries start on a shadow
        // granule (8 bytes) of their own, so that the poison covers exactly the three.
        std::vector<int32_t> block(8, -7);
        int32_t* base = block.data();
        while (((uintptr_t)(base + 3)) % 8 != 0) ++base;
        base[3] = 2;
        base[4] = 5;
        base[5] = 0;
        const int64_t ptr[3] = {3, 5, 6};
        std::vector<int64_t> store;
        int poisoned = -1;
#ifdef ARGS_CHECK_ASAN
        __asan_poison_memory_region(base, 3 * sizeof(int32_t));
        poisoned = 0;
        for (int i = 0; i < 3; ++i) poisoned += __asan_address_is_poisoned(base + i) ? 1 : 0;
#endif
        const int st = check_exclusions("als_rank_targets", ptr, base, 2, 6);
        const int64_t* r = rebase_ptr(ptr, 2, store);
#ifdef ARGS_CHECK_ASAN
        __asan_unpoison_memory_region(base, 3 * sizeof(int32_t));
#endif
        report("excl_slice_at_3", st, result("poisoned", poisoned) + list("rebased", r, 3));
    }

    // the rebase
    {
        const int64_t at0[4] = {0, 2, 2, 7};
        std::vector<int64_t> store;
        const int64_t* r = rebase_ptr(at0, 3, store);
        report("rebase_at_0", ALS_OK, result("same_pointer", r == at0) + result("store_size", (int64_t)store.size()));
        const int64_t at3[4] = {3, 5, 5, 10};
        const int64_t* q = rebase_ptr(at3, 3, store);
        report("rebase_at_3", ALS_OK, result("same_pointer", q == at3) + result("in_store", q == store.data()) +
                                          list("rebased", q, store.size()));
        const int64_t none[1] = {9};
        std::vector<int64_t> one;
        const int64_t* z = rebase_ptr(none, 0, one);
        report("rebase_no_owners", ALS_OK, list("rebased", z, one.size()));
    }
    return 0;
}
