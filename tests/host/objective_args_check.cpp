// Stand-alone check of check_query_rows (csrc/als_args.h), the check of als_implicit_objective's `rows`: one factor row
// per query inside the table, repeats allowed. tests/test_objective_host.py compiles this file with als_args.cpp and
// als_error.cpp under -fsanitize=address,undefined and runs it as its own process. The list is a heap block of exactly the
// given length, so a read past either end is a sanitizer report. One JSON line per case: the status and the
// als_last_error() text.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "als.h"
#include "als_args.h"

using namespace cfk_detail;

namespace {

void rows(const char* name, std::vector<int64_t> r, int64_t n_rows) {
    const int st = check_query_rows("als_implicit_objective", r.data(), (int64_t)r.size(), n_rows);
    std::string msg;
    if (st != ALS_OK)
        for (const char* ch = als_last_error(); *ch; ++ch) {
            if (*ch == '"' || *ch == '\\') msg.push_back('\\');
            msg.push_back(*ch);
        }
    printf("{\"case\": \"%s\", \"status\": %d, \"message\": \"%s\"}\n", name, st, msg.c_str());
}

}  // namespace

int main() {
    rows("ok", {0, 6, 3}, 7);
    rows("ok_repeated_row", {3, 3, 3, 0, 3}, 7);
    rows("ok_last_row_of_a_large_table", {(int64_t)1 << 40}, ((int64_t)1 << 40) + 1);
    rows("ok_no_queries", {}, 3);
    rows("negative", {0, -1, 9}, 7);
    rows("at_limit", {0, 1, 7}, 7);
    rows("beyond_int32", {6, (int64_t)1 << 33}, 7);
    rows("first_fault_is_reported", {8, -1}, 7);
    rows("empty_table", {0}, 0);
    return 0;
}
