// Stand-alone check of check_table_rows (csrc/als_args.h), the row-range check of als_similar: both row lists against
// the one table they index. tests/test_similar_host.py compiles this file with als_args.cpp and als_error.cpp under
// -fsanitize=address,undefined and runs it as its own process. The lists are heap blocks of exactly the given length,
// so a read past either end is a sanitizer report. One JSON line per case: the status and the als_last_error() text.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "als.h"
#include "als_args.h"

using namespace cfk_detail;

namespace {

void rows(const char* name, std::vector<int64_t> q, std::vector<int64_t> c, int64_t n_rows) {
    const int st = check_table_rows("als_similar", q.data(), (int64_t)q.size(), c.data(), (int64_t)c.size(), n_rows);
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
    rows("ok", {0, 6, 3, 3}, {6, 0, 0}, 7);
    rows("ok_first_and_last_row", {0}, {(int64_t)1 << 40}, ((int64_t)1 << 40) + 1);
    rows("ok_no_queries", {}, {1, 2}, 3);
    rows("ok_no_candidates", {1, 2}, {}, 3);
    rows("query_negative", {0, -1, 9}, {0}, 7);
    rows("query_at_limit", {0, 1, 7}, {0}, 7);
    rows("cand_negative", {0}, {5, 6, -3}, 7);
    rows("cand_at_limit", {6}, {7, 8}, 7);
    rows("cand_beyond_int32", {6}, {0, (int64_t)1 << 33}, 7);
    // two faults: the queries are reported first
    rows("order_query_before_cand", {8}, {-1}, 7);
    rows("empty_table", {0}, {0}, 0);
    return 0;
}
