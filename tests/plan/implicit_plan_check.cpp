// Stand-alone check of cfk::gram_table_plan and cfk::implicit_plan (csrc/als_plan.cpp), the launch plans of als_gram_table
// and als_solve_implicit: built together with als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as
// its own process (tests/test_implicit_host.py). Sweeps every kp (16, 32, 64, 128 at both element sizes; 80, 96, 112 at 8
// bytes), cu_count in {1, 8, 256} and 1 .. 10^7 rows / queries, checks every invariant from the plans alone and prints one
// JSON line: {"cases": n, "failed": {check: "count, first: shape"},
//             "gram": {"kp/elem/n": [threads, slabs, rows per slab, lds]}, "solve": {"kp/elem/n/cu": [threads, grid, batch, lds]}}.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "als_plan.h"

int main() {
    struct Shape { int kp, elem; };
    std::vector<Shape> shapes;
    for (int kp : {16, 32, 64, 128})
        for (int elem : {4, 8}) shapes.push_back({kp, elem});
    for (int kp : {80, 96, 112}) shapes.push_back({kp, 8});
    const int cus[] = {1, 8, 256};
    std::vector<int64_t> counts;
    for (int64_t n = 1; n <= 70; ++n) counts.push_back(n);
    for (int64_t n = 100; n <= 10000000; n *= 10)
        for (int64_t d = -1; d <= 1; ++d) counts.push_back(n + d);
    for (int64_t n : {255, 256, 257, 511, 512, 513, 1024, 2047, 2048, 2049, 4096, 5000, 65536, 262143, 262144, 262145,
                      1234567})
        counts.push_back(n);
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0;
    std::string gram, solve;
    for (const Shape& sh : shapes)
        for (int64_t n : counts) {
            const int kp = sh.kp, elem = sh.elem;
            int cu = 0;
            auto check = [&](const char* name, bool ok) {
                if (ok) return;
                if (!failed[name]++) {
                    char buf[160];
                    snprintf(buf, sizeof buf, "kp %d elem %d n %lld cu %d", kp, elem, (long long)n, cu);
                    first[name] = buf;
                }
            };
            const cfk::GramTablePlan ref = cfk::gram_table_plan(kp, elem, n, 1);
            for (int c : cus) {
                cu = c;
                ++n_cases;
                const cfk::GramTablePlan g = cfk::gram_table_plan(kp, elem, n, cu);
                check("gram_plan_ignores_the_device", g.slabs == ref.slabs && g.rows_per_slab == ref.rows_per_slab &&
                                                          g.lds_bytes == ref.lds_bytes && g.partial_bytes == ref.partial_bytes);
                check("gram_threads_are_the_kernel_s", g.threads == cfk::FOLDIN_THREADS && g.threads == 256);
                check("gram_slabs_within_the_cap", g.slabs >= 1 && g.slabs <= cfk::GRAM_TABLE_MAX_SLABS && g.slabs <= 1024);
                check("gram_slab_is_whole_batches",
                      g.rows_per_slab >= cfk::GRAM_TABLE_MIN_SLAB_ROWS && g.rows_per_slab % cfk::FOLDIN_MAX_BATCH == 0);
                // the slabs tile the rows exactly once: slab s owns [s L, min((s + 1) L, n)), none empty, none past n
                check("gram_slabs_tile_the_rows",
                      g.slabs * g.rows_per_slab >= n && (g.slabs - 1) * g.rows_per_slab < n);
                int64_t covered = 0;
                for (int64_t s = 0; s < g.slabs; ++s) {
                    const int64_t lo = s * g.rows_per_slab, hi = lo + g.rows_per_slab < n ? lo + g.rows_per_slab : n;
                    if (lo != covered || hi <= lo) covered = -1 - n;   // a gap, an overlap or an empty slab
                    else covered = hi;
                }
                check("gram_slabs_cover_each_row_once", covered == n);
                check("gram_slab_length_depends_on_the_rows_alone",
                      g.rows_per_slab == cfk::gram_table_plan(16, 4, n, 7).rows_per_slab);
                check("gram_lds_within_the_cu", g.lds_bytes > 0 && g.lds_bytes <= 163840);
                check("gram_lds_is_the_kernel_s", g.lds_bytes == cfk::gram_table_lds_bytes(kp, elem) &&
                                                      g.lds_bytes >= (int64_t)elem * cfk::FOLDIN_MAX_BATCH * (kp + 1));
                check("staged_rows_stay_16_byte_aligned", ((int64_t)cfk::foldin_pitch(kp) * elem) % 16 == 0);
                check("operand_reads_conflict_free", cfk::foldin_pitch(kp) % 32 == 16 && cfk::foldin_pitch(kp) >= kp);
                check("gram_partials_hold_every_tile",
                      g.partial_bytes == g.slabs * (int64_t)cfk::foldin_tiles(kp) * 256 * elem);

                const cfk::FoldinPlan p = cfk::implicit_plan(kp, elem, n, cu);
                const cfk::FoldinPlan f = cfk::foldin_plan(kp, elem, n, cu);
                check("solve_plan_is_fold_in_s", p.threads == f.threads && p.grid == f.grid && p.batch == f.batch &&
                                                     p.lds_bytes == f.lds_bytes);
                check("solve_lds_within_the_cu", p.lds_bytes > 0 && p.lds_bytes <= 163840);
                check("solve_lds_is_the_kernel_s", p.lds_bytes == cfk::foldin_lds_bytes(kp, elem, p.batch));
                check("solve_tiles_stay_16_byte_aligned",
                      ((int64_t)cfk::foldin_tiles(kp) * cfk::FOLDIN_TILE_ELEMS * elem) % 16 == 0);
                check("solve_batch_whole_mfma_steps", p.batch >= 4 && p.batch % 4 == 0 && p.batch <= cfk::FOLDIN_MAX_BATCH);
                check("solve_grid_within_the_queries", p.grid >= 1 && p.grid <= n);
                check("solve_grid_fills_no_more_than_the_device", p.grid <= (int64_t)cu * cfk::FOLDIN_MAX_WG_PER_CU);
                char key[128];
                snprintf(key, sizeof key, "%s\"%d/%d/%lld/%d\": [%d, %lld, %d, %lld]", solve.empty() ? "" : ", ", kp, elem,
                         (long long)n, cu, p.threads, (long long)p.grid, p.batch, (long long)p.lds_bytes);
                solve += key;
            }
            char key[128];
            snprintf(key, sizeof key, "%s\"%d/%d/%lld\": [%d, %lld, %lld, %lld]", gram.empty() ? "" : ", ", kp, elem,
                     (long long)n, ref.threads, (long long)ref.slabs, (long long)ref.rows_per_slab, (long long)ref.lds_bytes);
            gram += key;
        }
    printf("{\"cases\": %lld, \"failed\": {", (long long)n_cases);
    bool sep = false;
    for (auto& kv : failed)
        if (kv.second) {
            printf("%s\"%s\": \"%lld, first: %s\"", sep ? ", " : "", kv.first.c_str(), (long long)kv.second,
                   first[kv.first].c_str());
            sep = true;
        }
    printf("}, \"gram\": {%s}, \"solve\": {%s}}\n", gram.c_str(), solve.c_str());
    return 0;
}
