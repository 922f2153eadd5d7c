// Stand-alone check of cfk::foldin_plan (csrc/als_plan.cpp), the launch plan of als_fold_in: built together with
// als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as its own process
// (tests/test_foldin_host.py). Sweeps every kp, both element sizes and n_queries from 1 to 10^7, checks every invariant
// from the plan alone and prints one JSON line:
// {"cases": n, "failed": {check: "count, first: shape"}, "plans": {"kp/elem/n_queries/cu": [threads, grid, batch, lds]}}.
// With the argument `generic` it sweeps instead the strides only fp64 engines have (80, 96, 112: 65..112 features are on
// the generic solve path there, whose stride is the next multiple of 16), at 8-byte elements.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "als_plan.h"

int main(int argc, char** argv) {
    const bool generic = argc > 1 && !strcmp(argv[1], "generic");
    const std::vector<int> kps = generic ? std::vector<int>{80, 96, 112} : std::vector<int>{16, 32, 64, 128};
    const std::vector<int> elems = generic ? std::vector<int>{8} : std::vector<int>{4, 8};
    const int cus[] = {1, 8, 256};
    std::vector<int64_t> queries;
    for (int64_t n = 1; n <= 70; ++n) queries.push_back(n);
    for (int64_t n = 100; n <= 10000000; n *= 10)
        for (int64_t d = -1; d <= 1; ++d) queries.push_back(n + d);
    for (int64_t n : {255, 256, 257, 511, 512, 513, 1024, 2047, 2048, 2049, 4096, 5000, 65536, 1234567}) queries.push_back(n);
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0;
    std::string plans;
    for (int kp : kps)
        for (int elem : elems)
            for (int cu : cus)
                for (int64_t nq : queries) {
                    const cfk::FoldinPlan p = cfk::foldin_plan(kp, elem, nq, cu);
                    ++n_cases;
                    auto check = [&](const char* name, bool ok) {
                        if (ok) return;
                        if (!failed[name]++) {
                            char buf[160];
                            snprintf(buf, sizeof buf, "kp %d elem %d queries %lld cu %d", kp, elem, (long long)nq, cu);
                            first[name] = buf;
                        }
                    };
                    check("threads_are_the_kernel_s", p.threads == cfk::FOLDIN_THREADS && p.threads == 256);
                    check("lds_within_the_cu", p.lds_bytes > 0 && p.lds_bytes <= 163840);
                    check("lds_is_the_kernel_s", p.lds_bytes == cfk::foldin_lds_bytes(kp, elem, p.batch));
                    check("lds_holds_every_region",
                          p.lds_bytes >= (int64_t)elem * ((int64_t)(kp / 16) * (kp / 16 + 1) / 2 * 256 +
                                                          (int64_t)p.batch * kp + 4 * kp + p.batch));
                    check("staged_rows_stay_16_byte_aligned",
                          ((int64_t)cfk::foldin_tiles(kp) * cfk::FOLDIN_TILE_ELEMS * elem) % 16 == 0 &&
                              ((int64_t)cfk::foldin_pitch(kp) * elem) % 16 == 0);
                    check("operand_reads_conflict_free", cfk::foldin_pitch(kp) % 32 == 16 && cfk::foldin_pitch(kp) >= kp);
                    check("batch_whole_mfma_steps", p.batch >= 4 && p.batch % 4 == 0 && p.batch <= cfk::FOLDIN_MAX_BATCH);
                    check("grid_within_the_queries", p.grid >= 1 && p.grid <= nq);
                    check("grid_fills_no_more_than_the_device", p.grid <= (int64_t)cu * cfk::FOLDIN_MAX_WG_PER_CU);
                    check("grid_fits_the_lds", p.grid <= (int64_t)cu * (163840 / p.lds_bytes > 0 ? 163840 / p.lds_bytes : 1));
                    char key[96];
                    snprintf(key, sizeof key, "%s\"%d/%d/%lld/%d\": [%d, %lld, %d, %lld]", plans.empty() ? "" : ", ", kp, elem,
                             (long long)nq, cu, p.threads, (long long)p.grid, p.batch, (long long)p.lds_bytes);
                    plans += key;
                }
    printf("{\"cases\": %lld, \"failed\": {", (long long)n_cases);
    bool sep = false;
    for (auto& kv : failed)
        if (kv.second) {
            printf("%s\"%s\": \"%lld, first: %s\"", sep ? ", " : "", kv.first.c_str(), (long long)kv.second,
                   first[kv.first].c_str());
            sep = true;
        }
    printf("}, \"plans\": {%s}}\n", plans.c_str());
    return 0;
}
