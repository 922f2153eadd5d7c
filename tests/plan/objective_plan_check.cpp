// Stand-alone check of cfk::objective_plan (csrc/als_plan.cpp), the launch plan of als_implicit_objective: built together
// with als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as its own process
// (tests/test_objective_host.py). Sweeps every kp (16, 32, 64, 128 at both element sizes; 80, 96, 112 at 8 bytes), cu_count
// in {1, 8, 256} and 1 .. 10^7 queries, checks every invariant from the plans alone and prints one JSON line:
// {"cases": n, "failed": {check: "count, first: shape"}, "plans": {"kp/elem/n/cu": [threads, grid, lds, group lanes]}}.
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
    for (int64_t n : {255, 256, 257, 1279, 1280, 1281, 2047, 2048, 2049, 5000, 480189}) counts.push_back(n);
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0;
    std::string plans;
    for (const Shape& sh : shapes)
        for (int64_t n : counts)
            for (int cu : cus) {
                const int kp = sh.kp, elem = sh.elem;
                auto check = [&](const char* name, bool ok) {
                    if (ok) return;
                    if (!failed[name]++) {
                        char buf[160];
                        snprintf(buf, sizeof buf, "kp %d elem %d n %lld cu %d", kp, elem, (long long)n, cu);
                        first[name] = buf;
                    }
                };
                ++n_cases;
                const cfk::ObjectivePlan p = cfk::objective_plan(kp, elem, n, cu);
                const int lanes = cfk::objective_group_lanes(kp, elem);
                check("threads_are_the_kernel_s", p.threads == cfk::OBJECTIVE_THREADS && p.threads == 256);
                check("grid_within_the_queries", p.grid >= 1 && p.grid <= n);
                check("grid_fills_no_more_than_the_device", p.grid <= (int64_t)cu * cfk::OBJECTIVE_WG_PER_CU);
                check("grid_is_the_smaller_of_the_two", p.grid == n || p.grid == (int64_t)cu * cfk::OBJECTIVE_WG_PER_CU);
                check("lds_is_the_kernel_s", p.lds_bytes == cfk::objective_lds_bytes(kp) &&
                                                 p.lds_bytes == 8 * (int64_t)(kp + cfk::OBJECTIVE_RED_SLOTS));
                check("lds_holds_x_and_the_waves_sums", cfk::OBJECTIVE_RED_SLOTS >= 3 * (cfk::OBJECTIVE_THREADS / 64));
                check("lds_stays_16_byte_aligned", p.lds_bytes % 16 == 0 && p.lds_bytes <= 163840);
                check("lds_does_not_depend_on_the_call", p.lds_bytes == cfk::objective_plan(kp, elem, 1, 1).lds_bytes);
                // a group: a power of two of lanes inside one wave that covers the row's 16-byte pieces
                check("group_is_a_power_of_two", lanes >= 1 && (lanes & (lanes - 1)) == 0);
                check("group_covers_the_row", lanes * 16 >= kp * elem && (lanes == 1 || lanes * 8 < kp * elem));
                check("group_within_a_wave", lanes <= 64 && cfk::OBJECTIVE_THREADS % lanes == 0);
                char key[128];
                snprintf(key, sizeof key, "%s\"%d/%d/%lld/%d\": [%d, %lld, %lld, %d]", plans.empty() ? "" : ", ", kp, elem,
                         (long long)n, cu, p.threads, (long long)p.grid, (long long)p.lds_bytes, lanes);
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
