// Stand-alone check of cfk::recommend_plan (csrc/als_plan.cpp), the launch plan of als_recommend: built together with
// als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as its own process
// (tests/test_recommend_host.py). Sweeps the shapes, checks every invariant from the plan alone and prints one JSON
// line: {"cases": n, "failed": {check: count}, "first": {check: "shape"}, "split": n, "single": n}.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>

#include "als_plan.h"

int main() {
    const int64_t users[] = {1, 2, 63, 64, 65, 100, 1000, 16383, 16384, 16385, 1 << 17, 1 << 20};
    const int64_t cands[] = {1, 2, 63, 64, 65, 333, 5000, 17770, 1 << 20, (1 << 21) - 1, 1 << 21};
    const int kps[] = {16, 64, 128, 1024};
    const int cus[] = {1, 256};
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0, n_split = 0, n_single = 0;
    for (int64_t nu : users)
        for (int64_t nc : cands)
            for (int top_n = 1; top_n <= 64; ++top_n)
                for (int kp : kps)
                    for (int cu : cus) {
                        const cfk::RecommendPlan p = cfk::recommend_plan(nu, nc, top_n, kp, cu);
                        ++n_cases;
                        (p.segments > 1 ? n_split : n_single)++;
                        auto check = [&](const char* name, bool ok) {
                            if (ok) return;
                            if (!failed[name]++) {
                                char buf[160];
                                snprintf(buf, sizeof buf, "users %lld cand %lld top_n %d kp %d cu %d", (long long)nu,
                                         (long long)nc, top_n, kp, cu);
                                first[name] = buf;
                            }
                        };
                        check("segments_at_least_one", p.segments >= 1);
                        check("tiles_are_the_kernel_s", p.user_tile == cfk::REC_USER_TILE && p.cand_tile == cfk::REC_CAND_TILE);
                        check("user_tiles_cover_users", p.user_tiles * p.user_tile >= nu && (p.user_tiles - 1) * p.user_tile < nu);
                        check("segment_is_whole_tiles", p.seg_len > 0 && p.seg_len % p.cand_tile == 0);
                        // segment s = [s seg_len, min(n_cand, (s + 1) seg_len)): walk them
                        int64_t covered = 0;
                        bool exact = true, nonempty = true;
                        for (int64_t s = 0; s < p.segments; ++s) {
                            const int64_t lo = s * p.seg_len, hi = std::min(nc, lo + p.seg_len);
                            exact = exact && lo == covered;
                            nonempty = nonempty && hi > lo;
                            if (s + 1 < p.segments) exact = exact && (hi - lo) % p.cand_tile == 0;
                            covered = hi > lo ? hi : covered;
                        }
                        check("segments_tile_the_candidates", exact && covered == nc);
                        check("no_empty_segment", nonempty);
                        check("segments_fit_the_grid", p.segments <= cfk::REC_MAX_SEGMENTS);
                        check("lds_within_the_cu", p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024 &&
                                                       p.lds_bytes == cfk::recommend_lds_bytes(top_n));
                        check("single_segment_when_users_fill_the_device", p.user_tiles < cu || p.segments == 1);
                        check("split_reaches_the_device",
                              p.segments == 1 || p.user_tiles * p.segments >= std::min<int64_t>(cu, (nc + 63) / 64));
                        // workspace: recomputed with overflow-checked arithmetic
                        int64_t rows = 0, bytes = 0, total = 0;
                        bool ovf = false;
                        if (p.segments > 1) ovf = __builtin_mul_overflow(nu, p.segments, &rows);
                        ovf = ovf || __builtin_mul_overflow(rows, (int64_t)top_n * 8, &bytes);
                        ovf = ovf || __builtin_add_overflow(bytes, nu * 8 + nc * 8 + nu * top_n * 8 + 6 * 256, &total);
                        check("workspace_no_overflow", !ovf && p.partial_rows == rows && p.workspace_bytes > 0 &&
                                                           p.workspace_bytes <= total && p.workspace_bytes >= total - 12 * 256);
                        check("offsets_ascend_aligned",
                              p.off_urows == 0 && p.off_mrows >= nu * 8 && p.off_idx >= p.off_mrows + nc * 8 &&
                                  p.off_score >= p.off_idx + nu * top_n * 4 && p.off_part_score >= p.off_score + nu * top_n * 4 &&
                                  p.off_part_pos >= p.off_part_score + rows * top_n * 4 &&
                                  p.workspace_bytes >= p.off_part_pos + rows * top_n * 4 &&
                                  (p.off_mrows | p.off_idx | p.off_score | p.off_part_score | p.off_part_pos) % 256 == 0);
                    }
    printf("{\"cases\": %lld, \"split\": %lld, \"single\": %lld, \"failed\": {", (long long)n_cases, (long long)n_split,
           (long long)n_single);
    bool sep = false;
    for (auto& kv : failed)
        if (kv.second) {
            printf("%s\"%s\": \"%lld, first: %s\"", sep ? ", " : "", kv.first.c_str(), (long long)kv.second,
                   first[kv.first].c_str());
            sep = true;
        }
    printf("}}\n");
    return 0;
}
