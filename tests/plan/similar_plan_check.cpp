// Stand-alone check of cfk::similar_plan (csrc/als_plan.cpp), the launch plan of als_similar: built together with
// als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as its own process
// (tests/test_similar_host.py). Sweeps recommend_plan_check's grid, checks every invariant from the plan alone and prints
// one JSON line: {"cases": n, "failed": {check: "count, first: shape"}, "split": n, "single": n}.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "als_plan.h"

int main() {
    const int64_t queries[] = {1, 2, 63, 64, 65, 100, 1000, 16383, 16384, 16385, 1 << 17, 1 << 20};
    const int64_t cands[] = {1, 2, 63, 64, 65, 333, 5000, 17770, 1 << 20, (1 << 21) - 1, 1 << 21};
    const int kps[] = {16, 64, 128, 1024};
    const int cus[] = {1, 256};
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0, n_split = 0, n_single = 0;
    for (int64_t nq : queries)
        for (int64_t nc : cands)
            for (int top_n = 1; top_n <= 64; ++top_n)
                for (int kp : kps)
                    for (int cu : cus) {
                        const cfk::SimilarPlan sp = cfk::similar_plan(nq, nc, top_n, kp, cu);
                        const cfk::RecommendPlan& p = sp.sweep;
                        const cfk::RecommendPlan r = cfk::recommend_plan(nq, nc, top_n, kp, cu);
                        ++n_cases;
                        (p.segments > 1 ? n_split : n_single)++;
                        auto check = [&](const char* name, bool ok) {
                            if (ok) return;
                            if (!failed[name]++) {
                                char buf[160];
                                snprintf(buf, sizeof buf, "queries %lld cand %lld top_n %d kp %d cu %d", (long long)nq,
                                         (long long)nc, top_n, kp, cu);
                                first[name] = buf;
                            }
                        };
                        // the segmentation is recommend_plan's, number for number
                        check("segmentation_is_recommend_plan_s",
                              p.user_tile == r.user_tile && p.cand_tile == r.cand_tile && p.user_tiles == r.user_tiles &&
                                  p.segments == r.segments && p.seg_len == r.seg_len && p.lds_bytes == r.lds_bytes &&
                                  p.partial_rows == r.partial_rows);
                        check("segments_at_least_one", p.segments >= 1 && p.segments <= cfk::REC_MAX_SEGMENTS);
                        check("query_tiles_cover_queries",
                              p.user_tiles * p.user_tile >= nq && (p.user_tiles - 1) * p.user_tile < nq);
                        check("segment_is_whole_tiles", p.seg_len > 0 && p.seg_len % p.cand_tile == 0);
                        // segment s = [s seg_len, min(n_cand, (s + 1) seg_len)): walk them
                        int64_t covered = 0;
                        bool exact = true, nonempty = true;
                        for (int64_t s = 0; s < p.segments; ++s) {
                            const int64_t lo = s * p.seg_len, hi = std::min(nc, lo + p.seg_len);
                            exact = exact && lo == covered;
                            nonempty = nonempty && hi > lo;
                            covered = hi > lo ? hi : covered;
                        }
                        check("segments_tile_the_candidates", exact && covered == nc);
                        check("no_empty_segment", nonempty);
                        check("lds_within_the_cu", p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024);
                        // the workspace parts (offset, bytes), their sizes recomputed with overflow-checked arithmetic
                        int64_t rows = 0, list_b = 0, part_b = 0;
                        bool ovf = false;
                        if (p.segments > 1) ovf = __builtin_mul_overflow(nq, p.segments, &rows);
                        ovf = ovf || __builtin_mul_overflow(nq, (int64_t)top_n * 4, &list_b);
                        ovf = ovf || __builtin_mul_overflow(rows, (int64_t)top_n * 4, &part_b);
                        const std::vector<std::pair<int64_t, int64_t>> parts = {
                            {p.off_urows, nq * 8}, {p.off_mrows, nc * 8},   {p.off_idx, list_b},  {p.off_score, list_b},
                            {p.off_part_score, part_b}, {p.off_part_pos, part_b}, {sp.off_inv_q, nq * 4}, {sp.off_inv_c, nc * 4}};
                        bool aligned = true, disjoint = true;
                        int64_t end = 0, total = 0;
                        for (const auto& pt : parts) {   // in layout order: each starts at or after the end of the one before
                            aligned = aligned && pt.first % 256 == 0;
                            disjoint = disjoint && pt.first >= end;
                            ovf = ovf || __builtin_add_overflow(pt.first, pt.second, &end);
                            ovf = ovf || __builtin_add_overflow(total, pt.second, &total);
                        }
                        check("workspace_no_overflow", !ovf && p.partial_rows == rows);
                        check("offsets_aligned", aligned);
                        check("parts_disjoint", disjoint);
                        check("workspace_holds_every_part", sp.workspace_bytes >= end && sp.workspace_bytes > 0 &&
                                                                sp.workspace_bytes <= total + 8 * 256);
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
