// Stand-alone check of cfk::rank_plan (csrc/als_plan.cpp), the launch plan of als_rank_targets: built together with
// als_plan.cpp by the host compiler under AddressSanitizer + UBSan and run as its own process
// (tests/test_rank_host.py). Sweeps the shapes, checks every invariant from the plan alone and prints one JSON
// line: {"cases": n, "failed": {check: "count, first: shape"}, "split": n, "single": n}.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>

#include "als_plan.h"

int main() {
    const int64_t targets[] = {1, 2, 63, 64, 65, 100, 1000, 16383, 16384, 16385, 1 << 17, 1 << 20, (1 << 21) - 1, 1 << 21};
    const int64_t cands[] = {1, 2, 63, 64, 65, 333, 5000, 17770, 1 << 20, (1 << 21) - 1, 1 << 21};
    const int kps[] = {16, 64, 128, 1024};
    const int cus[] = {1, 256};
    std::map<std::string, int64_t> failed;
    std::map<std::string, std::string> first;
    int64_t n_cases = 0, n_split = 0, n_single = 0;
    for (int64_t nt : targets)
        for (int64_t nc : cands)
            for (int kp : kps)
                for (int cu : cus) {
                    const cfk::RankPlan p = cfk::rank_plan(nt, nc, kp, cu);
                    ++n_cases;
                    (p.segments > 1 ? n_split : n_single)++;
                    auto check = [&](const char* name, bool ok) {
                        if (ok) return;
                        if (!failed[name]++) {
                            char buf[160];
                            snprintf(buf, sizeof buf, "targets %lld cand %lld kp %d cu %d", (long long)nt, (long long)nc, kp, cu);
                            first[name] = buf;
                        }
                    };
                    check("segments_at_least_one", p.segments >= 1);
                    check("tiles_are_the_kernel_s", p.tgt_tile == cfk::RANK_TGT_TILE && p.cand_tile == cfk::RANK_CAND_TILE);
                    check("target_tiles_cover_targets", p.tgt_tiles * p.tgt_tile >= nt && (p.tgt_tiles - 1) * p.tgt_tile < nt);
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
                    check("segments_fit_the_grid", p.segments <= cfk::RANK_MAX_SEGMENTS && p.segments <= 65535);
                    check("lds_within_the_cu", p.lds_bytes > 0 && p.lds_bytes <= 160 * 1024 && p.lds_bytes == cfk::rank_lds_bytes());
                    check("single_segment_when_targets_fill_the_device", p.tgt_tiles < cu || p.segments == 1);
                    check("split_reaches_the_device",
                          p.segments == 1 || p.tgt_tiles * p.segments >= std::min<int64_t>(cu, (nc + 63) / 64));
                    // workspace: recomputed with overflow-checked arithmetic (24 bytes per target, 8 per candidate)
                    int64_t tb = 0, cb = 0, total = 0;
                    bool ovf = __builtin_mul_overflow(nt, (int64_t)24, &tb);
                    ovf = ovf || __builtin_mul_overflow(nc, (int64_t)8, &cb);
                    ovf = ovf || __builtin_add_overflow(tb, cb, &total);
                    check("workspace_no_overflow", !ovf && p.workspace_bytes >= total && p.workspace_bytes <= total + 6 * 256);
                    check("offsets_ascend_aligned",
                          p.off_trow == 0 && p.off_tpos >= nt * 8 && p.off_tuser >= p.off_tpos + nt * 4 &&
                              p.off_score >= p.off_tuser + nt * 4 && p.off_rank >= p.off_score + nt * 4 &&
                              p.off_mrows >= p.off_rank + nt * 4 && p.workspace_bytes >= p.off_mrows + nc * 8 &&
                              (p.off_tpos | p.off_tuser | p.off_score | p.off_rank | p.off_mrows | p.workspace_bytes) % 256 == 0);
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
