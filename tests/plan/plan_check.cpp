// plan_check -- builds the work plan (csrc/als_plan.h) of small synthetic blocks on the CPU, checks the plan's
// invariants from the plan alone and prints one JSON line per case: the layout, the counts, one boolean per invariant
// and an FNV-1a digest of every output array (tests/golden/plan_digests.json pins the digests). One more line holds the
// launch geometry of the any-k path (generic_plan) for every padded stride, checked and digested the same way.
// tests/test_plan_host.py compiles this file with als_plan.cpp under -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "als_plan.h"

using namespace cfk;

namespace {

constexpr int64_t BE = BLOCK_ENTRIES;
constexpr int XR = 8;
// whole filler rows of the two forced-ranges cases: enough for aligned queues (see the XCD queue checks)
constexpr int64_t FILL64 = 22, FILL128 = 25;

// Where a row's blocks sit in the opposite table: first slots spread evenly over [lo, hi) of it (fractions); `last_alone`
// puts the row's last block at the table's last slot instead (alone in range 7 when hi <= 7/8).
struct Span {
    double lo = 0.0, hi = 1.0;
    bool last_alone = false;
};

struct Case {
    std::string name;
    PlanKnobs kn;
    BlockShape sh;
    std::vector<int64_t> deg;
    std::map<size_t, Span> span;   // rows not listed spread over the whole table
    bool layout_only = false;      // the automatic rules of huge blocks: the layout is all there is to check
};

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* c = (const unsigned char*)p;
        for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    }
    void i64(int64_t v) { bytes(&v, 8); }
    template <class T>
    void vec(const std::vector<T>& v) {
        i64((int64_t)v.size());
        if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
    }
};

bool non_increasing(const std::vector<Task>& v) {
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i].nsteps > v[i - 1].nsteps) return false;
    return true;
}

bool task_less(const Task& a, const Task& b) { return std::memcmp(&a, &b, sizeof(Task)) < 0; }
bool task_eq(const Task& a, const Task& b) { return std::memcmp(&a, &b, sizeof(Task)) == 0; }

struct Checks {
    std::vector<std::pair<const char*, bool>> v;
    void add(const char* name, bool ok) { v.emplace_back(name, ok); }
};

void run(const Case& c) {
    const int64_t n_rows = (int64_t)c.deg.size();
    std::vector<int64_t> begin(n_rows + 1);
    int64_t o = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        begin[i] = o;
        o += (c.deg[i] + BE - 1) / BE * BE;
    }
    begin[n_rows] = o;
    const BlockLayout L = plan_layout(c.kn, c.sh, c.deg);
    Fnv f;
    f.i64(L.chunk);
    f.i64(L.ilv);
    f.i64(L.ranges);
    f.i64(L.presplit);
    printf("{\"case\": \"%s\", \"layout\": {\"chunk\": %lld, \"ilv\": %lld, \"ranges\": %d, \"presplit\": %d}", c.name.c_str(),
           (long long)L.chunk, (long long)L.ilv, (int)L.ranges, (int)L.presplit);
    if (c.layout_only) {
        printf(", \"digest\": \"%016llx\"}\n", (unsigned long long)f.h);
        return;
    }
    const int64_t n_blocks = o / BE;
    std::vector<int64_t> row_of_block((size_t)n_blocks);
    std::vector<int32_t> bfirst;
    if (L.ranges) bfirst.resize((size_t)n_blocks);
    for (int64_t i = 0; i < n_rows; ++i) {
        const int64_t nb = (c.deg[i] + BE - 1) / BE, b0 = begin[i] / BE;
        const auto it = c.span.find((size_t)i);
        const Span sp = it == c.span.end() ? Span() : it->second;
        for (int64_t q = 0; q < nb; ++q) {
            row_of_block[(size_t)(b0 + q)] = i;
            if (!L.ranges) continue;
            double fr = sp.lo + (sp.hi - sp.lo) * (double)q / (double)nb;
            int64_t slot = (int64_t)(fr * (double)c.sh.n_opp_rows);
            if (sp.last_alone && q == nb - 1) slot = c.sh.n_opp_rows - 1;
            bfirst[(size_t)(b0 + q)] = (int32_t)std::min(slot, c.sh.n_opp_rows - 1);
        }
    }
    const BlockPlan P = plan_build(c.kn, c.sh, L, c.deg, begin, bfirst);
    if (P.error) {
        printf(", \"error\": \"%s\"}\n", P.error);
        return;
    }
    auto range_of = [&](int64_t src_block) {
        return (int)std::min<int64_t>(XR - 1, (int64_t)bfirst[(size_t)src_block] * XR / c.sh.n_opp_rows);
    };
    auto src = [&](int64_t pos) { return P.perm.empty() ? pos : (int64_t)P.perm[(size_t)pos]; };
    auto interleaved = [&](int64_t row) { return L.ilv > 0 && c.deg[row] > L.ilv; };
    Checks ck;

    // ---- perm: a permutation of the blocks, row onto row, identity outside interleaved rows; empty without them
    {
        bool ok = true, any_ilv = false;
        for (int64_t i = 0; i < n_rows; ++i) any_ilv = any_ilv || interleaved(i);
        if (!any_ilv) ok = P.perm.empty();
        else if ((int64_t)P.perm.size() != n_blocks) ok = false;
        else {
            std::vector<int> seen((size_t)n_blocks, 0);
            for (int64_t p = 0; p < n_blocks && ok; ++p) {
                const int64_t s = P.perm[(size_t)p];
                if (s < 0 || s >= n_blocks || seen[(size_t)s]++) ok = false;
                else if (row_of_block[(size_t)s] != row_of_block[(size_t)p]) ok = false;
                else if (!interleaved(row_of_block[(size_t)p]) && s != p) ok = false;
            }
        }
        ck.add("perm_is_row_permutation", ok);
    }

    // ---- coverage: FULL + PARTIAL + entry-space tasks cover every block of the permuted in-block once
    std::vector<Task> work = P.tasks;
    for (int d = 0; d < 3; ++d) work.insert(work.end(), P.dual[d].begin(), P.dual[d].end());
    std::vector<int64_t> row_ent((size_t)n_rows, 0), row_full((size_t)n_rows, 0), row_part((size_t)n_rows, 0);
    {
        bool kinds = true, fields = true, cover = true, last_block = true;
        std::vector<int> covered((size_t)n_blocks, 0);
        for (const Task& t : work) {
            if (t.kind != TASK_FULL && t.kind != TASK_PARTIAL) { kinds = false; continue; }
            if (t.row < 0 || t.row >= n_rows || t.nent < 0) { fields = false; continue; }
            const int64_t d = c.deg[t.row], nb = (d + BE - 1) / BE, b0 = begin[t.row] / BE;
            if (t.begin % BE != 0 || t.nsteps != (t.nent + 3) / 4 || t.ndeg != d) fields = false;
            if (t.kind == TASK_FULL && t.slot != -1) fields = false;
            (t.kind == TASK_FULL ? row_full : row_part)[(size_t)t.row]++;
            row_ent[(size_t)t.row] += t.nent;
            const int64_t tb = (t.nent + BE - 1) / BE, p0 = t.begin / BE;
            if (p0 < b0 || p0 + tb > b0 + nb) { cover = false; continue; }
            int64_t real = 0;   // real entries of the task's blocks: the row's last source block holds the padding
            for (int64_t q = 0; q < tb; ++q) {
                covered[(size_t)(p0 + q)]++;
                const bool is_last = src(p0 + q) == b0 + nb - 1;
                real += is_last ? d - BE * (nb - 1) : BE;
                if (is_last && q != tb - 1) last_block = false;
            }
            if (real != t.nent) last_block = false;
        }
        for (int v : covered) cover = cover && v == 1;
        bool sums = true, one_way = true;
        for (int64_t i = 0; i < n_rows; ++i) {
            sums = sums && row_ent[(size_t)i] == c.deg[i];
            // a row is one FULL task, or PARTIAL tasks (with their REDUCE, below)
            one_way = one_way && ((row_full[(size_t)i] == 1 && row_part[(size_t)i] == 0) ||
                                  (row_full[(size_t)i] == 0 && row_part[(size_t)i] >= 1));
        }
        ck.add("work_tasks_are_full_or_partial", kinds);
        ck.add("task_fields_consistent", fields);
        ck.add("blocks_covered_once", cover);
        ck.add("row_nent_sums_to_deg", sums);
        ck.add("padded_block_last_nent_real", last_block);
        ck.add("row_full_xor_partial", one_way);
    }

    // ---- PARTIAL slots are 0 .. slots-1, each once; one REDUCE per split row over exactly its slots
    {
        std::vector<int> used((size_t)std::max<int64_t>(P.slots, 0), 0);
        std::vector<int64_t> lo((size_t)n_rows, INT64_MAX), hi((size_t)n_rows, -1);
        bool ok = true;
        int64_t n_partial = 0;
        for (const Task& t : work) {
            if (t.kind != TASK_PARTIAL) continue;
            ++n_partial;
            if (t.slot < 0 || t.slot >= P.slots || used[(size_t)t.slot]++) { ok = false; continue; }
            lo[(size_t)t.row] = std::min<int64_t>(lo[(size_t)t.row], t.slot);
            hi[(size_t)t.row] = std::max<int64_t>(hi[(size_t)t.row], t.slot);
        }
        ck.add("partial_slots_unique", ok && n_partial == P.slots);
        bool red = true;
        std::vector<int> n_red((size_t)n_rows, 0);
        std::vector<std::pair<int64_t, int64_t>> ranges;
        for (const Task& r : P.reduce) {
            if (r.kind != TASK_REDUCE || r.row < 0 || r.row >= n_rows) { red = false; continue; }
            n_red[(size_t)r.row]++;
            if (row_part[(size_t)r.row] == 0 || r.ndeg != c.deg[r.row]) red = false;
            // the row's slots are r.nsteps distinct numbers: with these bounds they are exactly [slot, slot + nsteps)
            if (r.slot != lo[(size_t)r.row] || r.slot + r.nsteps - 1 != hi[(size_t)r.row] ||
                r.nsteps != row_part[(size_t)r.row])
                red = false;
            ranges.emplace_back(r.slot, r.slot + r.nsteps);
        }
        for (int64_t i = 0; i < n_rows; ++i) red = red && n_red[(size_t)i] == (row_part[(size_t)i] > 0 ? 1 : 0);
        std::sort(ranges.begin(), ranges.end());
        int64_t at = 0;
        for (auto& r : ranges) {
            red = red && r.first == at;
            at = r.second;
        }
        ck.add("one_reduce_per_split_row_tiling_slots", red && at == P.slots);
    }

    // ---- longest first
    const bool queues = L.ranges && P.ilv_tasks > 0;   // the main launch is dealt into XCD queues
    {
        bool ok = non_increasing(P.reduce);
        for (int d = 0; d < 3; ++d) ok = ok && non_increasing(P.dual[d]);
        if (!queues) ok = ok && non_increasing(P.tasks);
        ck.add("lists_longest_first", ok);
    }

    // ---- XCD queues. A chunk task belongs to the range of its blocks; the main launch is the queues' tasks dealt four
    // at a time, queue 0 .. 7, so each range's chunk tasks keep their queue's longest-first order wherever they land.
    // Workgroup w (tasks 4w .. 4w+3) is queue w % 8 exactly when every queue ends at its equal share of the launch:
    // whole tasks only go to queues short of their share (4 tasks per workgroup at w = x mod 8), so that happens when
    // the task count is a multiple of 4 and no range has more chunk tasks than its share. The dealing promises the
    // alignment then, and only then (elsewhere the tail shifts: speed only); `queues_aligned` says which it is, and
    // the two position checks apply to aligned plans.
    bool aligned = false;
    if (queues) {
        bool whole = true, reaches = true, range_sorted = true;
        int32_t prev_r[XR];
        int64_t n_chunk[XR] = {};
        for (int x = 0; x < XR; ++x) prev_r[x] = INT32_MAX;
        std::vector<int> task_range(P.tasks.size(), -1);
        std::vector<std::vector<int>> has((size_t)n_rows, std::vector<int>(XR, 0));
        for (size_t p = 0; p < P.tasks.size(); ++p) {
            const Task& t = P.tasks[p];
            if (t.kind != TASK_PARTIAL || !interleaved(t.row)) continue;
            const int64_t tb = (t.nent + BE - 1) / BE, p0 = t.begin / BE;
            const int x = range_of(src(p0));
            for (int64_t q = 0; q < tb; ++q)
                if (range_of(src(p0 + q)) != x) whole = false;
            task_range[p] = x;
            n_chunk[x]++;
            has[(size_t)t.row][x] = 1;
            if (t.nsteps > prev_r[x]) range_sorted = false;
            prev_r[x] = t.nsteps;
        }
        for (int64_t i = 0; i < n_rows; ++i) {
            if (!interleaved(i)) continue;
            const int64_t nb = (c.deg[i] + BE - 1) / BE, b0 = begin[i] / BE;
            for (int64_t q = 0; q < nb; ++q)
                if (!has[(size_t)i][range_of(b0 + q)]) reaches = false;
        }
        ck.add("chunk_task_blocks_in_one_range", whole);
        ck.add("row_has_chunk_in_every_range_it_reaches", reaches);
        ck.add("range_chunks_longest_first", range_sorted);
        const int64_t total = (int64_t)P.tasks.size(), wgs = (total + 3) / 4;
        aligned = total % 4 == 0;
        for (int x = 0; x < XR; ++x) aligned = aligned && n_chunk[x] <= 4 * ((wgs - x + XR - 1) / XR);
        if (aligned) {
            bool sorted = true, in_queue = true;
            int32_t prev[XR];
            for (int x = 0; x < XR; ++x) prev[x] = INT32_MAX;
            for (size_t p = 0; p < P.tasks.size(); ++p) {
                const int x = (int)((p / 4) % XR);
                if (P.tasks[p].nsteps > prev[x]) sorted = false;
                prev[x] = P.tasks[p].nsteps;
                if (task_range[p] >= 0 && task_range[p] != x) in_queue = false;
            }
            ck.add("queue_positions_longest_first", sorted);
            ck.add("chunk_tasks_in_their_range_queue", in_queue);
        }
    }

    // ---- entry space
    {
        const int max_blocks = c.sh.path != Path::MFMA_SPLIT ? 0 : c.sh.kp == 128 ? 3 : c.sh.kp == 64 ? 1 : 0;
        auto qualifies = [&](const Task& t) {
            return t.kind == TASK_FULL && t.ndeg > 0 && t.ndeg <= c.sh.k && (t.nent + BE - 1) / BE <= max_blocks;
        };
        bool ok = true;
        for (int d = 0; d < 3; ++d) {
            if (d >= max_blocks || !c.kn.dual) ok = ok && P.dual[d].empty();
            for (const Task& t : P.dual[d]) ok = ok && qualifies(t) && (t.nent + BE - 1) / BE - 1 == d;
        }
        ck.add("entry_space_tasks_qualify", ok);
        bool none_left = true;
        if (c.kn.dual)
            for (const Task& t : P.tasks) none_left = none_left && !qualifies(t);
        ck.add("no_qualifying_task_left_in_main", none_left);
    }

    // ---- sq_all: every FULL + PARTIAL task, nothing else
    {
        std::vector<Task> a = work, b = P.sq_all;
        std::sort(a.begin(), a.end(), task_less);
        std::sort(b.begin(), b.end(), task_less);
        ck.add("sq_all_complete", a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin(), task_eq));
    }

    // ---- chunk partition: 4 row chunks, the second one empty
    {
        const int64_t bounds[5] = {0, std::min<int64_t>(3, n_rows), std::min<int64_t>(3, n_rows),
                                   std::max<int64_t>(n_rows / 2, std::min<int64_t>(3, n_rows)), n_rows};
        const std::vector<Task>* lists[5] = {&P.tasks, &P.reduce, &P.dual[0], &P.dual[1], &P.dual[2]};
        bool ok = true;
        for (const std::vector<Task>* in : lists) {
            std::vector<Task> out;
            std::vector<int32_t> off;
            partition_by_chunk(*in, 4, bounds, out, off);
            std::vector<Task> want;
            std::vector<int32_t> woff(1, 0);
            for (int ch = 0; ch < 4; ++ch) {
                for (const Task& t : *in)
                    if (t.row >= bounds[ch] && t.row < bounds[ch + 1]) want.push_back(t);
                woff.push_back((int32_t)want.size());
            }
            ok = ok && off == woff && out.size() == want.size() && std::equal(out.begin(), out.end(), want.begin(), task_eq);
            f.vec(out);
            f.vec(off);
        }
        ck.add("chunk_partition_stable", ok);
    }

    f.vec(P.tasks);
    f.vec(P.reduce);
    for (int d = 0; d < 3; ++d) f.vec(P.dual[d]);
    f.vec(P.sq_all);
    f.vec(P.perm);
    f.i64(P.slots);
    f.i64(P.ilv_rows);
    f.i64(P.ilv_tasks);

    int64_t n_full = 0;
    for (const Task& t : P.tasks) n_full += t.kind == TASK_FULL;
    printf(", \"n_rows\": %lld, \"n_blocks\": %lld, \"n_tasks\": %zu, \"n_full\": %lld, \"n_reduce\": %zu, "
           "\"n_dual\": [%zu, %zu, %zu], \"slots\": %lld, \"ilv_rows\": %lld, \"ilv_tasks\": %lld, \"perm\": %zu, "
           "\"queues\": %d, \"queues_aligned\": %d, \"checks\": {",
           (long long)n_rows, (long long)n_blocks, P.tasks.size(), (long long)n_full, P.reduce.size(), P.dual[0].size(),
           P.dual[1].size(), P.dual[2].size(), (long long)P.slots, (long long)P.ilv_rows, (long long)P.ilv_tasks,
           P.perm.size(), (int)queues, (int)aligned);
    for (size_t i = 0; i < ck.v.size(); ++i)
        printf("%s\"%s\": %s", i ? ", " : "", ck.v[i].first, ck.v[i].second ? "true" : "false");
    printf("}, \"deg\": [");
    for (int64_t i = 0; i < n_rows; ++i) printf("%s%lld", i ? ", " : "", (long long)c.deg[i]);
    printf("], \"digest\": \"%016llx\"}\n", (unsigned long long)f.h);
}

// ---- the cases -----------------------------------------------------------------------------------------------------

BlockShape shape(Path p, int k, int kp, int64_t n_opp_rows, int cu = 256) {
    BlockShape s;
    s.path = p;
    s.k = k;
    s.kp = kp;
    s.cu_count = cu;
    s.n_opp_rows = n_opp_rows;
    return s;
}

// Every block boundary of a short row, and long rows on and around the active chunk length c.
std::vector<int64_t> boundary_degrees(int64_t c) {
    return {0, 1, 31, 32, 33, 64, 65, 96, 97, 128, c, c + 1, 2 * c, 2 * c + 1, 7 * c + 5};
}

std::vector<int64_t> rows_of(int64_t n, int64_t d) { return std::vector<int64_t>((size_t)n, d); }
std::vector<int64_t> cat(std::vector<int64_t> a, const std::vector<int64_t>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

std::vector<Case> cases() {
    std::vector<Case> v;
    auto add = [&](const char* name, const PlanKnobs& kn, const BlockShape& sh, std::vector<int64_t> deg) -> Case& {
        Case c;
        c.name = name;
        c.kn = kn;
        c.sh = sh;
        c.deg = std::move(deg);
        v.push_back(c);
        return v.back();
    };
    PlanKnobs c64;   // contiguous chunks of 64 entries
    c64.chunk = 64;

    // -- paths, chunk 64, a table far too small to interleave
    add("valu_kp16", c64, shape(Path::VALU, 10, 16, 1000), boundary_degrees(64));
    add("mfma_kp32", c64, shape(Path::MFMA, 32, 32, 1000), boundary_degrees(64));
    add("split_kp32", c64, shape(Path::MFMA_SPLIT, 32, 32, 1000), boundary_degrees(64));
    add("split_kp64_k64", c64, shape(Path::MFMA_SPLIT, 64, 64, 1000), boundary_degrees(64));
    // a 1-block row of 41 > k entries stays out of entry space
    add("split_kp64_k40", c64, shape(Path::MFMA_SPLIT, 40, 64, 1000), cat(boundary_degrees(64), {40, 41}));
    add("split_kp128_k128", c64, shape(Path::MFMA_SPLIT, 128, 128, 1000), boundary_degrees(64));
    // an 80-entry, 3-block row with 80 > k stays out
    add("split_kp128_k70", c64, shape(Path::MFMA_SPLIT, 70, 128, 1000), cat(boundary_degrees(64), {70, 71, 80}));
    {
        PlanKnobs kn;   // with a chunk of 128 the 3-block rows are whole rows, the candidates of entry space
        kn.chunk = 128;
        add("split_kp128_k128_chunk128", kn, shape(Path::MFMA_SPLIT, 128, 128, 1000), boundary_degrees(128));
        add("split_kp128_k70_chunk128", kn, shape(Path::MFMA_SPLIT, 70, 128, 1000),
            cat(boundary_degrees(128), {70, 71, 80}));
    }
    add("generic_k130", c64, shape(Path::GENERIC, 130, 144, 1000), cat(boundary_degrees(64), {100000}));
    {
        PlanKnobs kn = c64;
        kn.dual = false;
        add("split_kp64_dual_off", kn, shape(Path::MFMA_SPLIT, 64, 64, 1000), boundary_degrees(64));
        PlanKnobs def;   // no override: the lower clamp of the chunk formula (1024 entries)
        add("split_kp64_default_chunk", def, shape(Path::MFMA_SPLIT, 64, 64, 1000), boundary_degrees(1024));
    }

    // -- interleave forced on, chunk c (so the interleave length is c too): the boundary rows, then rows whose blocks
    // reach 1, 2 and all 8 ranges of the table, a row whose padded 3-entry last block is alone in its range, and whole
    // rows (too long for entry space) enough that every queue's share of the launch covers its range's chunk tasks
    auto ilv_deg = [&](int64_t c, int64_t fill) {
        return cat(cat(boundary_degrees(c), {c + 1, 2 * c + 1, 40 * c + 7, 5 * c + 3}), cat(rows_of(24, c - 14), rows_of(fill, c)));
    };
    auto ilv_case = [&](const std::string& name, PlanKnobs kn, int k, int kp, int64_t c, int64_t fill) {
        kn.chunk = c;
        kn.interleave = 1;
        Case& cs = add(name.c_str(), kn, shape(Path::MFMA_SPLIT, k, kp, 1000), ilv_deg(c, fill));
        const size_t r0 = boundary_degrees(c).size();
        cs.span[r0 + 0] = Span{0.26, 0.37, false};   // all blocks in range 2
        cs.span[r0 + 1] = Span{0.40, 0.60, false};   // blocks in ranges 3 and 4
        cs.span[r0 + 3] = Span{0.0, 0.25, true};     // blocks in ranges 0 and 1, the 3-entry last one in 7
    };
    for (int rg : {0, 1}) {
        PlanKnobs kn;
        kn.xcd_ranges = rg;
        const std::string sfx = rg ? "_ranges" : "_noranges";
        ilv_case("ilv_kp64" + sfx, kn, 64, 64, 64, FILL64);
        // kp 128: k = 70 and a chunk of 128, so that the whole rows of 114 and 128 entries stay in the main launch
        ilv_case("ilv_kp128" + sfx, kn, 70, 128, 128, FILL128);
    }
    {
        PlanKnobs kn;
        kn.presplit = 0;
        ilv_case("ilv_kp64_presplit_off", kn, 64, 64, 64, 23);
        kn.presplit = -1;
        kn.ilv_chunk = 32;   // rows between the interleave length and the chunk
        ilv_case("ilv_kp64_ilv32_chunk64", kn, 64, 64, 64, 23);
        kn = c64;
        kn.interleave = 0;   // off beats a table that would interleave
        add("ilv_off_kp128", kn, shape(Path::MFMA_SPLIT, 128, 128, 100000, 1), ilv_deg(64, 23));
    }

    // -- automatic rules, one case either side of each threshold (table bytes = (n_opp_rows + 1) * 4 * kp); one compute
    // unit keeps the concurrency thresholds small
    const PlanKnobs def;
    const std::vector<int64_t> busy = cat(rows_of(20, 12288), boundary_degrees(1024));   // passes the 1.5x rule at 1 CU
    add("auto_table_32mb_at", def, shape(Path::MFMA_SPLIT, 64, 64, (32 << 20) / 256 - 1, 1), busy);
    add("auto_table_32mb_over", def, shape(Path::MFMA_SPLIT, 64, 64, (32 << 20) / 256, 1), busy);
    add("auto_table_256mib_at_kp64", def, shape(Path::MFMA_SPLIT, 64, 64, (256 << 20) / 256 - 1, 1), busy);
    add("auto_table_256mib_over_kp64", def, shape(Path::MFMA_SPLIT, 64, 64, (256 << 20) / 256, 1), busy);
    add("auto_table_256mib_at_kp128", def, shape(Path::MFMA_SPLIT, 128, 128, (256 << 20) / 512 - 1, 1), busy);
    add("auto_table_256mib_over_kp128", def, shape(Path::MFMA_SPLIT, 128, 128, (256 << 20) / 512, 1), busy);
    // 1.5 x 16 resident waves x 10,240 entries = 245,760 entries in rows longer than 10,240
    add("auto_concurrency_kp64_at", def, shape(Path::MFMA_SPLIT, 64, 64, 400000, 1), cat(rows_of(20, 12288), {10240, 5}));
    add("auto_concurrency_kp64_under", def, shape(Path::MFMA_SPLIT, 64, 64, 400000, 1),
        cat(cat(rows_of(19, 12288), {12287}), {10240, 5}));
    // the rule does not apply beyond a 128 MiB table
    add("auto_concurrency_kp64_big_table", def, shape(Path::MFMA_SPLIT, 64, 64, 600000, 1), {12288, 10240, 5});
    {
        // kp 128: 16,384 when rows longer than it hold 4 x 4 resident waves x 16,384 = 262,144 entries, else 4,096
        PlanKnobs kn;
        kn.chunk = 32768;
        add("auto_kp128_len_at", kn, shape(Path::MFMA_SPLIT, 128, 128, 100000, 1), cat(rows_of(8, 32768), {16384, 4097, 7}));
        add("auto_kp128_len_under", kn, shape(Path::MFMA_SPLIT, 128, 128, 100000, 1),
            cat(cat(rows_of(7, 32768), {32767}), {16384, 4097, 7}));
    }
    add("auto_ranges_128mib_at", def, shape(Path::MFMA_SPLIT, 64, 64, (128 << 20) / 256 - 1, 1), busy);
    add("auto_ranges_128mib_over", def, shape(Path::MFMA_SPLIT, 64, 64, (128 << 20) / 256, 1), busy);
    add("auto_presplit_8mb_at", def, shape(Path::MFMA_SPLIT, 64, 64, (8 << 20) / 256 - 1, 1), boundary_degrees(1024));
    add("auto_presplit_8mb_over", def, shape(Path::MFMA_SPLIT, 64, 64, (8 << 20) / 256, 1), boundary_degrees(1024));
    {
        // the 2^24-row guard beats knobs that force the interleave and the pre-split table
        PlanKnobs kn = c64;
        kn.interleave = 1;
        kn.presplit = 1;
        add("guard_rows_2p24_under", kn, shape(Path::MFMA_SPLIT, 64, 64, (1 << 24) - 2), boundary_degrees(64));
        add("guard_rows_2p24_at", kn, shape(Path::MFMA_SPLIT, 64, 64, (1 << 24) - 1), boundary_degrees(64));
    }
    // the chunk formula nnz_padded / 4096 between and at its clamps: layouts of blocks too large to build here
    Case& mid = add("layout_chunk_formula_mid", def, shape(Path::MFMA_SPLIT, 64, 64, 1000), rows_of(8000, 2000));
    mid.layout_only = true;
    Case& top = add("layout_chunk_formula_top", def, shape(Path::MFMA_SPLIT, 64, 64, 1000), rows_of(4, 1000000000));
    top.layout_only = true;
    return v;
}

// The launch geometry of the any-k path (generic_plan) for every padded stride 16, 32, ..., 1024 in both precisions:
// one row [precision, kp, g_in_lds, batch, lds_bytes, slab_elems] each, the invariants the kernel relies on, and a
// digest of all 128 plans.
void run_generic_plan() {
    Fnv f;
    Checks ck;
    bool batch_ok = true, lds_ok = true, tri_ok = true, mono_ok = true, slab_ok = true, stage_ok = true;
    printf("{\"case\": \"generic_launch_plan\", \"rows\": [");
    for (int precision = 0; precision < 2; ++precision) {
        const bool f64 = precision != 0;
        const int64_t elem = f64 ? 8 : 4;
        bool on_slab = false;
        for (int kp = 16; kp <= GENERIC_MAX_KP; kp += 16) {
            const GenericPlan p = generic_plan(precision, kp);
            const int64_t ntri = (int64_t)kp * (kp + 1) / 2;
            printf("%s[%d, %d, %d, %d, %lld, %lld]", precision || kp > 16 ? ", " : "", precision, kp, (int)p.g_in_lds,
                   p.batch, (long long)p.lds_bytes, (long long)p.slab_elems);
            f.i64(precision), f.i64(kp), f.i64(p.g_in_lds), f.i64(p.batch), f.i64(p.lds_bytes), f.i64(p.slab_elems);
            batch_ok &= 1 <= p.batch && p.batch <= GENERIC_MAX_BATCH;
            lds_ok &= p.lds_bytes + generic_static_lds_bytes(f64) <= GENERIC_LDS_LIMIT;
            // the staged rows start at the triangle's even-rounded end (16-byte aligned in fp64, 8-byte in fp32)
            const int64_t off = p.g_in_lds ? generic_tri_elems(kp) : 0;
            tri_ok &= off % 2 == 0 && off >= (p.g_in_lds ? ntri : 0) && off <= ntri + 1;
            stage_ok &= p.lds_bytes == (off + (int64_t)p.batch * kp) * elem;
            mono_ok &= !(on_slab && p.g_in_lds);
            on_slab |= !p.g_in_lds;
            slab_ok &= p.slab_elems == (p.g_in_lds ? 0 : ntri + 1);
        }
        mono_ok &= on_slab;   // kp = 1024 cannot hold its triangle in LDS in either precision
    }
    ck.add("batch_1_to_64", batch_ok);
    ck.add("static_plus_dynamic_lds_within_160k", lds_ok);
    ck.add("triangle_offset_even", tri_ok);
    ck.add("lds_bytes_are_triangle_plus_batch", stage_ok);
    ck.add("slab_once_then_always", mono_ok);
    ck.add("slab_elems_triangle_plus_one_or_zero", slab_ok);
    ck.add("static_lds_4112_and_16912", generic_static_lds_bytes(false) == 4112 && generic_static_lds_bytes(true) == 16912);
    printf("], \"invariants\": {");
    for (size_t i = 0; i < ck.v.size(); ++i) printf("%s\"%s\": %s", i ? ", " : "", ck.v[i].first, ck.v[i].second ? "true" : "false");
    printf("}, \"digest\": \"%016llx\"}\n", (unsigned long long)f.h);
}

}  // namespace

int main() {
    for (const Case& c : cases()) run(c);
    run_generic_plan();
    return 0;
}
