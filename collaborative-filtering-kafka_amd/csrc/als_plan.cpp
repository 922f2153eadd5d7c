// als_plan.cpp -- the work plan of a block (als_plan.h): how its long rows are split, and the task lists of its
// launches. Host arithmetic only: no HIP, no environment.
#include "als_plan.h"

#include <algorithm>

namespace cfk {

namespace {

// Chunk length (entries, multiple of 4) above which a row is split into PARTIAL tasks + a REDUCE task.
// Aim for enough wave-tasks to fill 256 CUs several times over while keeping partial traffic small.
int64_t chunk_entries(const PlanKnobs& kn, int64_t nnz_padded) {
    constexpr int64_t B = BLOCK_ENTRIES;
    if (kn.chunk >= 1) return (kn.chunk + B - 1) / B * B;
    // nnz/4096 (24.5k entries at Netflix shape; kbench: movie half + REDUCE 3.38 -> 3.19 ms against the
    // former nnz/24576 <= 8192, fewer 11-KB partial slots and REDUCE solves), still nnz-proportional so a
    // G-way shard keeps enough tasks for load balance
    int64_t c = nnz_padded / 4096;
    c = std::max<int64_t>(c, 1024);
    c = std::min<int64_t>(c, 32768);
    return (c + B - 1) / B * B;
}

// Bytes of the pre-split opposite table (sentinel row included).
int64_t presplit_table_bytes(const BlockShape& s) { return (s.n_opp_rows + 1) * (int64_t)presplit_row_bytes(s.kp); }

// The pre-split Gram exists for the split path at KP = 64 and 128, and its gather forms 32-bit byte offsets
// row * presplit_row_bytes with a 24-bit multiply: both the row (< 2^24) and the offset (< 2^32) must fit, also when
// a knob forces the path.
bool presplit_possible(const BlockShape& s) {
    if (s.path != Path::MFMA_SPLIT || (s.kp != 64 && s.kp != 128)) return false;
    return s.n_opp_rows + 1 < (1 << 24) && presplit_table_bytes(s) <= (int64_t)UINT32_MAX;
}

// Interleaved split rows: on a half whose opposite table outgrows the L2s but fits the Infinity
// Cache (the 123 / 246 MB user table of the Netflix-shape movie half at k = 64 / 128, the 256 MB item table of the
// power-law user half), a row longer than the returned length (entries) is split into
// nc = ceil(d / length) chunks of INTERLEAVED blocks -- chunk c = blocks c, c + nc, c + 2 nc, ... of the row -- so
// that every chunk covers the row's whole range of opposite slots. With the chunks dispatched together (longest
// first) the waves of an XCD then walk the opposite table in step and find its rows in their L2. Such a half gathers
// the pre-split table (the fp16 Gram). 0: contiguous chunks at chunk_entries() (the other halves).
int64_t interleave_chunk(const PlanKnobs& kn, const BlockShape& s, const std::vector<int64_t>& deg) {
    const int64_t sb = presplit_table_bytes(s);
    if (kn.interleave == 0 || !presplit_possible(s)) return 0;
    // auto: a table the L2s cannot hold (> 32 MB) that the 256 MiB Infinity Cache still holds; beyond the IC (configs[4]'s
    // 2.56 GB user table) the contiguous chunks read the long rows' near-dense user ranges in order and win (item half
    // of the power-law shard: 8.87 vs 14.6 ms interleaved, profiles/r06a)
    if (kn.interleave < 0 && (sb <= (32ll << 20) || sb > (256ll << 20))) return 0;
    auto long_work = [&](int64_t t) {   // entries in rows longer than t
        int64_t w = 0;
        for (int64_t d : deg) w += d > t ? d : 0;
        return w;
    };
    // the walk in step needs many chunks in flight: resident waves of the pre-split launch (4 per SIMD at KP = 64, 1 at
    // KP = 128). Chunk length (kbench, Netflix shape, movie half + its REDUCE, profiles/r06a): k = 64, whole data:
    // 8,192 / 10,240 / 12,288 / 16,384 / 24,576 entries 2.07 / 2.04 / 2.06 / 2.16 / 2.29 ms (contiguous chunks: 2.98);
    // one rank's shard of G = 2 / 4 / 8 (fewer chunks than twice the resident waves): 1.52 / 0.95 / 0.66 ms at the
    // best length vs 1.58 / 0.90 / 0.47 contiguous -- so k = 64 interleaves only with >= 1.5 x the resident waves of
    // chunks. k = 128 (whole data 4,096 / 8,192 / 16,384: 5.76 / 5.32 / 5.06 ms, contiguous 6.67; shards of G = 2 / 4
    // / 8 at 8,192: 4.92 / 2.55 / 1.37 vs 5.25 / 2.77 / 1.50) always. Round 6 (profiles/r06c/xcd2_*.log, movie half +
    // REDUCE): whole data 16,384 / 8,192 / 4,096: 5.07 / 5.26 / 5.71 ms; shards of G = 2 / 4 / 8 at 4,096: 4.17 / 2.36 /
    // ~1.40 ms vs 4.98 / 2.57 / 1.39 at 8,192 (2,048: 4.13 / 2.29 / 1.40; its REDUCE launch doubles) -- so 16,384 when
    // the long rows hold over ~4 chunks of it per resident wave (the whole Netflix shape), else 4,096.
    const int64_t conc = (int64_t)std::max(1, s.cu_count) * (s.kp == 128 ? 4 : 16);
    int64_t len;
    if (s.kp == 64) {
        len = 10240;
        // the concurrency rule holds for the 123 MB user table of a Netflix shard; the 256 MB item table of the
        // power-law shard's user half interleaves whatever its long-row work (9.43 -> 7.38 ms, profiles/r06a; the rule
        // alone had turned it off again: 9.47-9.57 ms, profiles/r06c/ranges_bench_ab)
        if (kn.interleave < 0 && sb <= (128ll << 20) && long_work(len) < len * conc * 3 / 2) return 0;
    } else {
        len = long_work(16384) >= 16384 * 4 * conc ? 16384 : 4096;
    }
    if (kn.ilv_chunk > 0) len = kn.ilv_chunk;
    return (len + BLOCK_ENTRIES - 1) / BLOCK_ENTRIES * BLOCK_ENTRIES;
}

constexpr int XR = 8;   // XCD ranges of the opposite table

bool longer(const Task& a, const Task& b) { return a.nsteps > b.nsteps; }

}  // namespace

BlockLayout plan_layout(const PlanKnobs& kn, const BlockShape& s, const std::vector<int64_t>& deg) {
    BlockLayout L;
    int64_t nnz_padded = 0;   // every row starts on a 32-entry block
    for (int64_t d : deg) nnz_padded += (d + BLOCK_ENTRIES - 1) / BLOCK_ENTRIES * BLOCK_ENTRIES;
    L.chunk = chunk_entries(kn, nnz_padded);
    // the generic path's workgroup takes a whole row of any length: no split rows
    const int64_t chunk = s.path == Path::GENERIC ? INT64_MAX : L.chunk;
    // (no longer than the contiguous chunk: a small block keeps enough tasks for load balance)
    L.ilv = std::min(interleave_chunk(kn, s, deg), chunk);
    // XCD ranges (ALS_XCD_RANGES): a long row's blocks are first grouped by the opposite slot of their first entry
    // into X = 8 ranges of the opposite table (a row's entries ascend by slot, so each range is a run of its blocks),
    // then each range's blocks are interleaved into chunks as below. Chunk tasks of range x all run on one XCD (the
    // task order below), so that XCD's L2 serves 1/8 of the table instead of every XCD fetching all of it.
    // Measured (profiles/r06c/ranges_*.log): the k = 64 Netflix-shape movie half (123 MB user table, one launch) 2.00
    // -> 1.80 ms, iteration 4.73 -> 4.60 ms; the k = 128 movie half (246 MB) and the power-law shard's chunked item-table
    // half (256 MB) a little slower, shards of G = 2 / 4 slower than their contiguous plan -- so auto = KP = 64 with an
    // opposite table within 128 MiB (each XCD's range within 16 MiB).
    const int64_t sb = presplit_table_bytes(s);
    L.ranges = L.ilv > 0 && s.n_opp_rows > 0 &&
               (kn.xcd_ranges > 0 || (kn.xcd_ranges < 0 && s.kp == 64 && sb <= (128ll << 20)));
    // Pre-split opposite table (scaled two-term fp16, cfk::launch_presplit_prepare, once per half) for the MFMA Gram: 4 KP
    // bytes per row (the fp32 row's size), 3 MFMAs per tile instead of the on-the-fly bf16 split's 6, no split VALU
    // (the rows reach LDS by DMA and the MFMA operands come back with transposed reads). Chosen where the Gram is
    // MFMA-bound: always at KP = 128, and at KP = 64 for a cache-resident opposite table (<= 8 MB: the 17,770-row
    // movie table of the user half, 2.99 vs 4.37 ms). The KP = 64 movie half gathers the 123 MB user table at the
    // Infinity-Cache ceiling either way, and the split pass over that table would cost more than it saves (3.08 vs
    // 3.01 ms; kbench). ALS_PRESPLIT=0/1 forces it off/on.
    L.presplit = s.kp == 128 || sb <= (8ll << 20) || L.ilv > 0;
    if (kn.presplit >= 0) L.presplit = kn.presplit == 1;
    L.presplit = L.presplit && presplit_possible(s);
    return L;
}

BlockPlan plan_build(const PlanKnobs& kn, const BlockShape& s, const BlockLayout& L, const std::vector<int64_t>& deg,
                     const std::vector<int64_t>& begin, const std::vector<int32_t>& bfirst) {
    BlockPlan P;
    const int64_t n_rows = (int64_t)deg.size(), n_opp_rows = s.n_opp_rows;
    const int64_t nnz_padded = begin[n_rows];
    // the generic path's workgroup takes a whole row of any length: no split rows
    const int64_t chunk = s.path == Path::GENERIC ? INT64_MAX : L.chunk;
    const int64_t ilv = L.ilv;
    const bool ranges = L.ranges;
    std::vector<Task>& tasks = P.tasks;     // whole rows and contiguous chunks; the main launch in the end
    std::vector<Task>& reduce = P.reduce;
    std::vector<Task> stasks;               // interleaved chunk tasks, until they join `tasks`
    int64_t& slots = P.slots;
    // Interleaved split rows: the long rows' blocks are permuted chunk-major (chunk c = blocks c, c + nc, ... of the
    // row, in order), each chunk one PARTIAL task of whole blocks (the row's last, padded block is the last block of
    // its chunk, so nent counts exactly the chunk's real entries), one REDUCE per row.
    std::vector<int32_t>& perm = P.perm;
    std::vector<int8_t> srange;   // XCD range of each interleaved chunk task (ranges only)
    if (ilv > 0) {
        constexpr int64_t BE = BLOCK_ENTRIES;
        std::vector<int64_t> piece[XR];
        for (int64_t i = 0; i < n_rows; ++i) {
            const int64_t d = deg[i];
            if (d <= ilv) continue;
            if (perm.empty()) {
                perm.resize((size_t)(nnz_padded / BE));
                for (size_t q = 0; q < perm.size(); ++q) perm[q] = (int32_t)q;
            }
            ++P.ilv_rows;
            const int64_t nb = (d + BE - 1) / BE, b0 = begin[i] / BE;
            for (auto& v : piece) v.clear();
            for (int64_t q = 0; q < nb; ++q) {
                const int x = ranges ? (int)std::min<int64_t>(XR - 1, (int64_t)bfirst[(size_t)(b0 + q)] * XR / n_opp_rows)
                                     : 0;
                piece[x].push_back(q);
            }
            Task t{};
            t.row = (int32_t)i;
            t.ndeg = (int32_t)d;
            t.kind = TASK_PARTIAL;
            const int64_t first = slots;
            int64_t pos = 0;
            for (int x = 0; x < XR; ++x) {
                const std::vector<int64_t>& pb = piece[x];
                if (pb.empty()) continue;
                const int64_t np = (int64_t)pb.size();
                const bool has_last = pb.back() == nb - 1;   // the row's padded block: last of its chunk below
                const int64_t pent = BE * np - (has_last ? BE * nb - d : 0);
                const int64_t nc = (pent + ilv - 1) / ilv;
                for (int64_t c = 0; c < nc; ++c) {
                    const int64_t p0 = pos;
                    bool last = false;
                    for (int64_t y = c; y < np; y += nc) {
                        perm[(size_t)(b0 + pos++)] = (int32_t)(b0 + pb[(size_t)y]);
                        last = pb[(size_t)y] == nb - 1;
                    }
                    const int64_t cnt = pos - p0;
                    const int64_t nent = last ? BE * (cnt - 1) + (d - BE * (nb - 1)) : BE * cnt;
                    Task p = t;
                    p.begin = begin[i] + BE * p0;
                    p.nent = (int32_t)nent;
                    p.nsteps = (int32_t)((nent + 3) / 4);
                    p.slot = (int32_t)slots++;
                    stasks.push_back(p);
                    srange.push_back((int8_t)x);
                }
            }
            Task r = t;
            r.begin = 0;
            r.slot = (int32_t)first;
            r.nsteps = (int32_t)(slots - first);
            r.kind = TASK_REDUCE;
            reduce.push_back(r);
        }
    }
    P.ilv_tasks = (int64_t)stasks.size();
    for (int64_t i = 0; i < n_rows; ++i) {
        if (ilv > 0 && deg[i] > ilv) continue;   // interleaved above
        const int64_t d = deg[i];
        Task t{};
        t.row = (int32_t)i;
        t.ndeg = (int32_t)d;
        if (d <= chunk) {
            t.begin = begin[i];
            t.nsteps = (int32_t)((d + 3) / 4);
            t.nent = (int32_t)d;
            t.slot = -1;
            t.kind = TASK_FULL;
            tasks.push_back(t);
        } else {
            const int64_t first = slots;
            for (int64_t o = 0; o < d; o += chunk) {
                Task p = t;
                p.begin = begin[i] + o;
                p.nsteps = (int32_t)((std::min(chunk, d - o) + 3) / 4);
                p.nent = (int32_t)std::min(chunk, d - o);
                p.slot = (int32_t)slots++;
                p.kind = TASK_PARTIAL;
                tasks.push_back(p);
            }
            Task r = t;
            r.begin = 0;
            r.slot = (int32_t)first;
            r.nsteps = (int32_t)(slots - first);
            r.kind = TASK_REDUCE;
            reduce.push_back(r);
        }
    }
    // Short rows in entry space (split-bf16 path): rows of <= 3 blocks at KP = 128, 1 block at KP = 64 solve the
    // (padded entries)^2 system of als_solve_dual instead of the KP x KP one. Only rows with n <= k entries: then
    // Y Y^T + lambda n I_n has the nonzero spectrum of Y^T Y + lambda n I_k plus nothing smaller, so the same
    // conditioning; with n > k the n x n system would carry n - k eigenvalues lambda n only (singular at
    // lambda = 0 where the reference's k x k system is not). ALS_DUAL=0 turns it off.
    P.sq_all = stasks;
    P.sq_all.insert(P.sq_all.end(), tasks.begin(), tasks.end());
    std::vector<Task>* dual = P.dual;
    {
        const int max_cd = s.path != Path::MFMA_SPLIT ? 0 : s.kp == 128 ? 6 : s.kp == 64 ? 2 : 0;
        const bool on = max_cd > 0 && kn.dual;
        if (on) {
            std::vector<Task> keep;
            for (const Task& t : tasks) {
                const int cd = 2 * ((t.nent + BLOCK_ENTRIES - 1) / BLOCK_ENTRIES);
                if (t.kind == TASK_FULL && t.ndeg > 0 && t.ndeg <= s.k && cd <= max_cd)
                    dual[cd / 2 - 1].push_back(t);
                else
                    keep.push_back(t);
            }
            tasks.swap(keep);
        }
    }
    if (slots > INT32_MAX || tasks.size() > (size_t)INT32_MAX) {
        P.error = "too many tasks / partial slots";
        return P;
    }
    // Longest tasks first (LPT): the grid drains with a short tail.
    std::stable_sort(tasks.begin(), tasks.end(), longer);
#ifdef CFK_DEBUG_KNOBS
    // ALS_TASK_ORDER=random / stagger[:W] (measurement knobs, debug build only): a seeded shuffle of the main launch's
    // tasks, or LPT windows alternating between its longer and shorter half
    if (kn.task_order == PlanKnobs::STAGGER) {
        // windows of W tasks (W = stagger:<W>, default 1024 = one 4-wave workgroup per CU) alternate between the
        // longer and the shorter half of the LPT list: co-resident waves of a CU run tasks of different lengths
        const size_t W = (size_t)kn.stagger_window;
        const size_t h = (tasks.size() + 1) / 2;
        std::vector<Task> out;
        out.reserve(tasks.size());
        size_t ia = 0, ib = h;
        while (ia < h || ib < tasks.size()) {
            for (size_t q = 0; q < W && ia < h; ++q) out.push_back(tasks[ia++]);
            for (size_t q = 0; q < W && ib < tasks.size(); ++q) out.push_back(tasks[ib++]);
        }
        tasks.swap(out);
    }
    if (kn.task_order == PlanKnobs::RANDOM) {
        uint64_t x = 0x9e3779b97f4a7c15ull;
        for (size_t i = tasks.size(); i > 1; --i) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            std::swap(tasks[i - 1], tasks[(size_t)(x % i)]);
        }
    }
#endif
    std::stable_sort(reduce.begin(), reduce.end(), longer);
    for (int c = 0; c < 3; ++c) std::stable_sort(dual[c].begin(), dual[c].end(), longer);

    // the interleaved chunks join the plain tasks, longest first
    if (!stasks.empty() && ranges) {
        // XCD ranges: workgroup w runs on the XCD of w % 8 (round-robin placement; speed only, never correctness), so
        // the workgroups at positions w = 8 j + x take range x's chunk tasks (queue x). The plain (whole-row) tasks have
        // no range: each goes, longest first, to the queue of least work among those still short of an equal share of
        // the task count, so the queues stay aligned to the round-robin. Every queue is longest first.
        std::vector<Task> q[XR];
        int64_t work[XR] = {};
        for (size_t t = 0; t < stasks.size(); ++t) {
            q[srange[t]].push_back(stasks[t]);
            work[srange[t]] += stasks[t].nsteps;
        }
        const int64_t total = (int64_t)(stasks.size() + tasks.size());
        const int64_t wgs = (total + 3) / 4;
        for (const Task& t : tasks) {   // already longest first
            int best = -1;
            for (int x = 0; x < XR; ++x) {
                const int64_t cap = 4 * ((wgs - x + XR - 1) / XR);   // tasks of the workgroups at w = x mod 8
                if ((int64_t)q[x].size() < cap && (best < 0 || work[x] < work[best])) best = x;
            }
            if (best < 0) best = (int)(std::min_element(work, work + XR) - work);
            q[best].push_back(t);
            work[best] += t.nsteps;
        }
        std::vector<Task> out;
        out.reserve((size_t)total);
        for (int x = 0; x < XR; ++x) std::stable_sort(q[x].begin(), q[x].end(), longer);
        for (size_t j = 0;; j += 4) {
            bool any = false;
            for (int x = 0; x < XR; ++x)
                for (size_t u = j; u < j + 4 && u < q[x].size(); ++u) {
                    out.push_back(q[x][u]);
                    any = true;
                }
            if (!any) break;
        }
        tasks.swap(out);
    } else if (!stasks.empty()) {
        tasks.insert(tasks.begin(), stasks.begin(), stasks.end());
        std::stable_sort(tasks.begin(), tasks.end(), longer);
    }
    return P;
}

void partition_by_chunk(const std::vector<Task>& in, int n_chunks, const int64_t* row_bounds, std::vector<Task>& out,
                        std::vector<int32_t>& off) {
    auto chunk_of = [&](int32_t row) {
        return (int)(std::upper_bound(row_bounds, row_bounds + n_chunks + 1, (int64_t)row) - row_bounds) - 1;
    };
    std::vector<std::vector<Task>> per(n_chunks);
    for (const Task& t : in) per[chunk_of(t.row)].push_back(t);
    off.assign(n_chunks + 1, 0);
    out.clear();
    for (int c = 0; c < n_chunks; ++c) {
        out.insert(out.end(), per[c].begin(), per[c].end());
        off[c + 1] = (int32_t)out.size();
    }
}

// The Gram stays in LDS while the packed triangle and GENERIC_MIN_LDS_BATCH staged rows fit beside the kernel's static
// vectors; then the batch is whatever still fits, at most GENERIC_MAX_BATCH. Beyond that the triangle goes to a
// per-workgroup global slab and the staged rows get GENERIC_SLAB_STAGE_BYTES.
GenericPlan generic_plan(int precision, int kp) {
    GenericPlan p{};
    const bool f64 = precision != 0;
    const int64_t elem = f64 ? 8 : 4;
    const int64_t tri_b = generic_tri_elems(kp) * elem;
    const int64_t avail = GENERIC_LDS_LIMIT - generic_static_lds_bytes(f64);
    const int64_t row_b = (int64_t)kp * elem;
    if (tri_b + GENERIC_MIN_LDS_BATCH * row_b <= avail) {
        p.g_in_lds = true;
        p.batch = (int)std::min<int64_t>(GENERIC_MAX_BATCH, (avail - tri_b) / row_b);
        p.lds_bytes = tri_b + p.batch * row_b;
        p.slab_elems = 0;
    } else {
        p.g_in_lds = false;
        p.batch = (int)std::max<int64_t>(1, std::min<int64_t>(GENERIC_MAX_BATCH, GENERIC_SLAB_STAGE_BYTES / row_b));
        p.lds_bytes = p.batch * row_b;
        p.slab_elems = (int64_t)kp * (kp + 1) / 2 + 1;
    }
    return p;
}

RecommendPlan recommend_plan(int64_t n_users, int64_t n_cand, int top_n, int kp, int cu_count) {
    (void)kp;
    RecommendPlan p;
    n_users = std::max<int64_t>(n_users, 0);
    n_cand = std::max<int64_t>(n_cand, 0);
    top_n = std::min(std::max(top_n, 1), REC_MAX_TOP_N);
    const int64_t cus = std::max(1, cu_count);
    p.user_tiles = (n_users + REC_USER_TILE - 1) / REC_USER_TILE;
    const int64_t cand_tiles = std::max<int64_t>(1, (n_cand + REC_CAND_TILE - 1) / REC_CAND_TILE);
    int64_t S = 1;
    if (p.user_tiles < cus) {
        const int64_t ut = std::max<int64_t>(1, p.user_tiles);
        S = std::min({cand_tiles, (4 * cus + ut - 1) / ut, REC_MAX_SEGMENTS});
    }
    const int64_t seg_tiles = (cand_tiles + S - 1) / S;
    p.segments = (cand_tiles + seg_tiles - 1) / seg_tiles;   // no empty segment
    p.seg_len = seg_tiles * REC_CAND_TILE;
    p.lds_bytes = recommend_lds_bytes(top_n);
    p.partial_rows = p.segments > 1 ? n_users * p.segments : 0;
    auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
    int64_t off = 0;
    p.off_urows = off, off += align(n_users * 8);
    p.off_mrows = off, off += align(n_cand * 8);
    p.off_idx = off, off += align(n_users * top_n * 4);
    p.off_score = off, off += align(n_users * top_n * 4);
    p.off_part_score = off, off += align(p.partial_rows * top_n * 4);
    p.off_part_pos = off, off += align(p.partial_rows * top_n * 4);
    p.workspace_bytes = off;
    return p;
}

SimilarPlan similar_plan(int64_t n_queries, int64_t n_cand, int top_n, int kp, int cu_count) {
    SimilarPlan p;
    p.sweep = recommend_plan(n_queries, n_cand, top_n, kp, cu_count);
    auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
    int64_t off = p.sweep.workspace_bytes;
    p.off_inv_q = off, off += align(std::max<int64_t>(n_queries, 0) * 4);
    p.off_inv_c = off, off += align(std::max<int64_t>(n_cand, 0) * 4);
    p.workspace_bytes = off;
    return p;
}

RankPlan rank_plan(int64_t n_targets, int64_t n_cand, int kp, int cu_count) {
    (void)kp;
    RankPlan p;
    n_targets = std::max<int64_t>(n_targets, 0);
    n_cand = std::max<int64_t>(n_cand, 0);
    const int64_t cus = std::max(1, cu_count);
    p.tgt_tiles = (n_targets + RANK_TGT_TILE - 1) / RANK_TGT_TILE;
    const int64_t cand_tiles = std::max<int64_t>(1, (n_cand + RANK_CAND_TILE - 1) / RANK_CAND_TILE);
    int64_t S = 1;
    if (p.tgt_tiles < cus) {
        const int64_t tt = std::max<int64_t>(1, p.tgt_tiles);
        S = std::min({cand_tiles, (RANK_WG_PER_CU * cus + tt - 1) / tt, RANK_MAX_SEGMENTS});
    }
    const int64_t seg_tiles = (cand_tiles + S - 1) / S;
    p.segments = (cand_tiles + seg_tiles - 1) / seg_tiles;   // no empty segment
    p.seg_len = seg_tiles * RANK_CAND_TILE;
    p.lds_bytes = rank_lds_bytes();
    auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
    int64_t off = 0;
    p.off_trow = off, off += align(n_targets * 8);
    p.off_tpos = off, off += align(n_targets * 4);
    p.off_tuser = off, off += align(n_targets * 4);
    p.off_score = off, off += align(n_targets * 4);
    p.off_rank = off, off += align(n_targets * 4);
    p.off_mrows = off, off += align(n_cand * 8);
    p.workspace_bytes = off;
    return p;
}

FoldinPlan foldin_plan(int kp, int elem_bytes, int64_t n_queries, int cu_count) {
    FoldinPlan p;
    int batch = FOLDIN_MAX_BATCH;
    while (batch > 4 && foldin_lds_bytes(kp, elem_bytes, batch) > FOLDIN_LDS_LIMIT) batch -= 4;
    p.batch = batch;
    p.lds_bytes = foldin_lds_bytes(kp, elem_bytes, batch);
    const int64_t per_cu =
        std::min<int64_t>(FOLDIN_MAX_WG_PER_CU, std::max<int64_t>(1, FOLDIN_LDS_LIMIT / std::max<int64_t>(1, p.lds_bytes)));
    p.grid = std::max<int64_t>(1, std::min<int64_t>(n_queries, per_cu * std::max(1, cu_count)));
    return p;
}

GramTablePlan gram_table_plan(int kp, int elem_bytes, int64_t n_rows, int cu_count) {
    (void)cu_count;
    GramTablePlan p;
    n_rows = std::max<int64_t>(n_rows, 0);
    const int64_t per = (n_rows + GRAM_TABLE_MAX_SLABS - 1) / GRAM_TABLE_MAX_SLABS;
    p.rows_per_slab =
        std::max<int64_t>(GRAM_TABLE_MIN_SLAB_ROWS, (per + FOLDIN_MAX_BATCH - 1) / FOLDIN_MAX_BATCH * FOLDIN_MAX_BATCH);
    p.slabs = std::max<int64_t>(1, (n_rows + p.rows_per_slab - 1) / p.rows_per_slab);
    p.lds_bytes = gram_table_lds_bytes(kp, elem_bytes);
    p.partial_bytes = p.slabs * foldin_tiles(kp) * 256 * (int64_t)elem_bytes;
    return p;
}

ObjectivePlan objective_plan(int kp, int elem_bytes, int64_t n_queries, int cu_count) {
    (void)elem_bytes;
    ObjectivePlan p;
    p.lds_bytes = objective_lds_bytes(kp);
    p.grid = std::max<int64_t>(1, std::min<int64_t>(n_queries, (int64_t)OBJECTIVE_WG_PER_CU * std::max(1, cu_count)));
    return p;
}

}  // namespace cfk
