// Fused top-N recommendation from the resident factors (als_recommend): score, compare, drop. The dense users x
// movies matrix of als_predict is never written anywhere.
//
// Score of (query user u, candidate position c) = als_predict's cell: the Java-float dot of U[user_rows[u]] and
// M[movie_rows[c]], computed tile by tile by als_score_tile.h (shared with als_rank.hip).
// Order (total): the higher score first, compared as floats (-0 == +0), equal scores by the smaller position c. The
// result therefore does not depend on tiles, segments or the order in which lanes insert.
//
// als_similar is the same sweep under the compile-time policy SIM: both row lists index one
// table, a cell is scaled by the inverse norms of its two rows (cosine), and the only exclusion is the query's own slot.
#include <climits>
#include <cmath>
#include <type_traits>

#include "als_internal.h"
#include "als_score_tile.h"

namespace cfk {
namespace {

constexpr int TU = score_tile::TR, TC = score_tile::TC, PITCH = score_tile::PITCH, QCAP = REC_QUEUE;
using score_tile::better;
static_assert(QCAP <= 64 && REC_MAX_TOP_N <= 64, "one queue entry and one list entry per lane of the merging wave");

__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// Orders the LDS accesses of the lanes of one wave: what any lane wrote before is visible to every lane after. The
// hardware completes a wave's LDS operations in program order; the fences and the barrier keep the compiler to it.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave merges nb new entries (lane l < nb holds (bs, bp)) into a sorted list of nl entries in LDS, keeping the
// best n. Rank by count: an entry's slot is the number of entries that come before it, so no entry moves twice and
// the outcome is independent of the order of the new entries. nl and nb are wave-uniform. Every lane has read its
// list entry into a register before any lane stores (wave_lds_sync), so the list is updated in place, and the caller
// may read it right after.
// Returns the new length. With NaN scores (out of contract) ranks may collide; every store stays inside [0, n).
__device__ __forceinline__ int merge_into_list(float* ls, int* lp, int nl, float bs, int bp, int nb, int n, int lane) {
    const bool ha = lane < nl, hb = lane < nb;
    const float as = ha ? ls[lane] : 0.f;
    const int ap = ha ? lp[lane] : 0;
    int ra = lane, rb = 0;
    for (int j = 0; j < nb; ++j) {
        const float qs = lane_f(bs, j);
        const int qp = lane_i(bp, j);
        ra += better(qs, qp, as, ap) ? 1 : 0;
        rb += better(qs, qp, bs, bp) ? 1 : 0;   // strict: not itself
    }
    for (int i = 0; i < nl; ++i) rb += better(lane_f(as, i), lane_i(ap, i), bs, bp) ? 1 : 0;
    wave_lds_sync();   // every lane holds its entry in registers before any lane stores
    if (ha && ra < n) {
        ls[ra] = as;
        lp[ra] = ap;
    }
    if (hb && rb < n) {
        ls[rb] = bs;
        lp[rb] = bp;
    }
    wave_lds_sync();   // the stores of all lanes before whatever a lane reads next
    return min(n, nl + nb);
}

// position c in the ascending range excl[lo, hi)?
__device__ __noinline__ bool excluded(const int32_t* __restrict__ excl, int64_t lo, int64_t hi, int c) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const int v = excl[mid];
        if (v == c) return true;
        if (v < c) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

struct RecArgs {
    const void* U;
    const void* M;
    int kp, k;
    const int64_t* urows;
    int64_t n_users;
    const int64_t* mrows;
    int64_t n_cand;
    int top_n;
    int64_t seg_len;
    const int64_t* excl_ptr;   // NULL: nothing excluded
    const int32_t* excl_idx;
    float* out_score;          // [n_users * gridDim.y][top_n]: the final lists (one segment) or the partial lists
    int32_t* out_pos;
};

// als_similar's sweep: U is the one table (M is not read), urows / mrows are the query and candidate slots of it,
// excl_ptr / excl_idx are not read.
struct SimArgs : RecArgs {
    const float* inv_q;   // [n_users] 1 / |query row|, 0 for a zero row; NULL: the plain dot, no scaling
    const float* inv_c;   // [n_cand] the same per candidate position
    int exclude_self;     // candidate positions that hold the query's own slot are not eligible
};

// Workgroup (blockIdx.x, blockIdx.y) = (user tile, candidate segment). Thread (ty, tx) of the 16 x 16 grid owns the
// cells of users ty + 16 i and candidates tx + 16 j (i, j < 4), scored by score_tile::score.
// SIM (als_similar) differs in three places, each under if constexpr: the table the candidate rows come from, the
// scaling of the 16 cells after score_tile::score, and the survivors' exclusion test.
template <class T, bool SIM>
__global__ __launch_bounds__(256) void als_recommend_kernel(std::conditional_t<SIM, SimArgs, RecArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float rsm[];
    const int n = a.top_n;
    float* su = rsm;                         // [TU][PITCH]
    float* sm = su + TU * PITCH;             // [TC][PITCH]
    float* qs = sm + TC * PITCH;             // [TU][QCAP] survivors waiting for a merge
    int* qp = (int*)(qs + TU * QCAP);
    float* ls = (float*)(qp + TU * QCAP);    // [TU][n] best so far, sorted
    int* lp = (int*)(ls + TU * n);
    float* tau_s = (float*)(lp + TU * n);    // [TU] the list's n-th entry once it is full: what a cell has to beat
    int* tau_p = (int*)(tau_s + TU);
    int* qcnt = tau_p + TU;                  // [TU] insert attempts since the last merge (may exceed QCAP)
    int* lcnt = qcnt + TU;                   // [TU]
    int* over = lcnt + TU;                   // some queue was full: merge, then the losers try again

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;
    const int64_t u0 = (int64_t)blockIdx.x * TU;
    const int64_t seg_begin = (int64_t)blockIdx.y * a.seg_len;
    const int64_t seg_end = min(a.n_cand, seg_begin + a.seg_len);
    const T* U = (const T*)a.U;
    const T* M = SIM ? U : (const T*)a.M;
    const int k = a.k;

    for (int i = tid; i < TU * n; i += 256) {
        ls[i] = -INFINITY;
        lp[i] = -1;
    }
    if (tid < TU) {
        tau_s[tid] = -INFINITY;   // with position INT_MAX: every cell comes before it
        tau_p[tid] = INT_MAX;
        qcnt[tid] = 0;
        lcnt[tid] = 0;
    }
    if (tid == 0) *over = 0;

    // staging (score_tile::score): this thread loads one feature of rows sr + 8 r
    const int sr = tid >> 5;
    const T* urow[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int64_t u = u0 + sr + 8 * r;
        urow[r] = u < a.n_users ? U + a.urows[u] * (int64_t)a.kp : nullptr;
    }
    // exclusion ranges of this thread's 4 users; SIM: their own slots (-1: no candidate holds it) and inverse norms
    int64_t ex_lo[SIM ? 1 : 4], ex_hi[SIM ? 1 : 4], qslot[SIM ? 4 : 1];
    float qinv[SIM ? 4 : 1];
    bool scale = false;
    if constexpr (SIM) {
        scale = a.inv_q != nullptr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t u = u0 + ty + 16 * i;
            qslot[i] = a.exclude_self && u < a.n_users ? a.urows[u] : -1;
            qinv[i] = scale && u < a.n_users ? a.inv_q[u] : 0.f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t u = u0 + ty + 16 * i;
            const bool has = a.excl_ptr != nullptr && u < a.n_users;
            ex_lo[i] = has ? a.excl_ptr[u] : 0;
            ex_hi[i] = has ? a.excl_ptr[u + 1] : 0;
        }
    }

    // merge the queues of this wave's users (wave w: users w, w + 4, ...) into their lists
    auto flush = [&]() {
        for (int u = wave; u < TU; u += 4) {
            const int nq = __builtin_amdgcn_readfirstlane(min(qcnt[u], QCAP));
            if (nq == 0) continue;
            const int nl = __builtin_amdgcn_readfirstlane(lcnt[u]);
            const float bs = lane < nq ? qs[u * QCAP + lane] : 0.f;
            const int bp = lane < nq ? qp[u * QCAP + lane] : 0;
            const int nl2 = merge_into_list(ls + u * n, lp + u * n, nl, bs, bp, nq, n, lane);
            if (lane == 0) {   // after the merge's stores (fenced there)
                lcnt[u] = nl2;
                qcnt[u] = 0;
                if (nl2 == n) {
                    tau_s[u] = ls[u * n + n - 1];
                    tau_p[u] = lp[u * n + n - 1];
                }
            }
        }
    };

    for (int64_t c0 = seg_begin; c0 < seg_end; c0 += TC) {
        const T* mrow[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t c = c0 + sr + 8 * r;
            mrow[r] = c < seg_end ? M + a.mrows[c] * (int64_t)a.kp : nullptr;
        }
        float acc[4][4];
        if constexpr (SIM) {
            // the tile's 4 inverse norms are asked for before the dots and used after them
            float cinv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t c = c0 + tx + 16 * j;
                cinv[j] = scale && c < seg_end ? a.inv_c[c] : 0.f;
            }
            score_tile::score(acc, su, sm, urow, mrow, k, c0 == seg_begin, tid);
            if (scale) {   // (cell * inv(q)) * inv(c): two rounded products
#pragma clang fp contract(off)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = (acc[i][j] * qinv[i]) * cinv[j];
            }
        } else {
            score_tile::score(acc, su, sm, urow, mrow, k, c0 == seg_begin, tid);
        }

        // selection: a cell that does not come before its user's threshold is dropped here; the exclusion list (SIM:
        // the candidate's slot) is consulted only for the survivors, and excluded ones never reach the queue (so they
        // cannot raise the threshold)
        unsigned pend = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ul = ty + 16 * i;
            if (u0 + ul >= a.n_users) continue;
            const float ts = tau_s[ul];
            const int tp = tau_p[ul];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t c = c0 + tx + 16 * j;
                if constexpr (SIM) {
                    if (c < seg_end && better(acc[i][j], (int)c, ts, tp) && a.mrows[c] != qslot[i])
                        pend |= 1u << (i * 4 + j);
                } else {
                    if (c < seg_end && better(acc[i][j], (int)c, ts, tp) &&
                        !(ex_hi[i] > ex_lo[i] && excluded(a.excl_idx, ex_lo[i], ex_hi[i], (int)c)))
                        pend |= 1u << (i * 4 + j);
                }
            }
        }
        for (;;) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (((pend >> (4 * i)) & 15u) == 0) continue;
                const int ul = ty + 16 * i;
                const float ts = tau_s[ul];
                const int tp = tau_p[ul];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned bit = 1u << (i * 4 + j);
                    if (!(pend & bit)) continue;
                    const int c = (int)(c0 + tx + 16 * j);
                    if (!better(acc[i][j], c, ts, tp)) {   // a merge since the first look raised the threshold
                        pend &= ~bit;
                        continue;
                    }
                    const int slot = atomicAdd(&qcnt[ul], 1);
                    if (slot < QCAP) {
                        qs[ul * QCAP + slot] = acc[i][j];
                        qp[ul * QCAP + slot] = c;
                        pend &= ~bit;
                    } else {
                        *over = 1;
                    }
                }
            }
            __syncthreads();
            if (*over == 0) break;   // uniform: every thread reads it between the same two barriers
            flush();
            __syncthreads();
            if (tid == 0) *over = 0;
            __syncthreads();
        }
    }

    __syncthreads();
    flush();
    __syncthreads();
    // sorted list, padded with (-1, -inf) as initialised
    const int64_t orow_stride = gridDim.y;
    for (int i = tid; i < TU * n; i += 256) {
        const int ul = i / n, j = i - ul * n;
        const int64_t u = u0 + ul;
        if (u >= a.n_users) continue;
        const int64_t o = (u * orow_stride + blockIdx.y) * n + j;
        const bool have = j < lcnt[ul];
        a.out_score[o] = have ? ls[i] : -INFINITY;
        a.out_pos[o] = have ? lp[i] : -1;
    }
}

// S partial lists per user -> the final list: one wave per user merges them one after the other under the same order.
// A segment whose best entry does not come before the current n-th best is skipped whole.
__global__ __launch_bounds__(256) void als_recommend_merge(const float* __restrict__ part_s,
                                                           const int32_t* __restrict__ part_p, int64_t n_users,
                                                           int64_t S, int n, float* __restrict__ out_score,
                                                           int32_t* __restrict__ out_pos) {
    __shared__ float ls[4][64];
    __shared__ int lp[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= n_users) return;   // whole waves leave; no workgroup barrier below
    ls[wave][lane] = -INFINITY;
    lp[wave][lane] = -1;
    int nl = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t base = (u * S + s) * n;
        const float bs = lane < n ? part_s[base + lane] : -INFINITY;
        const int bp = lane < n ? part_p[base + lane] : -1;
        const int nb = __builtin_amdgcn_readfirstlane(__popcll(__ballot(bp >= 0)));   // the padding is a suffix
        if (nb == 0) continue;
        if (nl == n) {
            const float ts = lane_f(ls[wave][n - 1], 0);
            const int tp = lane_i(lp[wave][n - 1], 0);
            if (!better(lane_f(bs, 0), lane_i(bp, 0), ts, tp)) continue;
        }
        nl = merge_into_list(ls[wave], lp[wave], nl, bs, bp, nb, n, lane);
    }
    if (lane < n) {
        out_score[u * n + lane] = lane < nl ? ls[wave][lane] : -INFINITY;
        out_pos[u * n + lane] = lane < nl ? lp[wave][lane] : -1;
    }
}

// Both calls' launch: the scoring kernel over (user tiles, segments), then the merge kernel when there are several
// segments. A: RecArgs or SimArgs, filled by the caller up to the outputs.
template <bool SIM, class A>
hipError_t launch_sweep(int precision, A a, int64_t n_users, int64_t n_cand, int top_n, const RecommendPlan& plan,
                        float* part_score, int32_t* part_pos, float* out_score, int32_t* out_pos, hipStream_t s) {
    if (n_users <= 0 || n_cand <= 0) return hipSuccess;
    if (top_n < 1 || top_n > REC_MAX_TOP_N || n_cand > INT32_MAX || plan.user_tiles > INT32_MAX ||
        plan.segments < 1 || plan.segments > REC_MAX_SEGMENTS || plan.lds_bytes > REC_LDS_LIMIT)
        return hipErrorInvalidValue;
    const bool split = plan.segments > 1;
    a.n_users = n_users;
    a.n_cand = n_cand;
    a.top_n = top_n;
    a.seg_len = plan.seg_len;
    a.out_score = split ? part_score : out_score;
    a.out_pos = split ? part_pos : out_pos;
    const dim3 grid((unsigned)plan.user_tiles, (unsigned)plan.segments);
    const void* fn = precision == 0 ? (const void*)als_recommend_kernel<float, SIM>
                                    : (const void*)als_recommend_kernel<double, SIM>;
    // top_n = 64 needs more than the 64 KiB a kernel gets by default. Every call sets the same bound (the largest any
    // top_n needs), so engines of several devices and host threads cannot lower it under one another's launch.
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)recommend_lds_bytes(REC_MAX_TOP_N));
    if (e != hipSuccess) return e;
    if (precision == 0) als_recommend_kernel<float, SIM><<<grid, 256, (size_t)plan.lds_bytes, s>>>(a);
    else als_recommend_kernel<double, SIM><<<grid, 256, (size_t)plan.lds_bytes, s>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess || !split) return e;
    als_recommend_merge<<<(unsigned)((n_users + 3) / 4), 256, 0, s>>>(part_score, part_pos, n_users, plan.segments,
                                                                     top_n, out_score, out_pos);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_recommend(int precision, const void* U, const void* M, int kp, int k, const int64_t* urows,
                            int64_t n_users, const int64_t* mrows, int64_t n_cand, int top_n,
                            const RecommendPlan& plan, const int64_t* excl_ptr, const int32_t* excl_idx,
                            float* part_score, int32_t* part_pos, float* out_score, int32_t* out_pos,
                            hipStream_t s) {
    RecArgs a{};
    a.U = U;
    a.M = M;
    a.kp = kp;
    a.k = k;
    a.urows = urows;
    a.mrows = mrows;
    a.excl_ptr = excl_ptr;
    a.excl_idx = excl_idx;
    return launch_sweep<false>(precision, a, n_users, n_cand, top_n, plan, part_score, part_pos, out_score, out_pos, s);
}

hipError_t launch_similar_sweep(int precision, const void* table, int kp, int k, const int64_t* qrows, int64_t n_queries,
                                const int64_t* crows, int64_t n_cand, int top_n, const RecommendPlan& plan,
                                const float* inv_q, const float* inv_c, bool exclude_self, float* part_score,
                                int32_t* part_pos, float* out_score, int32_t* out_pos, hipStream_t s) {
    if ((inv_q == nullptr) != (inv_c == nullptr)) return hipErrorInvalidValue;
    SimArgs a{};
    a.U = table;
    a.M = table;
    a.kp = kp;
    a.k = k;
    a.urows = qrows;
    a.mrows = crows;
    a.inv_q = inv_q;
    a.inv_c = inv_c;
    a.exclude_self = exclude_self ? 1 : 0;
    return launch_sweep<true>(precision, a, n_queries, n_cand, top_n, plan, part_score, part_pos, out_score, out_pos, s);
}

}  // namespace cfk
