// Held-out evaluation from the resident factors (als_rank_targets): the exact score of every (user, target) pair and
// the target's exact rank among the user's candidates, without writing or sorting a users x movies matrix.
//
// Score and order are als_recommend's (als_recommend.hip): the score of (query user u, candidate position c) is
// als_predict's cell -- the Java-float dot of U[user_rows[u]] and M[movie_rows[c]], fp32, product and partial sum rounded
// separately, features 0..k-1 in order, f64 factors narrowed to float first -- and (s, c) comes before (ts, tp) when
// s > ts as floats, or s == ts and c < tp. Under that total order the rank of a target is an integer: the number of
// non-excluded candidates that come before it. Counting replaces "select the best N": no list, no queue, no merge.
//   als_score_pairs   : the T target scores (the thresholds of the sweep, and the held-out RMSE path on their own).
//   als_rank_count    : the hot path. Rows of a tile are target entries; every cell of the candidate sweep adds
//                       better(cell, c, threshold) to a register counter. Exclusions are ignored here.
//   als_rank_excluded : per target, the user's excluded positions are scored with the same dot and those that come
//                       before the target are taken off again -- len(excl) k work per target against n_cand k.
// The order, the staging and the 4 x 4-cell loop are als_recommend_kernel's: both files take them from
// als_score_tile.h.
#include <climits>
#include <cmath>

#include "als_internal.h"
#include "als_score_tile.h"

namespace cfk {
namespace {

constexpr int TT = score_tile::TR, TC = score_tile::TC, PITCH = score_tile::PITCH;
using score_tile::better;
using score_tile::pair_dot;

// One thread per target entry.
template <class T>
__global__ __launch_bounds__(256) void als_score_pairs(const T* __restrict__ U, const T* __restrict__ M, int kp, int k,
                                                       const int64_t* __restrict__ trow,
                                                       const int32_t* __restrict__ tpos,
                                                       const int64_t* __restrict__ mrows, int64_t n_tgt,
                                                       float* __restrict__ score) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tgt) return;
    score[t] = pair_dot(U + trow[t] * (int64_t)kp, M + mrows[tpos[t]] * (int64_t)kp, k);
}

struct RankArgs {
    const void* U;
    const void* M;
    int kp, k;
    const int64_t* trow;     // [n_tgt] factor row of the target's user
    const int32_t* tpos;     // [n_tgt] the target's candidate position
    const float* tscore;     // [n_tgt] its score (als_score_pairs)
    int64_t n_tgt;
    const int64_t* mrows;
    int64_t n_cand;
    int64_t seg_len;
    int32_t* rank;           // [n_tgt]; several segments: zeroed before the launch
};

// Workgroup (blockIdx.x, blockIdx.y) = (target tile, candidate segment). Thread (ty, tx) of the 16 x 16 grid owns the
// cells of targets ty + 16 i and candidates tx + 16 j (i, j < 4), scored by score_tile::score exactly as in
// als_recommend_kernel.
template <class T>
__global__ __launch_bounds__(256) void als_rank_count(RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rksm[];
    float* su = rksm;                 // [TT][PITCH]
    float* sm = su + TT * PITCH;      // [TC][PITCH]

    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    const int64_t seg_begin = (int64_t)blockIdx.y * a.seg_len;
    const int64_t seg_end = min(a.n_cand, seg_begin + a.seg_len);
    const T* U = (const T*)a.U;
    const T* M = (const T*)a.M;
    const int k = a.k;

    // staging (score_tile::score): this thread loads one feature of rows sr + 8 r
    const int sr = tid >> 5;
    const T* urow[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int64_t t = t0 + sr + 8 * r;
        urow[r] = t < a.n_tgt ? U + a.trow[t] * (int64_t)a.kp : nullptr;   // a row beyond T gathers nothing
    }
    // this thread's 4 thresholds; a row beyond T is never written, its counter is simply not used
    float ts[4];
    int tp[4], cnt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t t = t0 + ty + 16 * i;
        const bool has = t < a.n_tgt;
        ts[i] = has ? a.tscore[t] : INFINITY;
        tp[i] = has ? a.tpos[t] : -1;
        cnt[i] = 0;
    }

    for (int64_t c0 = seg_begin; c0 < seg_end; c0 += TC) {
        const T* mrow[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int64_t c = c0 + sr + 8 * r;
            mrow[r] = c < seg_end ? M + a.mrows[c] * (int64_t)a.kp : nullptr;   // beyond the segment: zeros
        }
        float acc[4][4];
        score_tile::score(acc, su, sm, urow, mrow, k, c0 == seg_begin, tid);

        // count: no branch, no memory; the target's own cell has its score and its position, so it is never counted
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t c = c0 + tx + 16 * j;
            const bool in = c < seg_end;
#pragma unroll
            for (int i = 0; i < 4; ++i) cnt[i] += (in && better(acc[i][j], (int)c, ts[i], tp[i])) ? 1 : 0;
        }
    }

    // the 16 tx lanes of a target row are 16 consecutive lanes of one wave (one DPP row)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int v = cnt[i];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        const int64_t t = t0 + ty + 16 * i;
        if (tx == 0 && t < a.n_tgt) {
            if (gridDim.y == 1) a.rank[t] = v;
            else atomicAdd(&a.rank[t], v);   // integer: independent of the order of the segments
        }
    }
}

// One wave per target, lanes over the exclusion list of the target's user. Runs after als_rank_count on the same
// stream, so the wave owns rank[t].
template <class T>
__global__ __launch_bounds__(256) void als_rank_excluded(const T* __restrict__ U, const T* __restrict__ M, int kp, int k,
                                                         const int64_t* __restrict__ trow,
                                                         const int32_t* __restrict__ tpos,
                                                         const int32_t* __restrict__ tuser,
                                                         const float* __restrict__ tscore, int64_t n_tgt,
                                                         const int64_t* __restrict__ mrows,
                                                         const int64_t* __restrict__ excl_ptr,
                                                         const int32_t* __restrict__ excl_idx,
                                                         int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * 4 + wave;
    if (t >= n_tgt) return;   // whole waves leave; no barrier below
    const int64_t lo = excl_ptr[tuser[t]], hi = excl_ptr[tuser[t] + 1];
    if (hi <= lo) return;
    const T* u = U + trow[t] * (int64_t)kp;
    const float ts = tscore[t];
    const int tp = tpos[t];
    int n = 0;
    for (int64_t x = lo + lane; x < hi; x += 64) {
        const int c = excl_idx[x];
        n += better(pair_dot(u, M + mrows[c] * (int64_t)kp, k), c, ts, tp) ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if (lane == 0 && n) rank[t] -= n;
}

}  // namespace

hipError_t launch_score_pairs(int precision, const void* U, const void* M, int kp, int k, const int64_t* trow,
                              const int32_t* tpos, const int64_t* mrows, int64_t n_tgt, float* score, hipStream_t s) {
    if (n_tgt <= 0) return hipSuccess;
    if (n_tgt > INT32_MAX) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n_tgt + 255) / 256);
    if (precision == 0)
        als_score_pairs<float><<<grid, 256, 0, s>>>((const float*)U, (const float*)M, kp, k, trow, tpos, mrows, n_tgt, score);
    else
        als_score_pairs<double><<<grid, 256, 0, s>>>((const double*)U, (const double*)M, kp, k, trow, tpos, mrows, n_tgt, score);
    return hipGetLastError();
}

hipError_t launch_rank(int precision, const void* U, const void* M, int kp, int k, const int64_t* trow,
                       const int32_t* tpos, const int32_t* tuser, const float* tscore, int64_t n_tgt,
                       const int64_t* mrows, int64_t n_cand, const RankPlan& plan, const int64_t* excl_ptr,
                       const int32_t* excl_idx, int32_t* rank, hipStream_t s) {
    if (n_tgt <= 0 || n_cand <= 0) return hipSuccess;
    if (n_tgt > INT32_MAX || n_cand > INT32_MAX || plan.tgt_tiles > INT32_MAX || plan.segments < 1 ||
        plan.segments > RANK_MAX_SEGMENTS || plan.lds_bytes != rank_lds_bytes() ||
        plan.tgt_tiles * RANK_TGT_TILE < n_tgt || plan.segments * plan.seg_len < n_cand)
        return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (plan.segments > 1) {
        e = hipMemsetAsync(rank, 0, (size_t)n_tgt * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    RankArgs a{};
    a.U = U;
    a.M = M;
    a.kp = kp;
    a.k = k;
    a.trow = trow;
    a.tpos = tpos;
    a.tscore = tscore;
    a.n_tgt = n_tgt;
    a.mrows = mrows;
    a.n_cand = n_cand;
    a.seg_len = plan.seg_len;
    a.rank = rank;
    const dim3 grid((unsigned)plan.tgt_tiles, (unsigned)plan.segments);
    if (precision == 0) als_rank_count<float><<<grid, 256, (size_t)plan.lds_bytes, s>>>(a);
    else als_rank_count<double><<<grid, 256, (size_t)plan.lds_bytes, s>>>(a);
    e = hipGetLastError();
    if (e != hipSuccess || !excl_ptr) return e;
    const unsigned egrid = (unsigned)((n_tgt + 3) / 4);
    if (precision == 0)
        als_rank_excluded<float><<<egrid, 256, 0, s>>>((const float*)U, (const float*)M, kp, k, trow, tpos, tuser, tscore,
                                                      n_tgt, mrows, excl_ptr, excl_idx, rank);
    else
        als_rank_excluded<double><<<egrid, 256, 0, s>>>((const double*)U, (const double*)M, kp, k, trow, tpos, tuser,
                                                       tscore, n_tgt, mrows, excl_ptr, excl_idx, rank);
    return hipGetLastError();
}

}  // namespace cfk
