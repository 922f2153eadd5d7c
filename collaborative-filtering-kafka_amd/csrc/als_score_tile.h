// What als_recommend.hip and als_rank.hip share: the order of the results and the exact scores of one 64 x 64 tile.
//
// Score of (row r, candidate position c) = als_predict's cell: the Java-float dot of a U row and an M row
// (FeatureCollector.java:90-101, EJML multTransB): fp32, product and partial sum rounded separately, features 0..k-1 in
// order, f64 factors narrowed to float first. So the loop is VALU with contraction off -- an f32 MFMA rounds once per
// step -- and runs over the k features, not the padded stride. als_similar.hip takes the one-pair dot from here for its
// norms. Private to those kernel files.
#pragma once
#include "als_plan.h"

namespace cfk {
namespace score_tile {

constexpr int TR = REC_USER_TILE, TC = REC_CAND_TILE, FC = REC_FEAT_CHUNK, PITCH = REC_PITCH;
static_assert(TR == 64 && TC == 64, "a 16 x 16 thread grid of 4 x 4 cells");
static_assert(RANK_TGT_TILE == TR && RANK_CAND_TILE == TC && RANK_FEAT_CHUNK == FC && RANK_PITCH == PITCH,
              "both kernels run the same tile");

// (s, p) comes before (ts, tp) in the result order. False whenever s is NaN.
__device__ __forceinline__ bool better(float s, int p, float ts, int tp) { return s > ts || (s == ts && p < tp); }

// The exact dot of one pair straight from the tables: strictly sequential in feature order (als_score_pairs, and the
// squared norms of als_similar: pair_dot(r, r, k)).
template <class T>
__device__ __forceinline__ float pair_dot(const T* __restrict__ u, const T* __restrict__ m, int k) {
    float total = 0.f;
    {
#pragma clang fp contract(off)
        for (int f = 0; f < k; ++f) total = total + (float)u[f] * (float)m[f];   // rounded product, rounded sum
    }
    return total;
}

// The 4 x 4 cells of thread (ty, tx) = (tid >> 4, tid & 15) of a 256-thread workgroup: rows ty + 16 i, candidates
// tx + 16 j (i, j < 4). su [TR][PITCH] and sm [TC][PITCH] are the staged tiles in LDS; the 16 candidate rows a wave
// reads in one step are PITCH = 33 words apart (16 banks), its 4 rows of su are broadcasts. 16 independent accumulator
// chains per thread give the ILP; each chain is strictly in feature order across the staged chunks.
// Staging: thread -> feature tid & 31 of rows (tid >> 5) + 8 r (a wave loads two 128-byte row pieces per step);
// urow[r] / mrow[r] point at those factor rows, nullptr stages zeros. With one feature chunk (k <= FC) the rows of su
// are staged only when stage_u_once says so (the first tile of a sweep) and kept for the tiles after it.
// Every thread of the workgroup calls this; it starts with a barrier, so the caller's earlier LDS writes are visible and
// the previous tile's reads are over.
template <class T>
__device__ __forceinline__ void score(float (&acc)[4][4], float* su, float* sm, const T* const (&urow)[8],
                                      const T* const (&mrow)[8], int k, bool stage_u_once, int tid) {
    const int tx = tid & 15, ty = tid >> 4;
    const int sf = tid & 31, sr = tid >> 5;
    const int n_chunks = (k + FC - 1) / FC;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const int f0 = ch * FC;
        const int fc = min(FC, k - f0);
        const bool stage_u = n_chunks > 1 || stage_u_once;
        __syncthreads();   // the previous pass has read its tiles (first pass: the initial state is written)
        if (sf < fc) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = sr + 8 * r;
                if (stage_u) su[row * PITCH + sf] = urow[r] ? (float)urow[r][f0 + sf] : 0.f;
                sm[row * PITCH + sf] = mrow[r] ? (float)mrow[r][f0 + sf] : 0.f;
            }
        }
        __syncthreads();
        {
#pragma clang fp contract(off)
            for (int f = 0; f < fc; ++f) {
                float uv[4], mv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) uv[i] = su[(ty + 16 * i) * PITCH + f];
#pragma unroll
                for (int j = 0; j < 4; ++j) mv[j] = sm[(tx + 16 * j) * PITCH + f];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + uv[i] * mv[j];   // rounded product, rounded sum
            }
        }
    }
}

}  // namespace score_tile
}  // namespace cfk
