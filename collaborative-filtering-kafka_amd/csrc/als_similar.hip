// Nearest factor rows of one table (als_similar): the inverse norms of the listed rows. The
// sweep itself is als_recommend_kernel under its SIM policy (als_recommend.hip, launch_similar_sweep).
//
// inv(r) = 1.0f / sqrtf(cell(r, r)), 0 when cell(r, r) == 0, with cell = als_predict's cell (score_tile::pair_dot: fp32,
// product and partial sum rounded separately, features in order, f64 factors narrowed first). The square root and the
// division are IEEE-correctly rounded: the file is built with the default flags (no fast-math), under which sqrtf and
// the fp32 division are the refined sequences with fp32 denormals on.
#include <climits>
#include <cmath>

#include "als_internal.h"
#include "als_score_tile.h"

namespace cfk {
namespace {

// One thread per listed row: the queries first, then the candidates.
template <class T>
__global__ __launch_bounds__(256) void als_similar_norms(const T* __restrict__ table, int kp, int k,
                                                         const int64_t* __restrict__ qrows, int64_t n_queries,
                                                         const int64_t* __restrict__ crows, int64_t n_cand,
                                                         float* __restrict__ inv_q, float* __restrict__ inv_c) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_queries + n_cand) return;
    const bool is_q = t < n_queries;
    const int64_t i = is_q ? t : t - n_queries;
    const T* row = table + (is_q ? qrows[i] : crows[i]) * (int64_t)kp;
    const float d = score_tile::pair_dot(row, row, k);
    const float inv = d == 0.f ? 0.f : 1.0f / sqrtf(d);
    (is_q ? inv_q : inv_c)[i] = inv;
}

}  // namespace

hipError_t launch_similar_norms(int precision, const void* table, int kp, int k, const int64_t* qrows, int64_t n_queries,
                                const int64_t* crows, int64_t n_cand, float* inv_q, float* inv_c, hipStream_t s) {
    const int64_t n = n_queries + n_cand;
    if (n_queries < 0 || n_cand < 0 || n <= 0) return hipSuccess;
    if ((n + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + 255) / 256);
    if (precision == 0)
        als_similar_norms<float><<<grid, 256, 0, s>>>((const float*)table, kp, k, qrows, n_queries, crows, n_cand, inv_q, inv_c);
    else
        als_similar_norms<double><<<grid, 256, 0, s>>>((const double*)table, kp, k, qrows, n_queries, crows, n_cand, inv_q, inv_c);
    return hipGetLastError();
}

}  // namespace cfk
