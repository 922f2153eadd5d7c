// Private part of als_kernels.hip: the any-k kernels (fp32 k > 128, fp64 k > 64) -- one workgroup per row solve,
// squared error and collector prediction. Correctness for every k, not a benchmark configuration.
#pragma once

#include "als_device.h"

namespace cfk {
namespace {

// ---------------------------------------------------------------------------------------------------
// Generic path: any num_features beyond the wave-per-row kernels (fp32 k > 128, fp64 k > 64)
// ---------------------------------------------------------------------------------------------------
// One 256-thread workgroup per row (FULL tasks only: the work plan never splits a row on this path), grid-stride
// over the rows. MFeatureCalculator.java:85-99 for that row: the Gram's lower triangle and the RHS accumulated over
// LDS-staged batches of gathered factor rows, A + lambda n I (padded features: identity), a right-looking Cholesky
// (one pivot column per step, the trailing update spread over the workgroup), forward and backward substitution.
// G_LDS: the packed lower triangle lives in LDS while it and eight staged rows fit beside the static vectors below
// (generic_plan, als_plan.cpp: kp <= 272 in fp32, <= 176 in fp64, where a batch is down to 10 and 15 rows); otherwise
// in a per-workgroup slab of `scratch` (slab elements each). Not a benchmark configuration: correctness for every k (ALSAppRunner.java:18
// accepts any NUM_FEATURES), at the cost of O(k^2) LDS traffic per gathered row.
template <class T, bool G_LDS>
__global__ __launch_bounds__(256) void als_solve_generic(SolveArgs a, int kp, int batch, T* __restrict__ scratch,
                                                         int64_t slab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsmem[];
    const int tid = threadIdx.x;
    const int64_t ntri = (int64_t)kp * (kp + 1) / 2;
    T* G = G_LDS ? (T*)gsmem : scratch + (int64_t)blockIdx.x * slab;   // packed lower triangle, tri(i, j)
    T* stage = (T*)gsmem + (G_LDS ? ((ntri + 1) & ~(int64_t)1) : 0); // batch x kp gathered rows
    constexpr bool F64 = std::is_same<T, double>::value;
    __shared__ T vec[generic_vec_elems()];      // RHS / solution (kp <= GENERIC_MAX_KP) + pivot
    // fp64: the refinement step's residual / correction and per-entry residuals of a batch (<= GENERIC_MAX_BATCH)
    __shared__ T res[generic_res_elems(F64)];
    __shared__ T tb[generic_tb_elems(F64)];
    // what generic_plan leaves out of the dynamic LDS budget (the 16-byte aligned gsmem rounds the statics up)
    static_assert(sizeof(vec) + sizeof(res) + sizeof(tb) <= (size_t)generic_static_lds_bytes(F64) &&
                      (size_t)generic_static_lds_bytes(F64) < sizeof(vec) + sizeof(res) + sizeof(tb) + GENERIC_LDS_ALIGN,
                  "generic_plan's static LDS is not this kernel's");
    const T* opp = (const T*)a.opp;
    auto tri_ = [](int64_t i, int64_t j) { return i * (i + 1) / 2 + j; };
    for (int task = blockIdx.x; task < a.n_tasks; task += gridDim.x) {
        const Task tk = a.tasks[task];
        T* out = (T*)a.out + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)kp;
        for (int64_t x = tid; x < ntri; x += 256) G[x] = T(0);
        for (int i = tid; i < kp; i += 256) vec[i] = T(0);
        __syncthreads();
        const int n = (tk.nsteps + BLOCK_SUBSTEPS - 1) / BLOCK_SUBSTEPS * BLOCK_ENTRIES;   // padded span
        for (int base = 0; base < n; base += batch) {
            const int nb = min(batch, n - base);
            for (int x = tid; x < nb * kp; x += 256) {   // padding entries gather the zero sentinel row
                const int e = x / kp, f = x - e * kp;
                stage[x] = opp[(int64_t)a.col[tk.begin + base + e] * kp + f];
            }
            __syncthreads();
            for (int i = tid; i < kp; i += 256) {
                T acc = vec[i];
                for (int e = 0; e < nb; ++e) acc += (T)a.rat[tk.begin + base + e] * stage[e * kp + i];
                vec[i] = acc;
            }
            for (int64_t x = tid; x < ntri; x += 256) {
                // row i of the packed triangle holding x: i (i + 1) / 2 <= x
                int64_t i = (int64_t)((sqrt(8.0 * (double)x + 1.0) - 1.0) / 2.0);
                while (i * (i + 1) / 2 > x) --i;
                while ((i + 1) * (i + 2) / 2 <= x) ++i;
                const int64_t j = x - i * (i + 1) / 2;
                T acc = G[x];
                for (int e = 0; e < nb; ++e) acc += stage[e * kp + i] * stage[e * kp + j];
                G[x] = acc;
            }
            __syncthreads();
        }
        if (tk.ndeg == 0) {   // cannot occur in the reference; defined as 0 (as the other paths)
            for (int i = tid; i < kp; i += 256) out[i] = T(0);
            __syncthreads();
            continue;
        }
        const T reg = (T)a.lambda * (T)tk.ndeg;   // A + lambda * (float) n on the diagonal (MFeatureCalculator.java:91-95)
        for (int i = tid; i < kp; i += 256) {
            const int64_t d = tri_(i, i);
            G[d] = i < a.k ? G[d] + reg : T(1);
        }
        __syncthreads();
        for (int j = 0; j < kp; ++j) {   // Cholesky: column j of L, then the trailing update
            if (tid == 0) {
                const T d = sqrt(G[tri_(j, j)]);
                G[tri_(j, j)] = d;
                vec[GENERIC_MAX_KP] = d;
            }
            __syncthreads();
            const T d = vec[GENERIC_MAX_KP];
            for (int i = j + 1 + tid; i < kp; i += 256) G[tri_(i, j)] /= d;
            __syncthreads();
            const int m = kp - j - 1;
            for (int64_t x = tid; x < (int64_t)m * m; x += 256) {
                const int i = j + 1 + (int)(x / m), l = j + 1 + (int)(x % m);
                if (l <= i) G[tri_(i, l)] -= G[tri_(i, j)] * G[tri_(l, j)];
            }
            __syncthreads();
        }
        auto chol_solve = [&](T* v) {   // v <- (L L^T)^{-1} v
            for (int j = 0; j < kp; ++j) {   // forward: L y = v
                const T y = v[j] / G[tri_(j, j)];
                __syncthreads();
                if (tid == 0) v[j] = y;
                for (int i = j + 1 + tid; i < kp; i += 256) v[i] -= G[tri_(i, j)] * y;
                __syncthreads();
            }
            for (int j = kp - 1; j >= 0; --j) {   // backward: L^T x = y
                const T x = v[j] / G[tri_(j, j)];
                __syncthreads();
                if (tid == 0) v[j] = x;
                for (int i = tid; i < j; i += 256) v[i] -= G[tri_(j, i)] * x;
                __syncthreads();
            }
        };
        chol_solve(vec);
        if constexpr (std::is_same<T, double>::value) {
            // fp64 parity mode: one step of iterative refinement, x += (L L^T)^{-1} (b - A x), with the residual
            // formed from the rows themselves (A x = Y^T (Y x) + lambda n x; the triangle now holds L):
            // b - A x = sum_e y_e (r_e - y_e . x) - lambda n x. The Cholesky's own error on the near-zero elements
            // of a wide solution (~cond * eps of the row norm) drops by about cond.
            for (int i = tid; i < kp; i += 256) res[i] = -(i < a.k ? reg : T(1)) * vec[i];
            __syncthreads();
            const int wv = tid >> 6, ln = tid & 63;
            for (int base = 0; base < n; base += batch) {
                const int nb = min(batch, n - base);
                for (int x = tid; x < nb * kp; x += 256) {
                    const int e = x / kp, f = x - e * kp;
                    stage[x] = opp[(int64_t)a.col[tk.begin + base + e] * kp + f];
                }
                __syncthreads();
                for (int e = wv; e < nb; e += 4) {   // t_e = r_e - y_e . x, one wave per entry
                    T d = T(0);
                    for (int f = ln; f < kp; f += 64) d += stage[e * kp + f] * vec[f];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
                    if (ln == 0) tb[e] = (T)a.rat[tk.begin + base + e] - d;
                }
                __syncthreads();
                for (int i = tid; i < kp; i += 256) {
                    T acc = res[i];
                    for (int e = 0; e < nb; ++e) acc += stage[e * kp + i] * tb[e];
                    res[i] = acc;
                }
                __syncthreads();
            }
            chol_solve(res);
            for (int i = tid; i < kp; i += 256) vec[i] += res[i];
            __syncthreads();
        }
        for (int i = tid; i < kp; i += 256) out[i] = i < a.k ? vec[i] : T(0);
        __syncthreads();
    }
}

// Squared error of the generic path (any kp): one wave per task, lane = feature stripe.
template <class T>
__global__ __launch_bounds__(256) void als_sq_error_generic(SqErrArgs a, int kp) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tid = blockIdx.x * WAVES + wave;
    if (tid >= a.n_tasks) return;
    const Task tk = load_task(a.tasks + tid);
    const T* self = (const T*)a.self + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)kp;
    const T* opp = (const T*)a.opp;
    double se = 0.0;
    const int n = (tk.nsteps + BLOCK_SUBSTEPS - 1) / BLOCK_SUBSTEPS * BLOCK_ENTRIES;
    for (int e = 0; e < n; ++e) {
        const int w = e % BLOCK_ENTRIES;
        const int logical = e - w + (w % BLOCK_SUBSTEPS) * 4 + w / BLOCK_SUBSTEPS;
        if (logical >= tk.nent) continue;   // wave-uniform
        const T* y = opp + (int64_t)a.col[tk.begin + e] * kp;
        T dot = T(0);
        for (int f = lane; f < kp; f += 64) dot += self[f] * y[f];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) dot += __shfl_xor(dot, m);
        const double d = (double)a.rat[tk.begin + e] - (double)dot;
        se += d * d;
    }
    if (lane == 0) a.task_se[tid] = se;
}

// Collector dot products for any k (FeatureCollector.java:90-101, Java-float order): one thread per cell.
template <class T>
__global__ __launch_bounds__(256) void als_predict_generic(const T* __restrict__ U, const T* __restrict__ M, int kp,
                                                           int k, const int64_t* __restrict__ urows, int64_t n_u,
                                                           const int64_t* __restrict__ mrows, int64_t n_m,
                                                           float* __restrict__ out) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_u * n_m) return;
    const int64_t u = cell / n_m, m = cell % n_m;
    const T* x = U + urows[u] * kp;
    const T* y = M + mrows[m] * kp;
    float total = 0.f;
    {
#pragma clang fp contract(off)
        for (int f = 0; f < k; ++f) total = total + (float)x[f] * (float)y[f];
    }
    out[cell] = total;
}

}  // namespace
}  // namespace cfk
