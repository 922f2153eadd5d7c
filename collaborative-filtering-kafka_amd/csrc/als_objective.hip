// The implicit-feedback loss without the dense grid (als_implicit_objective). For a row x of one side with entries e
// (opposite rows y_e, ratings r_e >= 0) and G = Y^T Y of the whole opposite table,
//   f(x) = x^T G x  +  sum_e [ (1 + alpha r_e)(p_e - s_e)^2 - s_e^2 ]  +  lambda x^T x,    s_e = y_e . x,  p_e = [r_e > 0]
// is x^T A x - 2 b^T x + sum_{r_e > 0} (1 + alpha r_e) with the A and b of als_solve_implicit, and the sum of f over the
// rows of a side plus lambda tr(G) is the Hu-Koren-Volinsky loss over the full grid: the -s_e^2 takes the observed
// cells out of x^T G x, which counts every cell of the row with confidence 1 and preference 0.
//
// als_objective_kernel<T, KP>: one 256-thread workgroup per query, grid-stride over the host's longest-first
// permutation. All arithmetic after the loads is double in both engine precisions.
//   x      : the k true features of factor row rows[q] go into LDS as double (columns >= k count as zero).
//   G x    : thread f < k forms (G x)_f = sum_j G[j][f] x_j in ascending j -- G is symmetric, so the column read is
//            consecutive threads, consecutive addresses -- then x_f (G x)_f and x_f^2.
//   entries: dealt over groups of objective_group_lanes lanes, each lane one 16-byte piece of the row (the groups of the
//            fp64 strides 80, 96 and 112 are rounded up to 64 lanes, the extra lanes hold zeros). Group g takes the
//            entries g, g + NG, g + 2 NG, ... in that order: one row gather, one dot, summed over the group's lanes by an
//            xor butterfly (every lane ends with the same bits), then the term. An entry with r = 0 has p = 0 and
//            confidence 1: its term is s^2 - s^2 and is taken as the exact 0 it is, so no contraction of the expression
//            can leave a rounding residue.
//   sums   : the three per-thread partials go through a 64-lane xor butterfly and then, per wave, through LDS, where
//            thread 0 adds the four waves in ascending order. One fixed order, no atomics: a query's three doubles
//            depend on its entries, x, G, lambda and alpha only.
// als_gram_trace_kernel: lambda sum_{f < k} G[f][f] in ascending f, the ridge of the opposite side.
// DESIGN.md section 3.12 has the model, the resource figures and the measurements.
#include <climits>
#include <type_traits>

#include "als_device.h"

namespace cfk {
namespace {

// one shuffle of a double: two 32-bit halves
__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
    const long long b = __double_as_longlong(v);
    const int lo = __shfl_xor((int)(unsigned)(b & 0xffffffffll), m);
    const int hi = __shfl_xor((int)(b >> 32), m);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

template <class T, int KP>
__global__ __launch_bounds__(OBJECTIVE_THREADS) void als_objective_kernel(ObjectiveArgs a) {
    constexpr int VN = Vec16<T>::N;
    constexpr int LPE = KP / VN;                                      // lanes that hold a piece of a row
    constexpr int GL = objective_group_lanes(KP, (int)sizeof(T));     // lanes per group: a power of two >= LPE
    constexpr int NG = OBJECTIVE_THREADS / GL;                        // groups of the workgroup
    constexpr int UNROLL = 4;                                         // row gathers in flight per group
    static_assert(GL >= LPE && GL <= 64 && (GL & (GL - 1)) == 0, "a group is a power-of-two part of a wave");
    using VT = typename Vec16<T>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char osm[];
    double* xs = (double*)osm;     // [KP] x
    double* red = xs + KP;         // [OBJECTIVE_RED_SLOTS] the waves' sums: [wave][3]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = tid / GL, v = tid % GL;
    const int ke = a.k;
    const T* opp = (const T*)a.opp;
    const T* Gt = (const T*)a.gram;
    const double alpha = (double)a.alpha, lambda = (double)a.lambda;

    for (int64_t qi = blockIdx.x; qi < a.n_queries; qi += gridDim.x) {
        const int64_t q = a.order[qi];
        const int64_t lo = a.q_ptr[q];
        const int n = (int)(a.q_ptr[q + 1] - lo);
        const T* x = (const T*)a.self + a.rows[q] * (int64_t)KP;
        if (tid < KP) xs[tid] = tid < ke ? (double)x[tid] : 0.0;
        __syncthreads();

        // quadratic form and ridge, thread f < k
        double quad = 0.0, ridge = 0.0;
        if (tid < ke) {
            double gx = 0.0;
            for (int j = 0; j < ke; ++j) gx += (double)Gt[j * KP + tid] * xs[j];
            const double xf = xs[tid];
            quad = xf * gx;
            ridge = xf * xf;
        }

        // the entries of group g, ascending
        double xv[VN];
#pragma unroll
        for (int c = 0; c < VN; ++c) xv[c] = v < LPE ? xs[(v < LPE ? v : 0) * VN + c] : 0.0;
        const int32_t* idx = a.q_idx + lo;
        const int16_t* rat = a.q_rat + lo;
        double obs = 0.0;
        for (int base = g; base < n; base += NG * UNROLL) {
            VT y[UNROLL];
            int r[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int e = base + u * NG;
                y[u] = VT{};
                r[u] = -1;   // no entry
                if (e < n) {
                    r[u] = rat[e];
                    if (v < LPE) y[u] = *(const VT*)(opp + (int64_t)idx[e] * KP + v * VN);
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < VN; ++c) s += (double)y[u][c] * xv[c];
#pragma unroll
                for (int m = 1; m < GL; m <<= 1) s += shfl_xor_f64(s, m);
                if (r[u] > 0) {
                    const double d = 1.0 - s;
                    obs += (1.0 + alpha * (double)r[u]) * (d * d) - s * s;
                }
            }
        }
        if (v != 0) obs = 0.0;   // every lane of a group holds the group's sum: count it once

        // one fixed order: the wave's 64 lanes, then the four waves
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            quad += shfl_xor_f64(quad, m);
            obs += shfl_xor_f64(obs, m);
            ridge += shfl_xor_f64(ridge, m);
        }
        if (lane == 0) {
            red[wave * 3 + 0] = quad;
            red[wave * 3 + 1] = obs;
            red[wave * 3 + 2] = ridge;
        }
        __syncthreads();
        if (tid < 3) {
            double s = red[tid];
#pragma unroll
            for (int w = 1; w < OBJECTIVE_THREADS / 64; ++w) s += red[w * 3 + tid];
            a.parts[q * 3 + tid] = tid == 2 ? lambda * s : s;
        }
        // the next query's xs is written before a barrier and its red after one: no further barrier is needed here
    }
}

template <class T>
__global__ __launch_bounds__(64) void als_gram_trace_kernel(const T* __restrict__ gram, int kp, int k, float lambda,
                                                           double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int f = 0; f < k; ++f) s += (double)gram[f * kp + f];
    *out = (double)lambda * s;
}

// f(std::integral_constant<int, KP>) for the stride kp of an engine of element type T: fold_by_kp's strides.
template <class T, class F>
hipError_t objective_by_kp(int kp, F&& f) {
    switch (kp) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: break;
    }
    if constexpr (std::is_same<T, double>::value) {
        switch (kp) {
            case 80: return f(std::integral_constant<int, 80>{});
            case 96: return f(std::integral_constant<int, 96>{});
            case 112: return f(std::integral_constant<int, 112>{});
            default: break;
        }
    }
    return hipErrorInvalidValue;
}

template <class T>
hipError_t launch_objective_t(int kp, const ObjectiveArgs& a, const ObjectivePlan& plan, hipStream_t s) {
    const hipError_t e = objective_by_kp<T>(kp, [&](auto kpc) {
        constexpr int KP = decltype(kpc)::value;
        als_objective_kernel<T, KP><<<(unsigned)plan.grid, OBJECTIVE_THREADS, (size_t)plan.lds_bytes, s>>>(a);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    als_gram_trace_kernel<T><<<1, 64, 0, s>>>((const T*)a.gram, kp, a.k, a.lambda, a.parts + 3 * a.n_queries);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_objective(int precision, int kp, const ObjectiveArgs& a, const ObjectivePlan& plan, hipStream_t s) {
    if (a.n_queries <= 0) return hipSuccess;
    const int elem = precision == 0 ? 4 : 8;
    // the plan is the one objective_plan returns for this shape (the compute units enter the grid only: at most the
    // queries, at least 1)
    const ObjectivePlan want = objective_plan(kp, elem, a.n_queries, 0);
    if (kp > FOLDIN_MAX_KP || a.k < 1 || a.k > kp || !a.opp || !a.self || !a.gram || !a.q_ptr || !a.q_idx || !a.q_rat ||
        !a.rows || !a.order || !a.parts || plan.threads != OBJECTIVE_THREADS || plan.lds_bytes != want.lds_bytes ||
        plan.grid < 1 || plan.grid > a.n_queries || plan.grid > INT32_MAX)
        return hipErrorInvalidValue;
    return precision == 0 ? launch_objective_t<float>(kp, a, plan, s) : launch_objective_t<double>(kp, a, plan, s);
}

}  // namespace cfk
