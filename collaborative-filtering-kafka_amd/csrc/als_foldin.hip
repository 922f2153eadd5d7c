// Fold-in (als_fold_in): the factor row of a query that was not in the training block, from its ratings and the
// resident opposite factors -- x = (Y_S^T Y_S + lambda n I)^-1 Y_S^T r, the reference's normal equation
// (MFeatureCalculator.java:85-99), over ad-hoc rows. A serving path: one to a few thousand short rows per call, no work
// plan, no padded in-block, no per-engine state.
//
// One 256-thread workgroup owns one whole query (grid-stride over the queries), so a query's bits depend on nothing but
// its own entries: no atomics, no split across workgroups, every sum in one fixed order.
//   gather : batches of the query's opposite rows go into LDS through q_idx, 16 bytes per lane, a row's loads
//            contiguous; the tail of the last batch is zero-filled up to a whole MFMA step (4 entries). The next batch
//            is loaded into registers while the Gram of the current one runs.
//   Gram   : lower-triangle 16 x 16 tiles of Y^T Y on the matrix pipe at full input precision
//            (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64: a k-ordered fma chain per element). The tiles are dealt
//            over the 4 waves (tile t to wave t % 4) and stay in accumulator registers over all batches. Per 4 entries a
//            wave reads one operand register per 16-feature block it needs -- lane (g, c) holds Y[entry 4 s + g][16 b + c],
//            which is both the A operand of tile row b and the B operand of tile column b -- and issues all its tiles.
//   RHS    : Y^T r on the VALU, thread f < KP owns feature f, entries in order.
//   solve  : the tiles go through LDS into a thread-per-element layout; A + lambda n I, Jacobi scaling, a right-looking
//            Cholesky in registers over the k true features (the padded ones are an identity block that nothing couples
//            to; one barrier per column, the pivot column broadcast through LDS), forward and backward substitution
//            with the vector in registers (one barrier per step). fp64 adds the one refinement step of
//            als_solve_generic, the residual formed from the rows themselves.
// KP is the engine's factor stride: 16, 32, 64 or 128, and in fp64 also 80, 96 and 112 (65..112 features are on the
// generic solve path there, whose stride is the next multiple of 16).
// DESIGN.md section 3.9 has the layout, the resource figures and the measurements.
#include <climits>
#include <type_traits>

#include "als_device.h"

namespace cfk {
namespace {

#include "als_fold_tiles.h"   // accumulator types, tile maps, fold_gram_batch, fold_store_tiles, FoldBatch

template <class T, int KP>
__global__ __launch_bounds__(FOLDIN_THREADS) void als_fold_in_kernel(FoldinArgs a, int batch) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), MT = (NT + 3) / 4, P = foldin_pitch(KP);
    constexpr bool REFINE = std::is_same<T, double>::value;
    typedef typename FoldAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
    T* G = (T*)fsm;                               // [NT][16][FOLDIN_TILE_PITCH]
    T* stage = G + NT * FOLDIN_TILE_ELEMS;        // [batch][P]
    T* scl = stage + batch * P;                   // [KP] Jacobi scale 1 / sqrt(a_ii)
    T* dg = scl + KP;                             // [KP] diagonal of L
    T* bc = dg + KP;                              // [KP] substitution: the component being broadcast
    T* xs = bc + KP;                              // [KP] solution (refinement)
    T* tb = xs + KP;                              // [batch] ratings, then per-entry residuals
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    const int ke = a.k;
    const T* opp = (const T*)a.opp;

    // v <- (L L^T)^-1 v for the vector held one component per thread (tid < ke)
    auto chol_solve = [&](T v) -> T {
        for (int j = 0; j < ke; ++j) {   // forward: L y = v
            if (tid == j) bc[j] = v / dg[j];
            __syncthreads();
            if (tid > j && tid < ke) v -= G[fold_at(tid, j)] * bc[j];
        }
        T y = tid < ke ? bc[tid] : T(0);
        __syncthreads();
        for (int j = ke - 1; j >= 0; --j) {   // backward: L^T x = y
            if (tid == j) bc[j] = y / dg[j];
            __syncthreads();
            if (tid < j) y -= G[fold_at(j, tid)] * bc[j];
        }
        const T x = tid < ke ? bc[tid] : T(0);
        __syncthreads();
        return x;
    };

    for (int64_t q = blockIdx.x; q < a.n_queries; q += gridDim.x) {
        const int64_t lo = a.q_ptr[q];
        const int n = (int)(a.q_ptr[q + 1] - lo);
        T* out = (T*)a.out + q * KP;
        T* dst = a.dst_rows ? (T*)a.self + a.dst_rows[q] * KP : nullptr;
        if (n == 0) {   // cannot occur in the reference; defined as 0 (as every other path). Workgroup-uniform.
            if (tid < KP) {
                out[tid] = T(0);
                if (dst) dst[tid] = T(0);
            }
            continue;
        }
        const int32_t* idx = a.q_idx + lo;
        const int16_t* rat = a.q_rat + lo;

        Acc acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = Acc{};
        T rhs = T(0);
        FoldBatch<T, KP> fb;
        fold_load<T, KP>(fb, opp, idx, rat, min(batch, n), tid);
        for (int base = 0; base < n; base += batch) {
            const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
            fold_store<T, KP>(fb, stage, tb, nb4, tid);
            __syncthreads();
            if (base + batch < n)   // the next batch's rows travel while this one is multiplied
                fold_load<T, KP>(fb, opp, idx + base + batch, rat + base + batch, min(batch, n - base - batch), tid);
            if (tid < KP)
                for (int e = 0; e < nb; ++e) rhs += tb[e] * stage[e * P + tid];
            FOLD_BY_WAVE(wave, fold_gram_batch, acc, stage, nb4 >> 2, lane)
            __syncthreads();
        }
        FOLD_BY_WAVE(wave, fold_store_tiles, acc, G, lane)
        __syncthreads();

        // A + lambda (float) n I on the true features (MFeatureCalculator.java:91-95), then D^-1/2 A D^-1/2
        const T reg = (T)a.lambda * (T)n;
        if (tid < KP) {
            T s = T(1);
            if (tid < ke) {
                const T d = G[fold_at(tid, tid)] + reg;
                G[fold_at(tid, tid)] = d;
                s = T(1) / sqrt(d);
            }
            scl[tid] = s;
        }
        __syncthreads();
        // Right-looking Cholesky in registers: thread (ty, tx) owns element (ty, tx) of every tile, scaled as it is loaded.
        // Column j = 16 J + jj: its owners (tx = jj) publish the unscaled column, pivot included, through LDS (two
        // buffers in turn, one barrier per column); every thread scales the entries of its rows and columns by
        // 1 / sqrt(pivot) itself, the owners keep theirs as L, and the trailing tiles take the rank-1 update. J is a
        // compile-time index, so no register array is indexed dynamically. Rows above the diagonal of a diagonal tile
        // hold values nobody reads.
        const int ty = tid >> 4, tx = tid & 15;
        const int own = ty * FOLDIN_TILE_PITCH + tx;
        T g[NT];
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            g[tt] = G[tt * FOLDIN_TILE_ELEMS + own] * scl[16 * fold_tile_row(tt) + ty] * scl[16 * fold_tile_col(tt) + tx];
        });
        static_for<0, C>([&](auto Jc) {
            constexpr int J = decltype(Jc)::value;
            for (int jj = 0; jj < 16; ++jj) {
                const int j = 16 * J + jj;
                if (j < ke) {   // workgroup-uniform
                    T* cb = (j & 1) ? xs : bc;
                    if (tx == jj) static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        cb[16 * A + ty] = g[A * (A + 1) / 2 + J];
                    });
                    __syncthreads();
                    const T piv = cb[j];
                    const T rinv = T(1) / sqrt(piv);
                    if (tid == 0) dg[j] = sqrt(piv);
                    T li[C], ll[C];
                    static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        li[A] = cb[16 * A + ty] * rinv;
                        ll[A] = cb[16 * A + tx] * rinv;
                    });
                    static_for<J, C>([&](auto ac) {
                        constexpr int A = decltype(ac)::value;
                        // tile (A, J): the column itself where tx = jj, the finished columns left of it stay
                        T& gj = g[A * (A + 1) / 2 + J];
                        gj = tx == jj ? li[A] : (tx > jj ? gj - li[A] * ll[J] : gj);
                        static_for<J + 1, A + 1>([&](auto bc_) {
                            constexpr int B = decltype(bc_)::value;
                            g[A * (A + 1) / 2 + B] -= li[A] * ll[B];
                        });
                    });
                }
            }
        });
        __syncthreads();   // the last column's readers are done with bc / xs, which the substitution reuses
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            G[tt * FOLDIN_TILE_ELEMS + own] = g[tt];
        });
        __syncthreads();
        T x = chol_solve(rhs * (tid < KP ? scl[tid] : T(0)));
        x *= tid < KP ? scl[tid] : T(0);
        if constexpr (REFINE) {
            // one step of iterative refinement, x += A^-1 (b - A x), the residual from the rows themselves:
            // b - A x = sum_e y_e (r_e - y_e . x) - lambda n x (the triangle now holds L)
            if (tid < KP) xs[tid] = x;
            T res = -reg * x;
            __syncthreads();
            for (int base = 0; base < n; base += batch) {
                const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
                fold_load<T, KP>(fb, opp, idx + base, rat + base, nb, tid);
                fold_store<T, KP>(fb, stage, tb, nb4, tid);
                __syncthreads();
                for (int e = wave; e < nb; e += 4) {   // t_e = r_e - y_e . x, one wave per entry
                    T d = T(0);
                    for (int f = lane; f < KP; f += 64) d += stage[e * P + f] * xs[f];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
                    if (lane == 0) tb[e] -= d;
                }
                __syncthreads();
                if (tid < KP)
                    for (int e = 0; e < nb; ++e) res += stage[e * P + tid] * tb[e];
                __syncthreads();
            }
            const T dx = chol_solve(res * (tid < KP ? scl[tid] : T(0)));
            x += dx * (tid < KP ? scl[tid] : T(0));
        }
        if (tid < KP) {
            const T v = tid < ke ? x : T(0);
            out[tid] = v;
            if (dst) dst[tid] = v;
        }
        __syncthreads();
    }
}

template <class T, int KP>
hipError_t launch_one(const FoldinArgs& a, const FoldinPlan& plan, hipStream_t s) {
    // the fp64 k = 128 shape needs more than the 64 KiB a kernel gets by default. Every call sets the same bound per
    // instantiation (its plan does not depend on the call), so engines of several devices and host threads cannot lower
    // it under one another's launch.
    hipError_t e = hipFuncSetAttribute((const void*)als_fold_in_kernel<T, KP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)plan.lds_bytes);
    if (e != hipSuccess) return e;
    als_fold_in_kernel<T, KP><<<(unsigned)plan.grid, FOLDIN_THREADS, (size_t)plan.lds_bytes, s>>>(a, plan.batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_kp(int kp, const FoldinArgs& a, const FoldinPlan& plan, hipStream_t s) {
    switch (kp) {
        case 16: return launch_one<T, 16>(a, plan, s);
        case 32: return launch_one<T, 32>(a, plan, s);
        case 64: return launch_one<T, 64>(a, plan, s);
        case 128: return launch_one<T, 128>(a, plan, s);
        default: break;
    }
    // fp64 engines of 65..112 features are on the generic solve path, whose stride is the next multiple of 16
    if constexpr (std::is_same<T, double>::value) {
        switch (kp) {
            case 80: return launch_one<T, 80>(a, plan, s);
            case 96: return launch_one<T, 96>(a, plan, s);
            case 112: return launch_one<T, 112>(a, plan, s);
            default: break;
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_fold_in(int precision, int kp, const FoldinArgs& a, const FoldinPlan& plan, hipStream_t s) {
    if (a.n_queries <= 0) return hipSuccess;
    const int elem = precision == 0 ? 4 : 8;
    if (kp > FOLDIN_MAX_KP || a.k < 1 || a.k > kp || plan.threads != FOLDIN_THREADS || plan.grid < 1 ||
        plan.grid > a.n_queries || plan.grid > INT32_MAX || plan.batch < 4 || plan.batch % 4 != 0 ||
        plan.batch > FOLDIN_MAX_BATCH || plan.lds_bytes != foldin_lds_bytes(kp, elem, plan.batch) ||
        plan.lds_bytes > FOLDIN_LDS_LIMIT)
        return hipErrorInvalidValue;
    return precision == 0 ? launch_kp<float>(kp, a, plan, s) : launch_kp<double>(kp, a, plan, s);
}

}  // namespace cfk
