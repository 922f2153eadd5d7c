// Implicit-feedback ALS (Hu, Koren, Volinsky 2008; als_gram_table, als_solve_implicit). Every unobserved pair is a weak
// negative, so the per-query system holds the Gram of the whole opposite table:
//   G = Y^T Y,   A = G + alpha sum_e r_e y_e y_e^T + lambda I,   b = sum_{e: r_e > 0} (1 + alpha r_e) y_e,   x = A^-1 b
// (confidence c = 1 + alpha r, preference p = [r > 0]; plain lambda, not lambda n).
//
// Table Gram: slab s of the table (gram_table_plan: a function of the row count alone) goes through LDS in batches of
// FOLDIN_MAX_BATCH rows, staged as fold-in stages a batch (the same pitch, contiguous loads instead of indexed ones), and
// one 256-thread workgroup forms its lower-triangle 16 x 16 tiles with v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64
// (fold_gram_batch). The reduce kernel sums the slabs' tiles per element in ascending slab order -- fp32 in double,
// rounded once -- and writes the dense symmetric KP x KP matrix (the upper triangle mirrors the lower, padding is zero
// because the padded columns of the table are). No atomics, no dependence on the grid or the device: G is bitwise
// repeatable.
//
// Implicit solve: als_fold_in_kernel's launch contract (one 256-thread workgroup owns one whole query, grid-stride, every
// sum in one fixed order, no atomics) and its body, with these differences:
//   Gram   : tile (I, J) accumulates mfma(w y[I], y[J]) with w_e = alpha r_e -- a second operand register set, one
//            multiply per feature block and MFMA step. Only the lower triangle is read afterwards, so the diagonal tiles
//            need not be bitwise symmetric.
//   RHS    : sum (1 + w_e) y_e over the entries with r_e > 0, thread f owns feature f, entries in order.
//   system : when the tiles are in LDS every thread adds the matching elements of G from global memory, then lambda goes
//            on the k true diagonal entries; Jacobi scaling, register Cholesky and substitution as in fold-in.
//   refine : (fp64) residual sum_e y_e [(r_e > 0)(1 + w_e) - w_e (y_e . x)] - G x - lambda x.
//   order  : the loop walks a host-made permutation, longest query first; a query's bits do not depend on it.
// DESIGN.md section 3.10 has the model, the resource figures and the measurements.
#include <climits>
#include <type_traits>

#include "als_device.h"

namespace cfk {
namespace {

#include "als_fold_tiles.h"

// ---- table Gram ------------------------------------------------------------------------------------------------------

// fold_load for rows that lie one after another: entry e of the batch is row e of `rows`. No ratings.
template <class T, int KP>
__device__ __forceinline__ void gram_load(FoldBatch<T, KP>& f, const T* __restrict__ rows, int nb, int tid) {
    typedef FoldBatch<T, KP> B;
    static_for<0, B::NV>([&](auto vc) {
        constexpr int vv = decltype(vc)::value;
        const int x = tid + FOLDIN_THREADS * vv, e = x / B::CPR, c = x - e * B::CPR;
        typename B::V val = {};
        if (e < nb) val = *(const typename B::V*)(rows + (int64_t)e * KP + c * B::VN);
        f.v[vv] = val;
    });
    f.r = T(0);
}

// The tiles of wave W from their accumulators into the slab's partial tiles [NT][16][16] (C/D maps as fold_store_tiles).
template <class T, int KP, int W, int MT>
__device__ __forceinline__ void gram_store_partial(const typename FoldAcc<T>::type (&acc)[MT], T* __restrict__ part,
                                                   int lane) {
    constexpr int NT = foldin_tiles(KP);
    constexpr bool F64 = std::is_same<T, double>::value;
    const int g = lane >> 4, c = lane & 15;
    static_for<0, NT>([&](auto t) {
        constexpr int tt = decltype(t)::value;
        if constexpr (tt % 4 == W) {
            static_for<0, 4>([&](auto r) {
                constexpr int rr = decltype(r)::value;
                const int row = F64 ? g + 4 * rr : 4 * g + rr;
                part[tt * 256 + row * 16 + c] = acc[tt / 4][rr];
            });
        }
    });
}

template <class T, int KP>
__global__ __launch_bounds__(FOLDIN_THREADS) void als_gram_table_kernel(const T* __restrict__ table, int64_t n_rows,
                                                                       int64_t rows_per_slab, T* __restrict__ partial) {
    constexpr int NT = foldin_tiles(KP), MT = (NT + 3) / 4, P = foldin_pitch(KP), batch = FOLDIN_MAX_BATCH;
    typedef typename FoldAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    T* stage = (T*)gsm;          // [batch][P]
    T* tb = stage + batch * P;   // [batch] fold_store's rating slot (zeros)
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    const int64_t lo = (int64_t)blockIdx.x * rows_per_slab;
    const int n = (int)max((int64_t)0, min(rows_per_slab, n_rows - lo));
    const T* rows = table + lo * KP;

    Acc acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = Acc{};
    FoldBatch<T, KP> fb;
    gram_load<T, KP>(fb, rows, min(batch, n), tid);
    for (int base = 0; base < n; base += batch) {
        const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
        fold_store<T, KP>(fb, stage, tb, nb4, tid);
        __syncthreads();
        if (base + batch < n)   // the next batch's rows travel while this one is multiplied
            gram_load<T, KP>(fb, rows + (int64_t)(base + batch) * KP, min(batch, n - base - batch), tid);
        FOLD_BY_WAVE(wave, fold_gram_batch, acc, stage, nb4 >> 2, lane)
        __syncthreads();
    }
    FOLD_BY_WAVE(wave, gram_store_partial, acc, partial + (int64_t)blockIdx.x * (NT * 256), lane)
}

// gram[i][j] = sum over the slabs, in ascending order, of element (max(i, j), min(i, j)) of their triangles.
template <class T>
__global__ __launch_bounds__(256) void als_gram_reduce_kernel(const T* __restrict__ partial, int64_t slabs, int kp,
                                                              T* __restrict__ gram) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= kp * kp) return;
    const int r = x / kp, c = x - r * kp;
    const int i = max(r, c), j = min(r, c);
    const int I = i >> 4, J = j >> 4, C = kp >> 4;
    const int64_t slab_elems = (int64_t)(C * (C + 1) / 2) * 256;
    const T* p = partial + (I * (I + 1) / 2 + J) * 256 + (i & 15) * 16 + (j & 15);
    double s = 0.0;
    for (int64_t t = 0; t < slabs; ++t) s += (double)p[t * slab_elems];
    gram[x] = (T)s;
}

// ---- implicit solve --------------------------------------------------------------------------------------------------

// fold_gram_batch with a per-entry weight: tile (I, J) += (w y[I])^T y[J], w_e = alpha tb[e] (tb: the batch's ratings;
// lane (g, c) of step s holds entry 4 s + g, so one weight per lane and step).
template <class T, int KP, int W, int MT>
__device__ __forceinline__ void implicit_gram_batch(typename FoldAcc<T>::type (&acc)[MT], const T* __restrict__ stage,
                                                    const T* __restrict__ tb, T alpha, int nsteps, int lane) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), P = foldin_pitch(KP);
    const T* p = stage + (lane >> 4) * P + (lane & 15);
    const T* wr = tb + (lane >> 4);
    for (int s = 0; s < nsteps; ++s, p += 4 * P, wr += 4) {
        T op[C], wop[C];
        const T w = alpha * wr[0];
        static_for<0, C>([&](auto b) {
            op[b] = p[16 * b];
            wop[b] = w * op[b];
        });
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            if constexpr (tt % 4 == W) {
                constexpr int I = fold_tile_row(tt), J = fold_tile_col(tt);
                acc[tt / 4] = fold_mfma(wop[I], op[J], acc[tt / 4]);
            }
        });
    }
}

template <class T, int KP>
__global__ __launch_bounds__(FOLDIN_THREADS) void als_implicit_kernel(ImplicitArgs ia, int batch) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), MT = (NT + 3) / 4, P = foldin_pitch(KP);
    constexpr bool REFINE = std::is_same<T, double>::value;
    typedef typename FoldAcc<T>::type Acc;
    extern __shared__ __attribute__((aligned(16))) unsigned char ism[];
    T* G = (T*)ism;                               // [NT][16][FOLDIN_TILE_PITCH]
    T* stage = G + NT * FOLDIN_TILE_ELEMS;        // [batch][P]
    T* scl = stage + batch * P;                   // [KP] Jacobi scale 1 / sqrt(a_ii)
    T* dg = scl + KP;                             // [KP] diagonal of L
    T* bc = dg + KP;                              // [KP] substitution: the component being broadcast
    T* xs = bc + KP;                              // [KP] solution (refinement)
    T* tb = xs + KP;                              // [batch] ratings, then per-entry residuals
    const FoldinArgs& a = ia.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = uni(tid >> 6);
    const int ke = a.k;
    const T* opp = (const T*)a.opp;
    const T* Gt = (const T*)ia.gram;
    const T alpha = (T)ia.alpha, lam = (T)a.lambda;

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

    for (int64_t qi = blockIdx.x; qi < a.n_queries; qi += gridDim.x) {
        const int64_t q = ia.order[qi];
        const int64_t lo = a.q_ptr[q];
        const int n = (int)(a.q_ptr[q + 1] - lo);
        T* out = (T*)a.out + q * KP;
        T* dst = a.dst_rows ? (T*)a.self + a.dst_rows[q] * KP : nullptr;
        if (n == 0) {   // b = 0: the zero vector, written directly. Workgroup-uniform.
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
                for (int e = 0; e < nb; ++e) {
                    const T r = tb[e];
                    if (r > T(0)) rhs += (T(1) + alpha * r) * stage[e * P + tid];
                }
            FOLD_BY_WAVE(wave, implicit_gram_batch, acc, stage, tb, alpha, nb4 >> 2, lane)
            __syncthreads();
        }
        FOLD_BY_WAVE(wave, fold_store_tiles, acc, G, lane)
        __syncthreads();

        // + G: thread (ty, tx) owns element (ty, tx) of every tile, here as in the factorisation below
        const int ty = tid >> 4, tx = tid & 15;
        const int own = ty * FOLDIN_TILE_PITCH + tx;
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            G[tt * FOLDIN_TILE_ELEMS + own] += Gt[(16 * fold_tile_row(tt) + ty) * KP + 16 * fold_tile_col(tt) + tx];
        });
        __syncthreads();
        // + lambda I on the true features, then D^-1/2 A D^-1/2
        if (tid < KP) {
            T s = T(1);
            if (tid < ke) {
                const T d = G[fold_at(tid, tid)] + lam;
                G[fold_at(tid, tid)] = d;
                s = T(1) / sqrt(d);
            }
            scl[tid] = s;
        }
        __syncthreads();
        // Right-looking Cholesky in registers, exactly als_fold_in_kernel's: column j = 16 J + jj is published unscaled
        // through LDS (two buffers in turn, one barrier per column), every thread scales the entries of its rows and
        // columns by 1 / sqrt(pivot) itself, the owners keep theirs as L, the trailing tiles take the rank-1 update.
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
            // b - A x = sum_e y_e [(r_e > 0)(1 + w_e) - w_e (y_e . x)] - G x - lambda x (the triangle now holds L;
            // G is symmetric, so row tid of G x reads column tid: consecutive threads, consecutive addresses)
            if (tid < KP) xs[tid] = x;
            __syncthreads();
            T res = -lam * x;
            if (tid < KP)
                for (int j = 0; j < ke; ++j) res -= Gt[j * KP + tid] * xs[j];
            for (int base = 0; base < n; base += batch) {
                const int nb = min(batch, n - base), nb4 = (nb + 3) & ~3;
                fold_load<T, KP>(fb, opp, idx + base, rat + base, nb, tid);
                fold_store<T, KP>(fb, stage, tb, nb4, tid);
                __syncthreads();
                for (int e = wave; e < nb; e += 4) {   // t_e = (r_e > 0)(1 + w_e) - w_e (y_e . x), one wave per entry
                    T d = T(0);
                    for (int f = lane; f < KP; f += 64) d += stage[e * P + f] * xs[f];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
                    if (lane == 0) {
                        const T r = tb[e], w = alpha * r;
                        tb[e] = (r > T(0) ? T(1) + w : T(0)) - w * d;
                    }
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
hipError_t launch_gram_one(const T* table, int64_t n_rows, const GramTablePlan& plan, T* partial, T* gram, hipStream_t s) {
    // fp64 at the widest strides stages more than the 64 KiB a kernel gets by default; the bound is the same on every call
    hipError_t e = hipFuncSetAttribute((const void*)als_gram_table_kernel<T, KP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)plan.lds_bytes);
    if (e != hipSuccess) return e;
    als_gram_table_kernel<T, KP><<<(unsigned)plan.slabs, FOLDIN_THREADS, (size_t)plan.lds_bytes, s>>>(
        table, n_rows, plan.rows_per_slab, partial);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    als_gram_reduce_kernel<T><<<(unsigned)((KP * KP + 255) / 256), 256, 0, s>>>(partial, plan.slabs, KP, gram);
    return hipGetLastError();
}

template <class T, int KP>
hipError_t launch_implicit_one(const ImplicitArgs& a, const FoldinPlan& plan, hipStream_t s) {
    // as launch_fold_in: the same bound per instantiation on every call
    hipError_t e = hipFuncSetAttribute((const void*)als_implicit_kernel<T, KP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)plan.lds_bytes);
    if (e != hipSuccess) return e;
    als_implicit_kernel<T, KP><<<(unsigned)plan.grid, FOLDIN_THREADS, (size_t)plan.lds_bytes, s>>>(a, plan.batch);
    return hipGetLastError();
}

// The instantiations are fold-in's: 16, 32, 64, 128, and in fp64 also 80, 96, 112 (the generic solve path's strides).
#define IMPLICIT_BY_KP(T, kp, FN, ...)                                  \
    switch (kp) {                                                       \
        case 16: return FN<T, 16>(__VA_ARGS__);                         \
        case 32: return FN<T, 32>(__VA_ARGS__);                         \
        case 64: return FN<T, 64>(__VA_ARGS__);                         \
        case 128: return FN<T, 128>(__VA_ARGS__);                       \
        default: break;                                                 \
    }                                                                   \
    if constexpr (std::is_same<T, double>::value) {                     \
        switch (kp) {                                                   \
            case 80: return FN<T, 80>(__VA_ARGS__);                     \
            case 96: return FN<T, 96>(__VA_ARGS__);                     \
            case 112: return FN<T, 112>(__VA_ARGS__);                   \
            default: break;                                             \
        }                                                               \
    }                                                                   \
    return hipErrorInvalidValue;

template <class T>
hipError_t gram_kp(int kp, const void* table, int64_t n_rows, const GramTablePlan& plan, void* partial, void* gram,
                   hipStream_t s) {
    IMPLICIT_BY_KP(T, kp, launch_gram_one, (const T*)table, n_rows, plan, (T*)partial, (T*)gram, s)
}
template <class T>
hipError_t implicit_kp(int kp, const ImplicitArgs& a, const FoldinPlan& plan, hipStream_t s) {
    IMPLICIT_BY_KP(T, kp, launch_implicit_one, a, plan, s)
}

}  // namespace

hipError_t launch_gram_table(int precision, int kp, const void* table, int64_t n_rows, const GramTablePlan& plan,
                             void* partial, void* gram, hipStream_t s) {
    const int elem = precision == 0 ? 4 : 8;
    const GramTablePlan want = gram_table_plan(kp, elem, n_rows, 0);
    if (kp > FOLDIN_MAX_KP || n_rows < 0 || !table || !partial || !gram || plan.threads != FOLDIN_THREADS ||
        plan.slabs != want.slabs || plan.rows_per_slab != want.rows_per_slab || plan.lds_bytes != want.lds_bytes ||
        plan.slabs > GRAM_TABLE_MAX_SLABS || plan.lds_bytes > FOLDIN_LDS_LIMIT)
        return hipErrorInvalidValue;
    return precision == 0 ? gram_kp<float>(kp, table, n_rows, plan, partial, gram, s)
                          : gram_kp<double>(kp, table, n_rows, plan, partial, gram, s);
}

hipError_t launch_implicit(int precision, int kp, const ImplicitArgs& a, const FoldinPlan& plan, hipStream_t s) {
    if (a.f.n_queries <= 0) return hipSuccess;
    const int elem = precision == 0 ? 4 : 8;
    if (kp > FOLDIN_MAX_KP || a.f.k < 1 || a.f.k > kp || !a.gram || !a.order || plan.threads != FOLDIN_THREADS ||
        plan.grid < 1 || plan.grid > a.f.n_queries || plan.grid > INT32_MAX || plan.batch < 4 || plan.batch % 4 != 0 ||
        plan.batch > FOLDIN_MAX_BATCH || plan.lds_bytes != foldin_lds_bytes(kp, elem, plan.batch) ||
        plan.lds_bytes > FOLDIN_LDS_LIMIT)
        return hipErrorInvalidValue;
    return precision == 0 ? implicit_kp<float>(kp, a, plan, s) : implicit_kp<double>(kp, a, plan, s);
}

}  // namespace cfk
