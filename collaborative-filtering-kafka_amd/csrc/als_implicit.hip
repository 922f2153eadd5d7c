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
// Implicit solve: als_fold_solve_kernel<T, KP, ImplicitArgs> of als_fold_solve.h, the kernel fold-in runs, which takes
// the model's side at each of its five `if constexpr (IMPLICIT)` sites.
// DESIGN.md section 3.10 has the model, the resource figures and the measurements.
#include <climits>
#include <type_traits>

#include "als_device.h"

namespace cfk {
namespace {

#include "als_fold_tiles.h"
#include "als_fold_solve.h"   // als_fold_solve_kernel, fold_by_kp, fold_plan_ok, launch_fold_solve

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
    // the slab's partial tiles [NT][16][16]
    FOLD_BY_WAVE(wave, fold_store_tiles, acc, partial + (int64_t)blockIdx.x * (NT * 256), lane, FoldTilePitch<16>{})
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

template <class T>
hipError_t gram_kp(int kp, const void* table, int64_t n_rows, const GramTablePlan& plan, void* partial, void* gram,
                   hipStream_t s) {
    return fold_by_kp<T>(kp, [&](auto kpc) {
        return launch_gram_one<T, decltype(kpc)::value>((const T*)table, n_rows, plan, (T*)partial, (T*)gram, s);
    });
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
    if (!a.gram || !a.order || !fold_plan_ok(precision, kp, a.f, plan)) return hipErrorInvalidValue;
    return precision == 0 ? launch_fold_solve<float>(kp, a, plan, s) : launch_fold_solve<double>(kp, a, plan, s);
}

}  // namespace cfk
