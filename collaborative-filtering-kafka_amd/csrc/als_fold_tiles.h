// Private to als_foldin.hip and als_implicit.hip: what a 256-thread workgroup needs to form lower-triangle 16 x 16 MFMA
// Gram tiles of staged rows at full input precision -- the accumulator types, the tile maps, the per-wave batch product
// and tile store, and the two-half batch staging (FoldBatch / fold_load / fold_store). The layout is described in
// als_fold_solve.h and in DESIGN.md section 3.9. Include inside namespace cfk { namespace {.
#pragma once

typedef double f64x4 __attribute__((ext_vector_type(4)));

template <class T> struct FoldAcc;
template <> struct FoldAcc<float> { typedef f32x4 type; };
template <> struct FoldAcc<double> { typedef f64x4 type; };

__device__ __forceinline__ f32x4 fold_mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f64x4 fold_mfma(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// Lower-triangle tile t = I (I + 1) / 2 + J, J <= I.
constexpr int fold_tile_row(int t) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    return i;
}
constexpr int fold_tile_col(int t) { return t - fold_tile_row(t) * (fold_tile_row(t) + 1) / 2; }
// Element (i, j), j <= i, of the tiled triangle.
__device__ __forceinline__ int fold_at(int i, int j) {
    const int I = i >> 4, J = j >> 4;
    return (I * (I + 1) / 2 + J) * FOLDIN_TILE_ELEMS + (i & 15) * FOLDIN_TILE_PITCH + (j & 15);
}

// One batch of staged rows into the tiles of wave W: nsteps MFMA steps of 4 entries.
template <class T, int KP, int W, int MT>
__device__ __forceinline__ void fold_gram_batch(typename FoldAcc<T>::type (&acc)[MT], const T* __restrict__ stage,
                                                int nsteps, int lane) {
    constexpr int C = KP / 16, NT = foldin_tiles(KP), P = foldin_pitch(KP);
    const T* p = stage + (lane >> 4) * P + (lane & 15);
    for (int s = 0; s < nsteps; ++s, p += 4 * P) {
        T op[C];
        static_for<0, C>([&](auto b) { op[b] = p[16 * b]; });
        static_for<0, NT>([&](auto t) {
            constexpr int tt = decltype(t)::value;
            if constexpr (tt % 4 == W) {
                constexpr int I = fold_tile_row(tt), J = fold_tile_col(tt);
                acc[tt / 4] = fold_mfma(op[I], op[J], acc[tt / 4]);
            }
        });
    }
}

// The tiles of wave W from their accumulators into a tiled triangle [NT][16][PITCH]: the LDS triangle of the solve
// (FOLDIN_TILE_PITCH) or a slab's dense partial tiles of the table Gram (16). C/D map of the f32 form: column = lane & 15,
// row = 4 (lane >> 4) + r; of the f64 form: row = (lane >> 4) + 4 r.
template <int PITCH> using FoldTilePitch = std::integral_constant<int, PITCH>;
template <class T, int KP, int W, int MT, int PITCH>
__device__ __forceinline__ void fold_store_tiles(const typename FoldAcc<T>::type (&acc)[MT], T* __restrict__ G, int lane,
                                                 FoldTilePitch<PITCH>) {
    constexpr int NT = foldin_tiles(KP);
    constexpr bool F64 = std::is_same<T, double>::value;
    const int g = lane >> 4, c = lane & 15;
    static_for<0, NT>([&](auto t) {
        constexpr int tt = decltype(t)::value;
        if constexpr (tt % 4 == W) {
            static_for<0, 4>([&](auto r) {
                constexpr int rr = decltype(r)::value;
                const int row = F64 ? g + 4 * rr : 4 * g + rr;
                G[tt * (16 * PITCH) + row * PITCH + c] = acc[tt / 4][rr];
            });
        }
    });
}

// The wave's own instantiation of a per-wave step (the tiles of wave W are a compile-time set): a plain switch, so
// every call is inlined and the accumulators stay in registers.
#define FOLD_BY_WAVE(wave, FN, ...)                  \
    switch (wave) {                                  \
        case 0: FN<T, KP, 0, MT>(__VA_ARGS__); break; \
        case 1: FN<T, KP, 1, MT>(__VA_ARGS__); break; \
        case 2: FN<T, KP, 2, MT>(__VA_ARGS__); break; \
        default: FN<T, KP, 3, MT>(__VA_ARGS__); break; \
    }

// A batch of nb <= FOLDIN_MAX_BATCH opposite rows (and their ratings) of a query, in two halves so that the loads of the
// next batch are in flight while the Gram of this one runs: fold_load brings this thread's 16-byte pieces (piece x = tid +
// 256 v is columns [VN c, VN c + VN) of entry e, x = e CPR + c) and its rating into registers, fold_store puts them into
// the staging area; rows [nb, nb4) are zero-filled.
template <class T, int KP>
struct FoldBatch {
    typedef typename Vec16<T>::type V;
    static constexpr int VN = Vec16<T>::N, CPR = KP / VN, NV = FOLDIN_MAX_BATCH * CPR / FOLDIN_THREADS;
    static_assert(NV >= 1 && NV * FOLDIN_THREADS == FOLDIN_MAX_BATCH * CPR, "a batch is whole pieces per thread");
    V v[NV];
    T r;
};
template <class T, int KP>
__device__ __forceinline__ void fold_load(FoldBatch<T, KP>& f, const T* __restrict__ opp, const int32_t* __restrict__ idx,
                                          const int16_t* __restrict__ rat, int nb, int tid) {
    typedef FoldBatch<T, KP> B;
    static_for<0, B::NV>([&](auto vc) {
        constexpr int vv = decltype(vc)::value;
        const int x = tid + FOLDIN_THREADS * vv, e = x / B::CPR, c = x - e * B::CPR;
        typename B::V val = {};
        if (e < nb) val = *(const typename B::V*)(opp + (int64_t)idx[e] * KP + c * B::VN);
        f.v[vv] = val;
    });
    f.r = tid < nb ? (T)rat[tid] : T(0);
}
template <class T, int KP>
__device__ __forceinline__ void fold_store(const FoldBatch<T, KP>& f, T* __restrict__ stage, T* __restrict__ tb, int nb4,
                                           int tid) {
    typedef FoldBatch<T, KP> B;
    constexpr int P = foldin_pitch(KP);
    static_for<0, B::NV>([&](auto vc) {
        constexpr int vv = decltype(vc)::value;
        const int x = tid + FOLDIN_THREADS * vv, e = x / B::CPR, c = x - e * B::CPR;
        if (e < nb4) *(typename B::V*)(stage + e * P + c * B::VN) = f.v[vv];
    });
    if (tid < nb4) tb[tid] = f.r;
}
