// Private part of als_kernels.hip: the VALU path's solve -- the per-wave LDS carve-up and the in-wave Cholesky on
// a packed lower triangle (lane j = row j), fp32 and fp64.
#pragma once

#include "als_device.h"

namespace cfk {
namespace {

// ---------------------------------------------------------------------------------------------------
// Per-wave LDS carve-up
// ---------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int round16(int b) { return (b + 15) & ~15; }

template <class T, int KP, Path P>
struct WaveLds {
    static constexpr int G_BYTES = round16(KP * (KP + 1) / 2 * (int)sizeof(T));   // packed lower triangle
    static constexpr int STAGE_BYTES = (P == Path::VALU) ? round16(RSTAGE * KP * (int)sizeof(T)) : 0;
    static constexpr int MAIN_BYTES = G_BYTES > STAGE_BYTES ? G_BYTES : STAGE_BYTES;   // staging aliases G
    static constexpr int RHS_OFF = MAIN_BYTES;
    static constexpr int BC_OFF = RHS_OFF + round16(KP * (int)sizeof(T));
    static constexpr int SIDX_OFF = BC_OFF + round16(KP * (int)sizeof(T));
    static constexpr int SRAT_OFF = SIDX_OFF + ((P == Path::VALU) ? round16(RSTAGE * 4) : 0);
    static constexpr int BYTES = SRAT_OFF + ((P == Path::VALU) ? round16(RSTAGE * (int)sizeof(T)) : 0);
};

// ---------------------------------------------------------------------------------------------------
// In-wave Cholesky solve (lane j = row j), shared by both paths
// ---------------------------------------------------------------------------------------------------
// packed lower-triangular index (c <= r)
__host__ __device__ constexpr int tri(int r, int c) { return r * (r + 1) / 2 + c; }

// Pivot of one Cholesky step: d = sqrt(a), dinv = 1/sqrt(a). fp32 uses v_rsq_f32 (1 ulp; the fp32 fast mode
// is held to an MSE bound), fp64 keeps correctly rounded sqrt and division for the 1e-6 parity mode.
__device__ __forceinline__ void pivot(float a, float& d, float& dinv) {
    dinv = __builtin_amdgcn_rsqf(a);
    d = a * dinv;
}
__device__ __forceinline__ void pivot(double a, double& d, double& dinv) {
    d = sqrt(a);
    dinv = 1.0 / d;
}

// Lane j owns row j of A and computes row j of L. A lane never needs an entry right of its diagonal
// (i > j): those registers may hold anything finite, which makes the solve nearly select-free -- every
// step runs the same instructions on all lanes; only the per-step uniform results (1/L[p][p], the forward
// and backward solution components) are dropped into lane p with one compare + select; the row load and
// the transposition are unpredicated LDS accesses.
template <class T, int KP>
__device__ __forceinline__ void solve_store(T* P, const T* rhs_l, T* bc, const Task& tk, const SolveArgs& a,
                                            int lane) {
    using BV = typename Vec16<T>::type;
    constexpr int BN = Vec16<T>::N;
    static_assert(KP <= 64, "one row per lane");
    const int j = lane;
    const bool act = j < KP;
    const int jr = act ? j : KP - 1;
    T* out = (T*)a.out + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)KP;

    if (tk.ndeg == 0) {   // cannot occur in the reference (entities exist only once rated); defined as 0
        if (act) out[j] = T(0);
        return;
    }

    // A + lambda * (n * I) on the packed diagonal: fp32 mirrors add(A, lambda, n*I)
    // (MFeatureCalculator.java:91-95) -> A[j][j] + lambda*(float)n; padded features get an identity row.
    const T reg = (T)a.lambda * (T)tk.ndeg;
    const int rowbase = tri(jr, 0);
    if (act) {
        const T dd = P[rowbase + jr];
        P[rowbase + jr] = (j < a.k) ? dd + reg : T(1);
    }
    wave_sync();
    // Row j, entries 0..KP-1 read straight through the packed triangle: entries i > j land in the next
    // rows' storage (finite, never used). rowbase + i <= tri(KP-1, 0) + KP-1: always in bounds.
    T av[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) av[i] = P[rowbase + i];
    T y = act ? rhs_l[jr] : T(0);

    T dinv = T(0), z = T(0);     // lane p: 1/L[p][p] and the forward solution z_p
    T rs_cur, l;
    {
        T d;
        pivot(bcast(av[0], 0), d, rs_cur);
        l = av[0] * rs_cur;       // lane 0 gets ~L[0][0]; lanes > 0 L[j][0]
        av[0] = l;
    }
    static_for<0, KP>([&](auto P_) {
        constexpr int p = decltype(P_)::value;
        // forward substitution with column p: z_p = y_p / L[p][p]; y_j -= L[j][p] z_p (lanes > p; lane p
        // and lanes < p update registers they no longer need)
        const T zp = bcast(y, p) * rs_cur;
        const bool me = opaque(j) == p;
        z = me ? zp : z;
        dinv = me ? rs_cur : dinv;
        y -= l * zp;
        // look-ahead columns p+1, p+2 through v_readlane: the next pivots never wait on LDS
        if constexpr (p + 1 < KP) av[p + 1] -= bcast(l, p + 1) * l;
        if constexpr (p + 2 < KP) av[p + 2] -= bcast(l, p + 2) * l;
        // next pivot (p+1): lane p+1 gets ~L[p+1][p+1], lanes > p+1 L[j][p+1]
        T l_next = T(0), rs_next = T(0);
        if constexpr (p + 1 < KP) {
            T d;
            pivot(bcast(av[p + 1], p + 1), d, rs_next);
            l_next = av[p + 1] * rs_next;
            av[p + 1] = l_next;
        }
        // bulk trailing update of columns >= p+3: L[i][p] broadcast through LDS, 16 B per read,
        // double-buffered so that reads of the next chunk are in flight under this chunk's FMAs
        if constexpr (p + 3 < KP) {
            wave_sync();
            if (act) bc[j] = l;
            wave_sync();
            constexpr int CH = 4;                              // 16-B vectors per chunk
            constexpr int q0 = ((p + 3) / BN) * BN;
            constexpr int nvec = (KP - q0) / BN;
            constexpr int nch = (nvec + CH - 1) / CH;
            BV buf[2][CH];
            static_for<0, (CH < nvec ? CH : nvec)>([&](auto V_) {
                constexpr int v = decltype(V_)::value;
                buf[0][v] = *(const BV*)(bc + q0 + v * BN);
            });
            static_for<0, nch>([&](auto C_) {
                constexpr int c = decltype(C_)::value;
                if constexpr (c + 1 < nch) {
                    static_for<0, CH>([&](auto V_) {
                        constexpr int v = decltype(V_)::value;
                        if constexpr ((c + 1) * CH + v < nvec)
                            buf[(c + 1) & 1][v] = *(const BV*)(bc + q0 + ((c + 1) * CH + v) * BN);
                    });
                }
                static_for<0, CH>([&](auto V_) {
                    constexpr int v = decltype(V_)::value;
                    if constexpr (c * CH + v < nvec) {
                        static_for<0, BN>([&](auto E_) {
                            constexpr int e = decltype(E_)::value;
                            constexpr int i = q0 + (c * CH + v) * BN + e;
                            if constexpr (i >= p + 3) av[i] -= buf[c & 1][v][e] * l;
                        });
                    }
                });
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        static_for<p + 1, KP>([&](auto I_) { pin(av[decltype(I_)::value]); });
        l = l_next;
        rs_cur = rs_next;
        __builtin_amdgcn_sched_barrier(0);
    });
    // Transpose L through the packed triangle: lane j writes its row into ITS OWN segment only -- the
    // right-of-diagonal (garbage) entries i > j go to min(i, j) = the lane's diagonal slot, written before
    // the valid diagonal (descending i; same address, so program order holds). Then lane j reads column j.
    wave_sync();
    if (act) {
#pragma unroll
        for (int i = KP - 1; i >= 0; --i) P[rowbase + min(i, jr)] = av[i];
    }
    wave_sync();
#pragma unroll
    for (int i = 0; i < KP; ++i) av[i] = P[tri(i, 0) + jr];   // = L[i][j] for i >= j; garbage above
    // Backward substitution L^T x = z (column-oriented, p descending): x_p = z'_p / L[p][p],
    // z'_j -= L[p][j] x_p for j < p.
    T x = T(0);
#pragma unroll
    for (int p = KP - 1; p >= 0; --p) {
        const T xp = bcast(z, p) * bcast(dinv, p);
        x = (opaque(j) == p) ? xp : x;
        z -= av[p] * xp;
    }
    if (act) out[j] = (j < a.k) ? x : T(0);
}

}  // namespace
}  // namespace cfk
