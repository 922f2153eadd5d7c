// Private part of als_kernels.hip: the MFMA paths' solve -- cross-lane moves on the 4 x 16 lane grid, the sweep
// operator on one tile, the tile stores, and the block LDL^T solve with refinement on the accumulator tiles.
#pragma once

#include "als_mfma.h"

namespace cfk {
namespace {

// ---------------------------------------------------------------------------------------------------
// Cross-lane moves on the 4 x 16 lane grid (row g = lane >> 4, column c = lane & 15), VALU-only (no LDS)
// ---------------------------------------------------------------------------------------------------
// value of lane (g, L) at every lane of row g (DPP row_newbcast)
template <int L>
__device__ __forceinline__ float row_lane_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x150 + L, 0xf, 0xf, false));
}
// value of lane (G, c) at every lane (g, c): one ds_bpermute through the LDS crossbar (no LDS storage).
// Measured 3-5% faster on the solve-heavy user half than the v_permlane16/32_swap pair it replaced (the
// swaps clobber both operands, which cost register copies and hazard NOPs on every sweep step).
template <int G>
__device__ __forceinline__ float col_bcast(float v) {
    const int addr = ((int)(__lane_id() & 15) + 16 * G) * 4;
    return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v)));
}

// sum over the 4 rows at each column, result in every row
__device__ __forceinline__ float col_sum(float v) {
    const int x = __float_as_int(v);
    const auto s16 = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    const float y = __int_as_float((int)s16[0]) + __int_as_float((int)s16[1]);
    const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_int(y), __float_as_int(y), false, false);
    return __int_as_float((int)s32[0]) + __int_as_float((int)s32[1]);
}
// inclusive row_shr scan: lane (g, 15) ends with the sum over row g
__device__ __forceinline__ float row_sum_to_last(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));
    return v;
}

// Sweep operator (Goodnight) over all 16 pivots of one 16 x 16 tile in MFMA accumulator layout
// (lane (g, c), register r holds a[4g + r][c]): in place a -> -a^{-1}. Step p:
//   a[i][j] -= a[i][p] a[p][j] / d,  a[i][p] = a[i][p] / d,  a[p][j] = a[p][j] / d,  a[p][p] = -1 / d.
// Column p reaches each row by DPP row_newbcast, row p each column by two permlane swaps. The pivot row /
// column rules fold into the same four FMAs by offsetting a[p][p] by -1 in the broadcast operands:
// a[i][p] + a[i][p] (d - 1)(-1/d) = a[i][p] / d. That FMA is accurate to a few ulp only while d <= 1,
// which the caller guarantees by Jacobi-scaling the system to a unit diagonal (every later pivot is a
// Schur-complement diagonal of a unit-diagonal SPD matrix, so it stays in (0, 1]).
// The four row broadcasts are fused into the FMAs (v_fmac_f32_dpp row_newbcast, one instruction per register
// instead of a v_mov_b32_dpp + v_fmac_f32 pair; k = 64 / 128 user half -3 %, profiles/r05e/e18_*.log).
// A DPP read of a VGPR needs 2 wait states after a VALU write of it, and the compiler's hazard recognizer does not
// see VALU writes inside inline asm: the block waits 2 states before its first DPP read (the previous step's writes)
// and after its last write (a compiler-placed DPP or lane op reading the results next).
template <int L>
__device__ __forceinline__ void fmac_rowbcast4(f32x4& a, float t) {
    float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    asm("s_nop 1\n\t"
        "v_fmac_f32_dpp %0, %0, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %1, %1, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %2, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        "v_fmac_f32_dpp %3, %3, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
        : "v"(t), "i"(L));
    a[0] = a0;
    a[1] = a1;
    a[2] = a2;
    a[3] = a3;
}
// lane L ? x : v with the lane mask a scalar constant (s_mov): the compiler's select re-derived the mask by a
// v_cmp at every pivot step (one vector instruction, and a 2-state hazard before the v_cndmask reading it).
// AFTER_DPP: ends with the 2 wait states a following DPP read of the result needs (see fmac_rowbcast4).
template <int L, bool AFTER_DPP>
__device__ __forceinline__ float select_lane(float v, float x) {
    float r;
    if constexpr (AFTER_DPP)
        asm("v_cndmask_b32_e64 %0, %1, %2, %3\n\ts_nop 1" : "=v"(r) : "v"(v), "v"(x), "s"((uint64_t)1 << L));
    else
        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(x), "s"((uint64_t)1 << L));
    return r;
}
template <int p>
__device__ __forceinline__ void sweep_step(f32x4& a, int lane, float& nrd_min) {
    constexpr int pg = p >> 2, pr = p & 3;
    const float nrd = __builtin_amdgcn_rcpf(-bcast(a[pr], 16 * pg + p));   // -1 / d
    nrd_min = fminf(nrd_min, nrd);                                          // -1 / (smallest pivot)
    // the pivot lane's d - 1 (read next by v_readlane / ds_bpermute / the DPP block, which waits its own 2 states)
    a[pr] = select_lane<16 * pg + p, false>(a[pr], a[pr] - 1.f);
    const float t = col_bcast<pg>(a[pr]) * nrd;   // a[p][c] (d - 1 at c = p) * (-1/d)
    fmac_rowbcast4<p>(a, t);                       // a[4g + r][c] += a[4g + r][p] t[c]
    a[pr] = select_lane<16 * pg + p, true>(a[pr], nrd);
    (void)lane;
}
__device__ __forceinline__ void sweep_tile(f32x4& a, int lane, float& nrd_min) {
    static_for<0, 16>([&](auto P_) { sweep_step<decltype(P_)::value>(a, lane, nrd_min); });
}

// D + X^T Y of two 16 x 16 tiles in accumulator layout (the solve's block products): four v_mfma_f32_16x16x4_f32
// (exact fp32 products, 128 MFMA cycles)
__device__ __forceinline__ f32x4 tile_tn(const f32x4& X, const f32x4& Y, f32x4 D) {
#pragma unroll
    for (int s = 0; s < 4; ++s) D = __builtin_amdgcn_mfma_f32_16x16x4f32(X[s], Y[s], D, 0, 0, 0);
    return D;
}

// Lookahead schedule of the block factorisation: step P first finishes block column P + 1
// (V'_{P,P+1} and the update of T_{P+1,P+1}), so the 16-step sweep of T_{P+1,P+1} -- a dependent chain of
// broadcasts, latency-bound -- can start at once, and the rest of step P's MFMA work (block columns J >= P + 2) is
// issued between its steps. Items of step P, J descending, per J: V'_PJ = S_P T_PJ, then T_IJ += T_PI^T V'_PJ for
// I = P + 1 .. J (the same single update per tile as the plain order: bitwise equal results).
__host__ __device__ constexpr int la_items(int C, int P) {
    int n = 0;
    for (int J = C - 1; J >= P + 2; --J) n += 1 + (J - P);
    return n;
}
__host__ __device__ constexpr int la_item_J(int C, int P, int t) {
    for (int J = C - 1; J >= P + 2; --J) {
        if (t < 1 + J - P) return J;
        t -= 1 + J - P;
    }
    return -1;
}
__host__ __device__ constexpr int la_item_I(int C, int P, int t) {   // -1: the V'_PJ item of its J
    for (int J = C - 1; J >= P + 2; --J) {
        if (t < 1 + J - P) return t == 0 ? -1 : P + t;
        t -= 1 + J - P;
    }
    return -2;
}
// waves per SIMD of the pre-split KP = 64 kernel (register budget 512 / waves; LDS 16 x 8.25 KB at 4; 3 waves:
// 3.05 vs 2.83 ms user half, profiles/r05e/ab_k64_waves4_vs_3.log)
constexpr int PS64_WAVES = 4;

// Block LDL^T solve on the Gram tiles left in the MFMA accumulators (no LDS copy of the matrix).
// With C = KP/16 the accumulators hold G' = P G P^T (feature f = C*i + b at position 16*b + i) as upper
// tiles T_IJ (I <= J) in accumulator layout; MFMA operands read straight from those registers because for
// 16x16x4 the A/B slice s of lane (g, c) is "register s" of a tile read as X[4g+s][c] -- the k index runs
// over the rows of the tile, which is exactly what T_PI^T V and A^{-1} T need. Per block column P:
//   S = sweep(T_PP) = -T_PP^{-1};  V'_PJ = S T_PJ (= -T_PP^{-1} T_PJ);  T_IJ += T_PI^T V'_PJ (P < I <= J);
//   forward  b_I += V'_PI^T b_P,  u_P = S b_P;  backward  x_P = -u_P + sum_{I>P} V'_PI x_I.
// The explicit block inverses cost accuracy on ill-conditioned diagonal blocks (forward error grows with
// cond(T_PP), not just cond(A)), so the solve ends with one step of iterative refinement against the
// (scaled, regularised) Gram kept in registers: r = b - A x, x += solve(r). That brings the fp32 error
// below the reference's own fp32 LU (tests/test_gpu_parity.py). Vectors are held "lane (g, j) = element j"
// of each block; buf is KP floats of per-wave LDS.
// Tile storage of the solve. Up to KP = 64 the tiles stay in the MFMA accumulator registers (RegTiles), and so do
// they at KP = 128 on the pre-split path, which keeps no copy of the system (RowResidual); the other KP = 128 paths
// (36 tiles = 144 registers per copy, plus the kept copy) hold the working tiles in per-wave LDS ([tile][lane][reg]),
// loaded a tile at a time (LdsTiles).
template <int C>
struct RegTiles {
    f32x4* t;
    __device__ __forceinline__ f32x4 get(int i) const { return t[i]; }
    __device__ __forceinline__ void put(int i, const f32x4& v) { t[i] = v; }
};
template <int C>
struct RegStore {
    f32x4 t[MfmaAcc<C>::NT];
    __device__ __forceinline__ f32x4 get(int i) const { return t[i]; }
    __device__ __forceinline__ void put(int i, const f32x4& v) { t[i] = v; }
};
// KP = 128 working tiles: [tile][lane][reg] so a tile moves with one ds_read_b128 / ds_write_b128 per lane
// (kbench, k = 128: user half 23.3 -> 20.5 ms against a [tile][reg][lane] b32 layout, at the cost of 3 VGPR spills)
struct LdsTiles {
    float* p;   // per-wave base + 4 * lane
    __device__ __forceinline__ f32x4 get(int i) const { return *(const f32x4*)(p + i * 256); }
    __device__ __forceinline__ void put(int i, const f32x4& v) { *(f32x4*)(p + i * 256) = v; }
};
template <int C>
constexpr bool tiles_in_lds() { return C > 4; }
template <int C>
constexpr int tile_lds_floats() { return tiles_in_lds<C>() ? MfmaAcc<C>::NT * 4 * 64 : 0; }

// Logical in-block entry index of physical position q of a row's padded range (inverse of block_position).
__device__ __forceinline__ int logical_entry(int q) {
    const int w = q % BLOCK_ENTRIES;
    return q - w + (w % BLOCK_SUBSTEPS) * 4 + w / BLOCK_SUBSTEPS;
}

// Tag for solve_tiles' A0: keep NO copy of the system; a refinement step (rare: every Netflix-shape user row passes
// the pivot gate, tools/refine_accuracy.py) forms its residual from the factor rows instead, r = b - D (G (D x) +
// lambda n D x) with G z = sum_e y_e (y_e . z) over the row's entries. G z uses the exact fp32 rows; b is the RHS
// the Gram pass accumulated, which on the pre-split path comes from the split (h + m) values, so the step corrects
// the Gram's 2^-22 representation error but not the RHS's. Frees the copy's registers (4 waves per SIMD on the
// pre-split KP = 64 path instead of 3).
struct RowResidual {
    __device__ __forceinline__ void put(int, const f32x4&) {}
};

// T: working tiles (RegTiles / LdsTiles), A0: kept copy of the scaled system (RegStore / LdsTiles), or RowResidual.
// DUAL: the system is the entry Gram of a short row (als_solve_dual): unknown 16b + j = the row's entry at
// physical position 16b + j, real when that entry exists (padding entries get an identity row), and the
// solution alpha goes to buf[16b + j] (read by the caller after a wave_sync) instead of a factor row.
// u: the units of the tiles and the RHS -- the Gram terms are u^2 times the true ones and the RHS u times (the
// pre-split Gram's table scale; 1 elsewhere). A' = D A D and D b do not depend on u (D scales by 1/u), so the
// factorisation and the scaled solution are the same; the regularisation is added as lambda n u^2 and the solution
// leaves in true units as D x' u.
template <int C, bool DUAL = false, class TT, class KT>
__device__ __forceinline__ void solve_tiles(TT& T, KT& A0, const float (&rhs_acc)[C], float* buf, const Task& tk,
                                            const SolveArgs& a, int lane, float u = 1.f) {
    const int g = lane >> 4, j = lane & 15;
    float* out = (float*)a.out + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)(16 * C);
    auto is_real = [&](int b) { return DUAL ? logical_entry(16 * b + j) < tk.nent : C * j + b < a.k; };
    auto emit = [&](const float (&xs)[C]) {   // xs = solution in the scaled variables, times scol
        if constexpr (DUAL) {
            wave_sync();
            if (g == 0) {
#pragma unroll
                for (int b = 0; b < C; ++b) buf[16 * b + j] = is_real(b) ? xs[b] : 0.f;
            }
        } else if (g == 0) {
            using VT = typename VecC<C>::type;
            VT o;
#pragma unroll
            for (int b = 0; b < C; ++b) o[b] = is_real(b) ? xs[b] : 0.f;
            *(VT*)(out + C * j) = o;
        }
    };
    if (tk.ndeg == 0) {   // cannot occur in the reference (entities exist only once rated); defined as 0
        if (DUAL) {
            float z[C] = {};
            emit(z);
        } else if (g == 0) {
#pragma unroll
            for (int b = 0; b < C; ++b) out[C * j + b] = 0.f;
        }
        return;
    }
    // A + lambda * (n * I) (fp32, MFeatureCalculator.java:91-95: A[f][f] + lambda*(float)n); padded features
    // get an identity row (their Gram rows/columns are exactly zero: padded factor columns are zero).
    // Then Jacobi scaling A' = D A D, b' = D b, x = D x' with D = diag(A)^{-1/2}: lane (g, j) of block b
    // needs s for column j (scol) and for rows 4g..4g+3 (srow), exchanged through buf.
    const float reg = a.lambda * (float)tk.ndeg * (u * u);
    const int jr = j & 3;
    const bool diag_lane = opaque(j >> 2) == g;   // lane holds a diagonal entry, in register j & 3
    float scol[C];
#pragma unroll
    for (int b = 0; b < C; ++b) {
        f32x4 t = T.get(tile_index<C>(b, b));
        const bool real = is_real(b);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool diag = diag_lane && jr == r;
            t[r] = diag ? (real ? t[r] + reg : 1.f) : t[r];
        }
        T.put(tile_index<C>(b, b), t);
        float dv = t[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) dv = (jr == r) ? t[r] : dv;
        if (diag_lane) buf[16 * b + j] = __builtin_amdgcn_rsqf(dv);
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < C; ++b) scol[b] = buf[16 * b + j];
#pragma unroll
    for (int I = 0; I < C; ++I) {
        const f32x4 srow = *(const f32x4*)(buf + 16 * I + 4 * g);   // s for rows 4g .. 4g + 3 of block I
#pragma unroll
        for (int J = I; J < C; ++J) {
            f32x4 t = T.get(tile_index<C>(I, J));
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] *= srow[r] * scol[J];
            T.put(tile_index<C>(I, J), t);
            A0.put(tile_index<C>(I, J), t);
        }
    }
    wave_sync();
    float b0[C];
#pragma unroll
    for (int b = 0; b < C; ++b) b0[b] = col_sum(rhs_acc[b]) * scol[b];

    // ---- factorisation (matrix part only), lookahead schedule ----
    float nrd_min = -1.f;
    {
        {
            f32x4 S0 = T.get(tile_index<C>(0, 0));
            sweep_tile(S0, lane, nrd_min);
            T.put(tile_index<C>(0, 0), S0);
        }
        static_for<0, C - 1>([&](auto P_) {
            constexpr int P = decltype(P_)::value;
            const f32x4 S = T.get(tile_index<C>(P, P));   // -T_PP^{-1}
            const f32x4 orig = T.get(tile_index<C>(P, P + 1));
            const f32x4 v1 = tile_tn(S, orig, f32x4{0.f, 0.f, 0.f, 0.f});
            f32x4 D = tile_tn(orig, v1, T.get(tile_index<C>(P + 1, P + 1)));
            T.put(tile_index<C>(P, P + 1), v1);
            constexpr int m = la_items(C, P);
            f32x4 vcur = {0.f, 0.f, 0.f, 0.f};
            auto item = [&](auto T_) {
                constexpr int t = decltype(T_)::value;
                constexpr int J = la_item_J(C, P, t), I = la_item_I(C, P, t);
                if constexpr (I < 0) {
                    vcur = tile_tn(S, T.get(tile_index<C>(P, J)), f32x4{0.f, 0.f, 0.f, 0.f});
                } else {
                    // T_PI: I = P + 1 was replaced by V'_{P,P+1} above (orig keeps it); P + 1 < I <= J is still the
                    // original (replaced only when its own, later, J group ends)
                    const f32x4 TPI = (I == P + 1) ? orig : T.get(tile_index<C>(P, I));
                    T.put(tile_index<C>(I, J), tile_tn(TPI, vcur, T.get(tile_index<C>(I, J))));
                    if constexpr (I == J) T.put(tile_index<C>(P, J), vcur);   // block row P now holds V'_PJ
                }
            };
            // the sweep of T_{P+1,P+1} with step P's remaining items between its 16 pivot steps
            static_for<0, 16>([&](auto Q_) {
                constexpr int q = decltype(Q_)::value;
                sweep_step<q>(D, lane, nrd_min);
                static_for<q * m / 16, (q + 1) * m / 16>(item);
            });
            T.put(tile_index<C>(P + 1, P + 1), D);
        });
    }

    // ---- x = A^{-1} rhs with the factorisation ----
    auto solve_vec = [&](const float (&rhs)[C], float (&x)[C]) {
        float bw[C], u[C];
#pragma unroll
        for (int b = 0; b < C; ++b) bw[b] = rhs[b];
        static_for<0, C>([&](auto P_) {
            constexpr int P = decltype(P_)::value;
            const f32x4 S = T.get(tile_index<C>(P, P));
            wave_sync();
            if (g == 0) buf[j] = bw[P];           // b_P[4g + r] into every lane of row g
            wave_sync();
            const f32x4 bb = *(const f32x4*)(buf + 4 * g);
            float su = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) su += S[r] * bb[r];
            u[P] = col_sum(su);
            static_for<P + 1, C>([&](auto I_) {
                constexpr int I = decltype(I_)::value;
                const f32x4 V = T.get(tile_index<C>(P, I));
                float sb = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) sb += V[r] * bb[r];
                bw[I] += col_sum(sb);
            });
        });
        static_for<0, C>([&](auto Q_) {
            constexpr int P = C - 1 - decltype(Q_)::value;
            if constexpr (P == C - 1) {
                x[P] = -u[P];
            } else {
                f32x4 w = {0.f, 0.f, 0.f, 0.f};
                static_for<P + 1, C>([&](auto I_) {
                    constexpr int I = decltype(I_)::value;
                    const f32x4 V = T.get(tile_index<C>(P, I));
#pragma unroll
                    for (int r = 0; r < 4; ++r) w[r] += V[r] * x[I];
                });
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = row_sum_to_last(w[r]);
                wave_sync();
                if (j == 15) *(f32x4*)(buf + 4 * g) = w;
                wave_sync();
                x[P] = buf[j] - u[P];
            }
        });
    };
    float x[C];
    solve_vec(b0, x);
    // Well-conditioned systems skip the refinement step: every pivot of the scaled (unit-diagonal) system is a
    // Schur-complement diagonal in (0, 1]; when the smallest is >= a.refine_min_pivot the block factorisation's
    // error is already below the reference's own fp32 LU error. The test is wave-uniform.
    if (-1.f / nrd_min >= a.refine_min_pivot) {
        float xs[C];
#pragma unroll
        for (int b = 0; b < C; ++b) xs[b] = x[b] * scol[b] * u;
        emit(xs);
        return;
    }
    if (a.flags & SOLVE_FLAG_SKIP_REFINE) {   // diagnostics only
        float xs[C];
#pragma unroll
        for (int b = 0; b < C; ++b) xs[b] = x[b] * scol[b] * u;
        emit(xs);
        return;
    }

    // ---- one refinement step: r = b - A x, x += A^{-1} r ----
    float r[C];
    if constexpr (std::is_same<KT, RowResidual>::value) {
        static_assert(!DUAL, "row residual: primal systems only");
        // z = D x (lane (g, j), block b: feature C j + b, the layout of a C-float piece of a factor row)
        float z[C], acc[C];
#pragma unroll
        for (int b = 0; b < C; ++b) {
            z[b] = x[b] * scol[b] * u;   // true units
            acc[b] = 0.f;
        }
        using VT = typename VecC<C>::type;
        const char* obase = (const char*)a.opp + (uint32_t)(C * j * sizeof(float));
        const int32_t* cb = a.col + tk.begin + 8 * g;   // group g: physical entries 8 g .. 8 g + 7 of each block
        const int nblk = (tk.nsteps + BLOCK_SUBSTEPS - 1) / BLOCK_SUBSTEPS;
        for (int blk = 0; blk < nblk; ++blk) {
            const i32x4 c0 = *(const i32x4*)(cb + blk * BLOCK_ENTRIES);
            const i32x4 c1 = *(const i32x4*)(cb + blk * BLOCK_ENTRIES + 4);
#pragma unroll
            for (int t = 0; t < 8; ++t) {   // padding entries read the zero sentinel row
                const uint32_t row = (uint32_t)(t < 4 ? c0[t] : c1[t - 4]);
                const VT y = *(const VT*)(obase + row * (uint32_t)(16 * C * sizeof(float)));
                float p = 0.f;
#pragma unroll
                for (int b = 0; b < C; ++b) p += y[b] * z[b];
                p = row_lane_bcast<15>(row_sum_to_last(p));   // y_e . z over the 16 lanes of the row group
#pragma unroll
                for (int b = 0; b < C; ++b) acc[b] += y[b] * p;
            }
        }
        const float reg = a.lambda * (float)tk.ndeg;
#pragma unroll
        for (int b = 0; b < C; ++b) {
            const float gz = col_sum(acc[b]);
            r[b] = b0[b] - (is_real(b) ? scol[b] * u * (gz + reg * z[b]) : x[b]);   // padded features: identity rows
        }
    } else {
    wave_sync();
    if (g == 0) {
#pragma unroll
        for (int b = 0; b < C; ++b) buf[16 * b + j] = x[b];
    }
    wave_sync();
    f32x4 xr[C];                                   // x_b[4g + q] in row g
#pragma unroll
    for (int b = 0; b < C; ++b) xr[b] = *(const f32x4*)(buf + 16 * b + 4 * g);
    float res[C];
    f32x4 w[C];
#pragma unroll
    for (int b = 0; b < C; ++b) {
        res[b] = 0.f;
        w[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int I = 0; I < C; ++I)
#pragma unroll
        for (int J = I; J < C; ++J) {
            const f32x4 t = A0.get(tile_index<C>(I, J));
#pragma unroll
            for (int q = 0; q < 4; ++q) w[I][q] += t[q] * x[J];            // rows of block I
            if (I != J) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) s += t[q] * xr[I][q];          // (A_IJ^T x_I) at column c
                res[J] += s;
            }
        }
#pragma unroll
    for (int b = 0; b < C; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) w[b][q] = row_sum_to_last(w[b][q]);
    wave_sync();
    if (j == 15) {
#pragma unroll
        for (int b = 0; b < C; ++b) *(f32x4*)(buf + 16 * b + 4 * g) = w[b];
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < C; ++b) r[b] = b0[b] - buf[16 * b + j] - (C > 1 ? col_sum(res[b]) : 0.f);
    }
    float dx[C];
    solve_vec(r, dx);
    float xs[C];
#pragma unroll
    for (int b = 0; b < C; ++b) xs[b] = (x[b] + dx[b]) * scol[b] * u;
    emit(xs);
}

}  // namespace
}  // namespace cfk
