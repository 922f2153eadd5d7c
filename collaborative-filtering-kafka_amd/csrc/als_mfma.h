// Private part of als_kernels.hip: MFMA arithmetic -- the exact bf16 / fp16 operand splits, the k = 32 tile
// products, MFMA_DRAIN with its hazard note, the accumulator layout (MfmaAcc) and the diagonal folds.
#pragma once

#include "als_device.h"

namespace cfk {
namespace {

// ---------------------------------------------------------------------------------------------------
// MFMA Gram path (fp32, KP = 16*C with C in {2, 4})
// ---------------------------------------------------------------------------------------------------
// Exact three-term bf16 split of two fp32 values, packed as bf16 pairs (element 0 = x0 in the low half):
// x = h + m + l with h = bf16_rn(x), m = bf16_rn(x - h), l = bf16_rn(x - h - m). Each residual is exact in
// fp32 and |m| <= 2^-9 |x|, |l| <= 2^-18 |x|, so the dropped partial products m*l, l*m, l*l of x*y are
// below 2^-26 |x y| -- under the fp32 rounding of the product itself -- and every bf16 x bf16 partial
// product is exact in the fp32 MFMA accumulation. 11 VALU instructions per pair.
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ void split3(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    h = pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
    m = pk_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
    l = pk_bf16(s0, s1);
}
__device__ __forceinline__ bf16x8 as_bf16x8(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }
// One 32-entry block of a bf16 partial product: D += A^T B over k = 32 (lane (g, i) element e <-> entry 8g + e).
__device__ __forceinline__ f32x4 mfma_k32(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
}

// Two-term fp16 split of the pre-split tables (als_presplit_scan): x' = x 2^s (s = split_exp of the table's largest |x|,
// so |x'| <= 2^14), h = f16_rn(x'), m = f16_rn(x' - h). x' - h is exact in fp32 and |x' - h - m| <= 2^-22 |x'|, so
// h + m carries 22 significant bits of every value. A product is taken as hh + hm + mh (the dropped mm and the
// representation error are <= 3 2^-22 |x'y'|); every fp16 x fp16 partial product is exact in the fp32 MFMA
// accumulation. Against the three-term bf16 split (six products) this halves the Gram MFMAs. Its accuracy, with the
// rest of the solve exact: per-row error 0.07-0.08x the reference's own fp32 EJML error on every test block, equal
// to rounding the inputs to fp32; the fp32 solve, not the Gram, sets the error.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split2(float x0, float x1, unsigned& h, unsigned& m) {
    const f16x2 hv = __builtin_convertvector(f32x2{x0, x1}, f16x2);
    const f32x2 hf = __builtin_convertvector(hv, f32x2);
    const f16x2 mv = __builtin_convertvector(f32x2{x0 - hf[0], x1 - hf[1]}, f16x2);
    h = __builtin_bit_cast(unsigned, hv);
    m = __builtin_bit_cast(unsigned, mv);
}
__device__ __forceinline__ f32x4 mfma_f16(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
}
// Scale exponent s of a pre-split table from the bits of its largest |x| (als_presplit_scan): 2^s max|x| <= 2^14 < the fp16
// maximum 65504 (no overflow at any rounding), and the table's values use the whole fp16 range (m stays normal for
// |x| >= 2^-17 max|x|). A zero, infinite or NaN maximum keeps s = 0; s is clamped so 2^s and 2^-2s stay usable.
__device__ __forceinline__ int split_exp(uint32_t maxbits) {
    if (maxbits == 0 || maxbits >= 0x7f800000u) return 0;
    int e = (int)(maxbits >> 23) - 127;          // max in [2^e, 2^(e+1)) (normal)
    if (e == -127) e = -126;                     // subnormal maximum
    else if (maxbits & 0x7fffffu) e += 1;        // e = ceil(log2(max))
    const int s = 14 - e;
    return s < -100 ? -100 : (s > 100 ? 100 : s);
}
// Close a group of v_mfma_f32_16x16x32_bf16: the compiler lets VALU instructions overwrite an MFMA's
// A/B/C registers one instruction after it (it models the operands as read at issue), which on gfx950
// intermittently corrupted the Gram (found as run-to-run differences in ~0.1% of rows, tools/determinism.py).
// Every split step therefore issues its MFMAs as one group (sched_barrier before it) and ends it with 16
// wait states before any later instruction may touch the operand registers: bitwise deterministic, same speed.
#ifndef CFK_DRAIN_NOPS
#define CFK_DRAIN_NOPS 2
#endif
#define MFMA_DRAIN()                                                          \
    do {                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                    \
        static_for<0, CFK_DRAIN_NOPS>([&](auto) { asm volatile("s_nop 7"); }); \
        __builtin_amdgcn_sched_barrier(0);                                    \
    } while (0)
// RHS of the on-the-fly split path: computed before its block's MFMA group and materialised there. Computed
// after it (and with SLP-vectorised packed-fp32 VALU), LLVM deferred the RHS products into v_pk_mul /
// v_pk_add_f32 chains next to the next block's MFMAs, and on gfx950 that intermittently lost ~1/3 of RHS
// component 3 in lanes 48..63 of a wave (tools/split_diag.py: 5 of 5 captured failures had this signature;
// 9 wrong movie rows in 300 Netflix-shape halves). Both this and building the kernels without SLP
// vectorisation (Makefile) remove it (0 in 300 halves each).

template <int C>
struct MfmaAcc {
    static constexpr int NT = C * (C + 1) / 2;     // upper-triangular tiles (b1 <= b2)
    static constexpr int NWORDS = NT * 4 + C;       // per-lane words of one partial slot
    f32x4 g[NT];
    float rhs[C];
};

template <int C>
__host__ __device__ constexpr int tile_index(int b1, int b2) { return b1 * C - (b1 * (b1 - 1)) / 2 + (b2 - b1); }

// Diagonal tiles of the split Gram: hm + mh = X + X^T and hl + lh = Y + Y^T with X = h m^T, Y = h l^T, so the
// split paths accumulate X + Y per diagonal tile in E (2 MFMAs instead of 4 per block) and fold
// G_bb += E_b + E_b^T once per task: 8 of the 60 Gram MFMAs per block saved.

// One MFMA operand of the three-term split: the 8 values v(0..7) of a lane as bf16 pairs h4 / m4 / l4. PIN: each word
// materialised where it is computed (pin), so an MFMA group issued after a sched_barrier contains no VALU.
template <bool PIN, class V>
__device__ __forceinline__ void split_operand(V&& v, u32x4& h4, u32x4& m4, u32x4& l4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned h, m, l;
        split3(v(2 * q), v(2 * q + 1), h, m, l);
        if constexpr (PIN) {
            pin(h);
            pin(m);
            pin(l);
        }
        h4[q] = h;
        m4[q] = m;
        l4[q] = l;
    }
}
// The pinned operands of N blocks, v(b, e) = value e of block b.
template <int N, class V>
__device__ __forceinline__ void split_operands(V&& v, u32x4 (&H)[N], u32x4 (&M)[N], u32x4 (&L)[N]) {
#pragma unroll
    for (int b = 0; b < N; ++b) split_operand<true>([&](int e) { return v(b, e); }, H[b], M[b], L[b]);
}
// One tile's MFMAs of a 32-entry block of the split Gram, t += (H1 + M1 + L1)^T (H2 + M2 + L2) less the three products
// below fp32 rounding (split3), in the one order every split path issues (the order decides the bits):
// M.M, H.L, L.H, H.M, M.H, H.H into t; DIAG (the two operands are the same block): M.M into t, H.L and H.M into *e
// (folded as e + e^T once per task, fold_diag), then H.H into t. e is read only when DIAG.
template <bool DIAG>
__device__ __forceinline__ void split_tile_mfma(f32x4& t, f32x4* e, const u32x4& H1, const u32x4& M1, const u32x4& L1,
                                                const u32x4& H2, const u32x4& M2, const u32x4& L2) {
    t = mfma_k32(M1, M2, t);
    if constexpr (DIAG) {
        *e = mfma_k32(H1, L1, *e);
        *e = mfma_k32(H1, M1, *e);
    } else {
        t = mfma_k32(H1, L2, t);
        t = mfma_k32(L1, H2, t);
        t = mfma_k32(H1, M2, t);
        t = mfma_k32(M1, H2, t);
    }
    t = mfma_k32(H1, H2, t);
}

// G_bb += E_b + E_b^T. E^T via v_mfma_f32_16x16x4_f32 against the identity: with both operands in accumulator
// layout the four k-slices compute D += E^T I (see solve_tiles), each output one exact product plus C.
template <int C>
__device__ __forceinline__ void fold_diag(MfmaAcc<C>& acc, f32x4 (&E)[C], int lane) {
    f32x4 I;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = ((lane >> 4) * 4 + r == (lane & 15)) ? 1.f : 0.f;
        pin(v);
        I[r] = v;
    }
    f32x4 D[C];
#pragma unroll
    for (int b = 0; b < C; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc.g[tile_index<C>(b, b)][r] + E[b][r];
            float e = E[b][r];
            pin(v);
            pin(e);
            D[b][r] = v;
            E[b][r] = e;
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < C; ++b) {
        f32x4 t = D[b];
#pragma unroll
        for (int s = 0; s < 4; ++s) t = __builtin_amdgcn_mfma_f32_16x16x4f32(E[b][s], I[s], t, 0, 0, 0);
        acc.g[tile_index<C>(b, b)] = t;
    }
    MFMA_DRAIN();
}

// The same fold with E^T read back transposed from the wave's free LDS image (the pre-split Gram's) instead of 4 C
// v_mfma_f32_16x16x4_f32 against the identity: (acc + E) + E^T in the same order, bitwise the MFMA fold (each of its
// outputs is one exact product plus zeros). The pre-split path uses it (k = 64 / 128 user half -1.6 / -1.8 % in three
// interleaved rounds, profiles/r05e/e26_*.log). Bank-conflict-free image (round 6): lane (g, c) stores its column
// piece E[4g .. 4g+3][c] as one ds_write_b128 at dword 20 c + 4 g of its tile's 1280-B region, so the eight lanes of
// every b128 write group cover the 32 banks once; lane (g, c) then reads E[c][4g + r] with ds_read_b32 at dword
// 20 (4g + r) + 4 (c >> 2) + (c & 3) = 80 g + 20 r + c: 32 distinct banks per 32-lane group. (Round 5 read a
// 16-dword-stride image: 4-way conflicts, SQ_LDS_BANK_CONFLICT 0.118 of the user launch's LDS cycles.)
constexpr int FOLD_TILE_BYTES = 1280;
template <int C>
__device__ __forceinline__ void fold_diag_lds(MfmaAcc<C>& acc, const f32x4 (&E)[C], int lane, unsigned char* img) {
    static_assert(C * FOLD_TILE_BYTES <= 2 * C * 1024, "fold image within the wave's LDS-DMA image");
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int b = 0; b < C; ++b) *(f32x4*)(img + b * FOLD_TILE_BYTES + (20 * c + 4 * g) * 4) = E[b];
    wave_sync();
    const int rd = (80 * g + c) * 4;
#pragma unroll
    for (int b = 0; b < C; ++b) {
        f32x4 t = acc.g[tile_index<C>(b, b)];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            t[r] = (t[r] + E[b][r]) + *(const float*)(img + b * FOLD_TILE_BYTES + rd + r * 80);
        acc.g[tile_index<C>(b, b)] = t;
    }
    wave_sync();
}

}  // namespace
}  // namespace cfk
