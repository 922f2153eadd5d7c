// Private part of als_kernels.hip: the pre-split fp16 Gram pipeline of als_solve_mfma -- one task's Gram and RHS from
// the pre-split table through LDS-DMA and transposed LDS reads, and the unit handling that follows it.
#pragma once

#include "als_mfma.h"

namespace cfk {
namespace {

// Pre-split fp16 Gram of one FULL / PARTIAL task into acc (tiles, RHS) and E (the diagonal tiles' h m^T terms,
// folded by the caller), in the table's scaled units: Gram terms times 2^(2 sc), the RHS times 2^sc; returns sc.
// The caller brings a PARTIAL task's sums back to true units for its slot and lets a FULL task's solve work in the
// scaled ones (solve_tiles' u: the scaled system is the same after the Jacobi scaling), which saves the 72 ldexp of
// the unscaling at KP = 64. img: the wave's 2 C KB LDS image (1-KB aligned); buf: its KP floats.
template <int KP>
__device__ __forceinline__ int gram_presplit(const SolveArgs& a, const Task& tk, MfmaAcc<KP / 16>& acc,
                                             f32x4 (&E)[KP / 16], unsigned char* img, float* buf, int lane) {
    constexpr int C = KP / 16;
    constexpr int B = BLOCK_SUBSTEPS;
    const int g = lane >> 4, j = lane & 15;
    const int nblk = (tk.nsteps + B - 1) / B;
    // Two-term fp16 Gram over a PRE-SPLIT opposite table (launch_presplit_prepare, once per half: the scaled h/m fp16
    // terms of every factor row, split2). Tile (b1, b2) takes hh + hm + mh (3 MFMAs), a diagonal tile hh + E
    // with E = h m^T folded as E + E^T once per task (2 MFMAs). The RHS Y^T r is 2 MFMAs per feature block on
    // B[k][c] = rh_k (columns 0-7) / rm_k (columns 8-15), r = rh + rm exact in fp16 for every Java short:
    // column 0 + column 8 = Y_b^T r. KP = 64: 34 MFMAs per 32-entry block (the on-the-fly bf16 split: 52
    // + VALU RHS); KP = 128: 116 (200 + VALU RHS).
    static_assert(C == 4 || C == 8, "pre-split Gram: KP = 64 or 128");
    constexpr int NPL = 2;                 // planes h, m
    const char* tbase = (const char*)a.opp_split;
    const int sc = split_exp(*a.amax);     // the table's scale 2^sc (wave-uniform scalar load)
    f32x4 racc[C];
#pragma unroll
    for (int b = 0; b < C; ++b) racc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the block's MFMAs on operands P[plane h/m][feature block b] (entries 8g..8g+7 of feature C j + b as
    // fp16 pairs) and the fp16 rating pairs R of the same entries (rh or rm by the lane's column)
    // FIRST (the task's first block): every accumulator's first MFMA takes the inline constant 0 as its C operand,
    // so the 72 zeroing moves of the accumulators (KP = 64) are not needed on this path
    auto mfma_block = [&](const u32x4 (&P)[NPL][C], const u32x4& R, auto FIRST_) {
        constexpr bool FIRST = decltype(FIRST_)::value;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b1 = 0; b1 < C; ++b1)
#pragma unroll
            for (int b2 = b1; b2 < C; ++b2) {
                f32x4 t = FIRST ? zero : acc.g[tile_index<C>(b1, b2)];
                if (b1 == b2) {
                    E[b1] = mfma_f16(P[0][b1], P[1][b1], FIRST ? zero : E[b1]);
                } else {
                    t = mfma_f16(P[0][b1], P[1][b2], t);
                    t = mfma_f16(P[1][b1], P[0][b2], t);
                }
                t = mfma_f16(P[0][b1], P[0][b2], t);
                acc.g[tile_index<C>(b1, b2)] = t;
            }
#pragma unroll
        for (int b = 0; b < C; ++b) {
            f32x4 t = FIRST ? zero : racc[b];
            t = mfma_f16(P[1][b], R, t);
            t = mfma_f16(P[0][b], R, t);
            racc[b] = t;
        }
        MFMA_DRAIN();
    };
    // LDS image of one 32-entry block per wave (2 C KB: 8 KB at KP = 64, 16 KB at KP = 128): 2 C LDS-DMA
    // instructions (plane pl, 128-B plane half ph, entry quarter m) of 1 KB, instruction = 8 rows x one
    // 128-B half plane, lane 8 r + i holding 16-B chunk i ^ 2 (r >> 1) of the row of entry
    // k = 16 (m >> 1) + 8 (r >> 2) + 4 (m & 1) + (r & 3): whole cache lines per row for the address unit (8
    // lines per instruction), and a chunk swizzle that makes the transposed reads conflict-free. Operand
    // (pl, b) of lane (g, 4 q + p) = two ds_read_b64_tr_b16 (h = 0, 1: entries 8 g + 4 h + 0..3), lane
    // 4 q + p addressing entry 8 g + 4 h + q, plane positions 16 b + 4 p .. + 3 (features C j + b,
    // j = 4 p .. 4 p + 3); the 16 lanes of a group receive features j = 0..15 of their 4 entries: exactly
    // the MFMA A/B operand, no lane movement.
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    constexpr int NH = C / 4;              // 128-B halves per plane
    const int r8 = lane >> 3;
    const uint32_t ld_off = 16u * (uint32_t)((lane & 7) ^ (2 * (r8 >> 1)));
    const int q = (lane >> 2) & 3, p = lane & 3, rr = 4 * (g & 1) + q;
    uint32_t rd[4];   // per feature block b & 3 (the 128-B half b >> 2 is an immediate)
#pragma unroll
    for (int b = 0; b < 4; ++b)
        rd[b] = 2048u * (uint32_t)(g >> 1) + 16u * (uint32_t)(8 * rr + ((2 * b + (p >> 1)) ^ (2 * (rr >> 1)))) +
                8u * (uint32_t)(p & 1);
    // per-plane table bases kept in SGPRs (opaque to the optimiser: folded into the per-lane offset they
    // would force 64-bit addresses; an LDS-DMA takes no immediate offset here, it would move the LDS
    // destination too), so every DMA takes the saddr form with one 32-bit lane offset per row
    const char* tpl[NPL * NH];
#pragma unroll
    for (int x = 0; x < NPL * NH; ++x) {
        tpl[x] = tbase + (x / NH) * 2 * KP + (x % NH) * 128;
        asm volatile("" : "+s"(tpl[x]));
    }
    auto issue = [&](const i32x4& cv) {
        static_for<0, 4>([&](auto M_) {
            constexpr int m = decltype(M_)::value;
            // 24-bit multiply: pre-split tables are host-checked < 2^24 rows and < 4 GiB
            const uint32_t vo = __umul24((uint32_t)cv[m], (uint32_t)presplit_row_bytes(KP)) + ld_off;
            static_for<0, NPL * NH>([&](auto X_) {
                constexpr int x = decltype(X_)::value;   // plane x / NH, half x % NH
                __builtin_amdgcn_global_load_lds((const void*)(tpl[x] + vo),
                                                 (lds_void*)(img + (x * 4 + m) * 1024), 16, 0, 0);
            });
        });
    };
    auto read1 = [&](auto PL_, auto B_) {
        constexpr int pl = decltype(PL_)::value, b = decltype(B_)::value;
        u32x4 P;
        static_for<0, 2>([&](auto H_) {
            constexpr int h = decltype(H_)::value;
            const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (lds_s16x4*)(img + rd[b & 3] + ((pl * NH + (b >> 2)) * 4 + h) * 1024));
            const u32x2 w = __builtin_bit_cast(u32x2, v);
            P[2 * h] = w[0];
            P[2 * h + 1] = w[1];
        });
        return P;
    };
    auto read = [&](u32x4 (&P)[NPL][C]) {
        static_for<0, NPL>([&](auto PL_) {
            static_for<0, C>([&](auto B_) { P[decltype(PL_)::value][decltype(B_)::value] = read1(PL_, B_); });
        });
    };
    if (nblk > 0) {
        const int lastb = nblk - 1;
        const i32x4* cp = (const i32x4*)(a.col_ps + tk.begin) + r8;          // + 8 per block
        // rating pairs of the lane's column half: rh (columns 0-7) or rm (columns 8-15)
        const u32x4* rp = (const u32x4*)(a.rat_pk + (j >= 8 ? a.rat_lo_off : 0) + (tk.begin >> 1)) + g;
        i32x4 cv = cp[0];
        u32x4 Rn = rp[0];
        issue(cv);
        cv = cp[8 * min(1, lastb)];
        auto step = [&](int b, auto FIRST_) {
            const u32x4 R = Rn;
            // every vector-memory op of this wave done: this block's LDS-DMA (and the column / rating loads
            // the DMA issue and the MFMAs below need anyway) -- explicit, not left to the compiler's tracking
            // of LDS-DMA writes (tests/test_isa_guard.py checks it)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            u32x4 P[NPL][C];
            read(P);
            // the operands are in registers before the image is overwritten by the next block's DMA
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (b < lastb) issue(cv);
            cv = cp[8 * min(b + 2, lastb)];
            Rn = rp[4 * min(b + 1, lastb)];
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(P, R, FIRST_);
            __builtin_amdgcn_sched_barrier(0);
        };
        step(0, std::true_type{});
        for (int b = 1; b < nblk; ++b) step(b, std::false_type{});
    }
    // RHS tiles (row i of block b = feature C i + b; column 0 = Y^T rh, column 8 = Y^T rm) -> the per-lane
    // partial layout of the other paths: lane (0, j) holds feature C j + b, the other rows zero (col_sum
    // restores it). The lane's (g, j) derived afresh (opaque): kept live across the Gram loop, one spilled.
    const int lane2 = opaque(lane), g2 = lane2 >> 4, j2 = lane2 & 15;
    wave_sync();
#pragma unroll
    for (int b = 0; b < C; ++b) {
        f32x4 v = racc[b];
#pragma unroll
        for (int r = 0; r < 4; ++r)   // lane (g, 8) += lane (g, 0): DPP row_shr:8
            v[r] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[r]), 0x118, 0xf, 0xf, false));
        if (j2 == 8) *(f32x4*)(buf + 16 * b + 4 * g2) = v;
    }
    wave_sync();
#pragma unroll
    for (int b = 0; b < C; ++b) acc.rhs[b] = (g2 == 0) ? buf[16 * b + j2] : 0.f;
    wave_sync();
    return sc;
}

// Pre-split units: a PARTIAL task's slot holds true units (the REDUCE launch sums slots unscaled); a FULL task
// solves in units of 2^keep (solve_tiles' u), keep = sc clamped to +-30 so that lambda n 2^(2 keep) stays a
// normal float (a table far from unit scale, rare, pays the ldexp of the difference). Powers of two: exact.
// Brings acc from gram_presplit's units 2^ps_sc to 2^keep and returns u = 2^keep.
template <int C>
__device__ __forceinline__ float rescale_presplit(const Task& tk, MfmaAcc<C>& acc, int ps_sc) {
    const int keep = tk.kind == TASK_PARTIAL ? 0 : min(max(ps_sc, -30), 30);
    if (ps_sc != keep) {   // wave-uniform
        const int d = ps_sc - keep;
#pragma unroll
        for (int p = 0; p < MfmaAcc<C>::NT; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc.g[p][r] = ldexpf(acc.g[p][r], -2 * d);
#pragma unroll
        for (int c = 0; c < C; ++c) acc.rhs[c] = ldexpf(acc.rhs[c], -d);
    }
    return ldexpf(1.f, keep);
}

}  // namespace
}  // namespace cfk
