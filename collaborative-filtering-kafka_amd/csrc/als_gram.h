// Private part of als_kernels.hip: the Gram pipelines of als_solve_mfma that gather fp32 factor rows into registers --
// the block loader and row gather they share, the fp32 Gram and the on-the-fly bf16 split Gram of one task.
#pragma once

#include "als_mfma.h"

namespace cfk {
namespace {

// Gather pipeline over blocks of B = 8 sub-steps (32 entries, layout [g][t], see block_position):
// lane (g, j) loads the 8 column indices / ratings of its group with two 16-B loads, issued one
// block ahead of that block's gathers, which are issued one block ahead of their MFMAs. The loop
// body is branch-free, so vmcnt retires in program order with 8 gathers (8 KB per wave) still in
// flight under each block's 80 MFMAs.
struct Cols { i32x4 i[2]; };
struct Rats { f32x4 r[2]; };
struct Idx : Cols, Rats {};
// The column and rating blocks of one task, as lane group g reads them.
struct BlockLoader {
    const int32_t* cb;
    const float* rb;
    __device__ __forceinline__ BlockLoader(const SolveArgs& a, const Task& tk, int g)
        : cb(a.col + tk.begin + g * BLOCK_SUBSTEPS), rb(a.rat + tk.begin + g * BLOCK_SUBSTEPS) {}
    __device__ __forceinline__ void cols(int blk, Cols& x) const {
        const int32_t* c = cb + (int64_t)blk * BLOCK_ENTRIES;
        x.i[0] = *(const i32x4*)c;
        x.i[1] = *(const i32x4*)(c + 4);
    }
    __device__ __forceinline__ void rats(int blk, Rats& x) const {
        const float* r = rb + (int64_t)blk * BLOCK_ENTRIES;
        x.r[0] = *(const f32x4*)r;
        x.r[1] = *(const f32x4*)(r + 4);
    }
    __device__ __forceinline__ void idx(int blk, Idx& x) const {
        cols(blk, x);
        rats(blk, x);
    }
};
// Lane (g, j)'s C-float piece of the opposite factor rows a block names. Unconditional: padding entries index the
// sentinel zero row. Wave-uniform table base + 32-bit unsigned per-lane byte offsets (row << log2(row bytes), + this
// lane's piece; host-checked: opposite table <= 4 GiB, e.g. 16.7M rows at k = 64): the loads take the saddr form, one
// v_lshl_add_u32 per gathered row instead of a 64-bit address per lane.
template <int KP>
struct RowGather {
    static constexpr int C = KP / 16, B = BLOCK_SUBSTEPS;
    static constexpr int ROW_SHIFT = __builtin_ctz(KP * sizeof(float));
    using VT = typename VecC<C>::type;
    const char* obase;
    uint32_t lane_off;
    __device__ __forceinline__ RowGather(const SolveArgs& a, int j)
        : obase((const char*)a.opp), lane_off((uint32_t)(C * j * sizeof(float))) {}
    __device__ __forceinline__ VT row(int32_t col) const {
        return *(const VT*)(obase + (((uint32_t)col << ROW_SHIFT) + lane_off));
    }
    __device__ __forceinline__ void block(const Cols& x, VT (&y)[B]) const {
#pragma unroll
        for (int t = 0; t < B; ++t) y[t] = row(x.i[t >> 2][t & 3]);
    }
    template <int h>   // sub-steps 4 h .. 4 h + 3
    __device__ __forceinline__ void half(const Cols& x, VT (&y)[B / 2]) const {
#pragma unroll
        for (int t = 0; t < B / 2; ++t) y[t] = row(x.i[h][t]);
    }
};

// One sub-step (4 entries, one gathered piece per lane) of the fp32 Gram: a v_mfma_f32_16x16x4_f32 per upper tile,
// the RHS a per-lane FMA.
template <int C>
__device__ __forceinline__ void f32_step(MfmaAcc<C>& acc, const typename VecC<C>::type& y, float r) {
#pragma unroll
    for (int b1 = 0; b1 < C; ++b1)
#pragma unroll
        for (int b2 = b1; b2 < C; ++b2)
            acc.g[tile_index<C>(b1, b2)] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                y[b1], y[b2], acc.g[tile_index<C>(b1, b2)], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < C; ++c) acc.rhs[c] += r * y[c];
}

// fp32 Gram of one FULL / PARTIAL task (ALS_GRAM=f32, and KP = 32 without the split).
template <int KP>
__device__ __forceinline__ void gram_f32(const SolveArgs& a, const Task& tk, MfmaAcc<KP / 16>& acc, int lane) {
    constexpr int C = KP / 16, B = BLOCK_SUBSTEPS;
    using VT = typename VecC<C>::type;
    const int n = tk.nsteps;
    const int nblk = (n + B - 1) / B;
    const BlockLoader ld(a, tk, lane >> 4);
    const RowGather<KP> rows(a, lane & 15);
    if (nblk <= 0) return;
    if constexpr (C > 4) {
        // KP = 128: 288 MFMAs per block, so half a block of prefetch (4 gathered rows per lane in
        // flight) covers the gather latency and halves the staging registers (the 36 accumulator
        // tiles already take 144). Stage = 4 sub-steps = one 16-B index/rating vector per lane.
        constexpr int H = B / 2;
        Idx x_c, x_n;
        VT y_c[H], y_n[H];
        ld.idx(0, x_c);
        ld.idx(nblk > 1 ? 1 : 0, x_n);
        rows.template half<0>(x_c, y_c);
        for (int b = 0; b + 1 < nblk; ++b) {
            rows.template half<1>(x_c, y_n);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < H; ++t) f32_step<C>(acc, y_c[t], x_c.r[0][t]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < H; ++t) y_c[t] = y_n[t];
            Idx x_nn;
            ld.idx(b + 2 < nblk ? b + 2 : nblk - 1, x_nn);   // clamped: always a valid address
            rows.template half<0>(x_n, y_n);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < H; ++t) f32_step<C>(acc, y_c[t], x_c.r[1][t]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < H; ++t) y_c[t] = y_n[t];
            x_c = x_n;
            x_n = x_nn;
        }
        const int last = n - (nblk - 1) * B;
        rows.template half<1>(x_c, y_n);
#pragma unroll
        for (int t = 0; t < H; ++t)
            if (t < last) f32_step<C>(acc, y_c[t], x_c.r[0][t]);     // wave-uniform
#pragma unroll
        for (int t = 0; t < H; ++t)
            if (H + t < last) f32_step<C>(acc, y_n[t], x_c.r[1][t]);
    } else {
        Idx x_c, x_n;
        VT y_c[B], y_n[B];
        ld.idx(0, x_c);
        ld.idx(nblk > 1 ? 1 : 0, x_n);
        rows.block(x_c, y_c);
        for (int b = 0; b + 1 < nblk; ++b) {
            Idx x_nn;
            ld.idx(b + 2 < nblk ? b + 2 : nblk - 1, x_nn);   // clamped: always a valid address
            rows.block(x_n, y_n);
            // keep the prefetch above the MFMAs: without this the scheduler sinks the gathers below
            // them (saving registers) and every block waits out a full memory latency
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < B; ++t) f32_step<C>(acc, y_c[t], x_c.r[t >> 2][t & 3]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < B; ++t) y_c[t] = y_n[t];
            x_c = x_n;
            x_n = x_nn;
        }
        const int last = n - (nblk - 1) * B;     // sub-steps with real entries in the last block
#pragma unroll
        for (int t = 0; t < B; ++t)
            if (t < last) f32_step<C>(acc, y_c[t], x_c.r[t >> 2][t & 3]);   // wave-uniform
    }
}

// Tile (b1, b2) of the on-the-fly split Gram for one block: split_tile_mfma on the accumulators, E taking the
// diagonal tiles' H.L + H.M.
template <int C>
__device__ __forceinline__ void split_tile(MfmaAcc<C>& acc, f32x4 (&E)[C], const u32x4 (&H)[C], const u32x4 (&M)[C],
                                           const u32x4 (&L)[C], int b1, int b2) {
    f32x4& t = acc.g[tile_index<C>(b1, b2)];
    if (b1 == b2) split_tile_mfma<true>(t, &E[b1], H[b1], M[b1], L[b1], H[b1], M[b1], L[b1]);
    else split_tile_mfma<false>(t, nullptr, H[b1], M[b1], L[b1], H[b2], M[b2], L[b2]);
}

// On-the-fly three-term bf16 split Gram of one FULL / PARTIAL task (ALS_PRESPLIT=0, KP = 32, and the range guard's
// fallback), into acc and E (folded by the caller, fold_diag).
// One v_mfma_f32_16x16x32_bf16 consumes a whole 32-entry block. Lane (g, j)
// holds A[i = j][k = 8g + t] = y_t[C*j + b] (its own gathered piece, component b, entry t of its
// group): with the interleaved feature order (f = C*i + b) the operands need no lane movement,
// and the accumulators come out in exactly the layout of the f32 path (tile (b1, b2) holds
// G[C*i + b1][C*j' + b2]), so the solve, the partial slots and the REDUCE pass are shared.
// Padding entries gather the sentinel zero row with rating 0, so the last block needs no mask.
template <int KP>
__device__ __forceinline__ void gram_split(const SolveArgs& a, const Task& tk, MfmaAcc<KP / 16>& acc,
                                           f32x4 (&E)[KP / 16], int lane) {
    constexpr int C = KP / 16, B = BLOCK_SUBSTEPS;
    using VT = typename VecC<C>::type;
    const int nblk = (tk.nsteps + B - 1) / B;
    const BlockLoader ld(a, tk, lane >> 4);
    const RowGather<KP> rows(a, lane & 15);
    if (nblk <= 0) return;
    const int lastb = nblk - 1;
    Cols I0, I1;
    Rats R0, R1;
    VT Y0[B], Y1[B];
    if constexpr (C > 4) {
        // KP = 128, one wave per SIMD: no second wave hides the split VALU behind this wave's MFMAs, so
        // the wave interleaves them itself. The tiles are issued column by column (column c = tiles
        // (b1 <= c, c): 6c + 4 MFMAs), and the split of feature block c + 1 -- the only new operand
        // column c + 1 needs -- plus a share of the RHS FMAs run in the issue gaps of column c's MFMAs
        // (an MFMA holds vector issue for 8 of its 16 cycles: two VALU per gap). Column 7's gaps split
        // feature block 0 of the next block. No operand register dies before column 7 and all of them
        // are kept allocated past the closing drain (keep_alive), so no VALU result can land in a
        // register an MFMA in flight still reads. Same products, same accumulation order per tile and
        // per RHS component as the C <= 4 split_step: bitwise equal results.
        u32x4 H[C], M[C], L[C];
        auto split_feat = [&](const VT (&y)[B], int c, u32x4& h4, u32x4& m4, u32x4& l4) {
            split_operand<false>([&](int e) { return y[e][c]; }, h4, m4, l4);
        };
        auto keep_alive = [&]() {
#pragma unroll
            for (int b = 0; b < C; ++b) asm volatile("" ::"v"(H[b]), "v"(M[b]), "v"(L[b]));
        };
        // one block: y/x = this block, yn = the next block (its feature block 0 is split here) when NEXT
        auto block = [&](const VT (&y)[B], const Rats& x, const VT (&yn)[B], auto next_) {
            constexpr bool NEXT = decltype(next_)::value;
            u32x4 hn, mn, ln;
            static_for<0, C>([&](auto C_) {
                constexpr int c = decltype(C_)::value;
#pragma unroll
                for (int b1 = 0; b1 <= c; ++b1) split_tile<C>(acc, E, H, M, L, b1, c);
                if constexpr (c + 1 < C) split_feat(y, c + 1, H[c + 1], M[c + 1], L[c + 1]);
                // RHS components 0-1 in column 5's gaps, 2-4 in column 6's, 5-7 in column 7's
                constexpr int r0 = c == 5 ? 0 : c == 6 ? 2 : c == 7 ? 5 : C;
                constexpr int r1 = c == 5 ? 2 : c == 6 ? 5 : c == 7 ? 8 : C;
#pragma unroll
                for (int f = r0; f < r1; ++f)
#pragma unroll
                    for (int t = 0; t < B; ++t) acc.rhs[f] += x.r[t >> 2][t & 3] * y[t][f];
                if constexpr (NEXT && c == C - 1) split_feat(yn, 0, hn, mn, ln);
                static_for<0, 6 * c + 4>([&](auto) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // 2 VALU
                });
                __builtin_amdgcn_sched_barrier(0);
            });
            MFMA_DRAIN();
            keep_alive();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NEXT) {
                H[0] = hn;
                M[0] = mn;
                L[0] = ln;
            }
        };
        using Yes = std::integral_constant<bool, true>;
        using No = std::integral_constant<bool, false>;
        // one block per trip, staging rotated (two blocks per trip with ping-pong buffers made the
        // register allocator shuffle the 144 accumulator registers at every back edge)
        ld.cols(0, I0);
        ld.cols(min(1, lastb), I1);
        rows.block(I0, Y0);
        ld.rats(0, R0);
        split_feat(Y0, 0, H[0], M[0], L[0]);
        for (int b = 0; b < lastb; ++b) {
            rows.block(I1, Y1);
            ld.rats(b + 1, R1);
            ld.cols(min(b + 2, lastb), I1);
            __builtin_amdgcn_sched_barrier(0);
            block(Y0, R0, Y1, Yes{});
#pragma unroll
            for (int t = 0; t < B; ++t) Y0[t] = Y1[t];
            R0 = R1;
        }
        block(Y0, R0, Y1, No{});
    } else {
        auto split_step = [&](const VT (&y)[B], const Rats& x) {
            u32x4 H[C], M[C], L[C];
            split_operands<C>([&](int b, int e) { return y[e][b]; }, H, M, L);
            // the RHS before the MFMA group, materialised (see the RHS note at MFMA_DRAIN)
#pragma unroll
            for (int t = 0; t < B; ++t)
#pragma unroll
                for (int c = 0; c < C; ++c) acc.rhs[c] += x.r[t >> 2][t & 3] * y[t][c];
#pragma unroll
            for (int c = 0; c < C; ++c) pin(acc.rhs[c]);
            // the operands are materialised above (pin: MachineSink ignores sched_barrier), so the MFMA group
            // below contains no VALU that could overwrite an operand register of an MFMA in flight
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b1 = 0; b1 < C; ++b1)
#pragma unroll
                for (int b2 = b1; b2 < C; ++b2) split_tile<C>(acc, E, H, M, L, b1, b2);
            MFMA_DRAIN();
        };
        // Two blocks per trip with ping-pong buffers (no register rotation): column indices are loaded two
        // blocks ahead of their gathers' use, gathers and ratings one block ahead of their MFMAs.
        // Invariant at the loop top: Y0/R0 in flight for block b, I1 = columns of b+1, I0 = columns of b+2.
        ld.cols(0, I0);
        ld.cols(min(1, lastb), I1);
        rows.block(I0, Y0);
        ld.rats(0, R0);
        ld.cols(min(2, lastb), I0);
        int b = 0;
        for (; b + 2 < nblk; b += 2) {
            rows.block(I1, Y1);
            ld.rats(b + 1, R1);
            ld.cols(min(b + 3, lastb), I1);
            __builtin_amdgcn_sched_barrier(0);
            split_step(Y0, R0);
            __builtin_amdgcn_sched_barrier(0);
            rows.block(I0, Y0);
            ld.rats(b + 2, R0);
            ld.cols(min(b + 4, lastb), I0);
            __builtin_amdgcn_sched_barrier(0);
            split_step(Y1, R1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (nblk - b == 2) {
            rows.block(I1, Y1);
            ld.rats(b + 1, R1);
            __builtin_amdgcn_sched_barrier(0);
            split_step(Y0, R0);
            split_step(Y1, R1);
        } else {
            split_step(Y0, R0);
        }
    }
}

}  // namespace
}  // namespace cfk
