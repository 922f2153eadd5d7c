// als_kernels.hip -- hand-written gfx950 (CDNA4) kernels for the ALS half-iteration, and their launchers.
//
// Hot path being replaced: MFeatureCalculator.java:66-104 / UFeatureCalculator.java:66-104 (EJML fp32
// multTransA -> add(lambda * n * I) -> invert -> mult, one entity at a time). Here one 64-lane wave owns
// one Task (cfk::Task, see als_internal.h): it gathers the opposite factor rows of its in-block entries,
// accumulates the Gram matrix Y^T Y and RHS Y^T r, and -- for FULL / REDUCE tasks -- regularises and solves the
// k x k system inside the wave, writing one factor row.
//
// One of the library's .hip units: the half-iteration, squared error, predict and the copies (als_build, als_recommend,
// als_rank, als_foldin and als_implicit hold their own kernels). Device helpers: private headers, one concern each, in order:
//   als_device.h         vector types, wave_sync, bcast, uni, static_for, opaque, pin, load_task
//   als_slots.h          partial-slot codec and integrity report (SlotCodec), store_partial, sum_partial_slots
//   als_lds_solve.h      VALU path: per-wave LDS carve-up and the packed-lower-triangle Cholesky (solve_store)
//   als_mfma.h           bf16 / fp16 operand splits, tile products, MFMA_DRAIN, MfmaAcc, the diagonal folds
//   als_tile_solve.h     MFMA paths: sweep operator and block LDL^T solve on the accumulator tiles (solve_tiles)
//   als_gram.h           Gram pipelines on gathered fp32 rows: block loader, row gather, gram_f32, gram_split
//   als_gram_presplit.h  the pre-split fp16 Gram pipeline (LDS-DMA, transposed LDS reads), rescale_presplit
//   als_generic.h        the any-k workgroup-per-row kernels
// Below: the table preparation kernels of the pre-split Gram, als_solve_mfma (the MFMA paths: Gram, fold, solve),
// als_solve_dual (short rows in entry space), als_solve_valu, squared error, prediction, and the launchers.
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "als_internal.h"
#include "als_device.h"
#include "als_slots.h"
#include "als_lds_solve.h"
#include "als_mfma.h"
#include "als_tile_solve.h"
#include "als_gram.h"
#include "als_gram_presplit.h"
#include "als_generic.h"

namespace cfk {
namespace {

// Waves (tasks) per workgroup of the MFMA kernel: WAVES (4) at every KP, KP = 128 with its per-wave LDS tiles
// included. The one place to change should a KP ever want another count.
template <int KP>
constexpr int mfma_waves() { return WAVES; }

// Range statistics of a table for the pre-split Gram, from the bits of |x| (non-negative floats order as unsigned
// integers): word 0 = the largest |x| (the split scale, split_exp), word 1 = ~(the smallest nonzero row maximum) (a
// max of complements is a min; 0 = no nonzero row). als_presplit_scan accumulates them while it splits the table.
// The pre-split (table-wide scale, two fp16 terms) keeps ~22 significant bits for values within 2^-17 of the table's
// largest |x| and falls toward the fp16 subnormal floor below; it serves a half only when every nonzero row's
// maximum is within PRESPLIT_RANGE of the table's. Otherwise that half's Gram runs on the fp32 table with the
// on-the-fly three-term bf16 split (an 8-bit exponent per value): the pre-split kernels exit at once and the
// guarded on-the-fly launch after them does the work (SolveArgs::presplit_fallback).
constexpr float PRESPLIT_RANGE = 65536.f;
__device__ __forceinline__ bool presplit_ok(const uint32_t* st) {
    const uint32_t mx = st[0], rc = st[1];
    if (mx >= 0x7f800000u) return false;   // inf / NaN in the table: the fp32 path propagates it as the reference would
    if (rc == 0) return true;              // no nonzero row
    return __uint_as_float(mx) <= PRESPLIT_RANGE * __uint_as_float(~rc);
}

// fp32 table -> fp16 h/m planes (presplit_row_bytes(KP) per row, als_internal.h) at the scale 2^sc: item t = (row, b,
// jh) splits features C (8 jh + i) + b, i = 0..7, and writes 16 B per plane at plane position 16 b + 8 jh. Returns the
// bits of the largest |x| of its eight values.
template <int KP>
__device__ __forceinline__ uint32_t presplit_item(const float* __restrict__ src, unsigned* __restrict__ dst, int64_t t,
                                                  int sc) {
    constexpr int C = KP / 16;
    const int64_t row = t / (2 * C);
    const int b = (int)(t % (2 * C)) >> 1, jh = (int)(t & 1);
    const float* s = src + row * KP + C * 8 * jh + b;
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = s[C * i];
    u32x4 h, m;
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned hh, mm;
        split2(ldexpf(x[2 * i], sc), ldexpf(x[2 * i + 1], sc), hh, mm);
        h[i] = hh;
        m[i] = mm;
        v = max(v, max(__float_as_uint(x[2 * i]) & 0x7fffffffu, __float_as_uint(x[2 * i + 1]) & 0x7fffffffu));
    }
    unsigned* o = dst + row * (presplit_row_bytes(KP) / 4) + (16 * b + 8 * jh) / 2;
    *(u32x4*)o = h;
    *(u32x4*)(o + KP / 2) = m;   // plane stride 2 KP bytes
    return v;
}
// The one pass of a table's preparation: splits the table at the PREDICTED exponent *pred (the exponent this side's
// table was last split at; PREP_NO_EXP: none yet, any exponent does) and accumulates the range words of the same
// values into set[0..1], which als_presplit_confirm zeroed after the preparation before last. Grid-stride over
// 1024-thread workgroups; the 2 C items of a row are consecutive lanes of one wave (the stride is a multiple of 64);
// workgroup reduction, at most one vector-memory atomicMax per workgroup and word (thousands of same-address atomics
// serialise: 53 us for the 4.5 MB M table), none where the word already holds as much. set[PREP_EXP] <- *pred.
template <int KP>
__global__ __launch_bounds__(1024) void als_presplit_scan(const float* __restrict__ src, unsigned* __restrict__ dst,
                                                         int64_t n_items, const uint32_t* __restrict__ pred,
                                                         uint32_t* __restrict__ set) {
    const uint32_t p = *pred;
    const int sc = p == PREP_NO_EXP ? 0 : (int)p;
    uint32_t m = 0, rmin = 0xffffffffu;
    const int64_t stride = (int64_t)gridDim.x * 1024;
    for (int64_t t0 = (int64_t)blockIdx.x * 1024 + (threadIdx.x & ~63); t0 < n_items; t0 += stride) {
        const int64_t t = t0 + (threadIdx.x & 63);
        uint32_t v = t < n_items ? presplit_item<KP>(src, dst, t, sc) : 0;
        m = max(m, v);
#pragma unroll
        for (int o = 1; o < 2 * (KP / 16); o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));   // the row's maximum
        if (v != 0 && t < n_items) rmin = min(rmin, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = max(m, (uint32_t)__shfl_xor((int)m, o));
        rmin = min(rmin, (uint32_t)__shfl_xor((int)rmin, o));
    }
    __shared__ uint32_t wm[16], wr[16];
    if ((threadIdx.x & 63) == 0) {
        wm[threadIdx.x >> 6] = m;
        wr[threadIdx.x >> 6] = rmin;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        m = threadIdx.x < 16 ? wm[threadIdx.x] : 0;
        rmin = threadIdx.x < 16 ? wr[threadIdx.x] : 0xffffffffu;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {
            m = max(m, (uint32_t)__shfl_xor((int)m, o));
            rmin = min(rmin, (uint32_t)__shfl_xor((int)rmin, o));
        }
        if (threadIdx.x == 0) {
            // the words only grow during the launch: a value read early can only ask for an atomic too many
            if (m > __hip_atomic_load(set, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(set, m);
            if (~rmin > __hip_atomic_load(set + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(set + 1, ~rmin);
            if (blockIdx.x == 0) set[PREP_EXP] = p;
        }
    }
}
// After the scan: the table's true exponent is split_exp of set[0]. Where the scan split at it (the prediction was
// right, as it is unless the table's maximum crossed a power of two), every wave exits after its scalar loads; else
// the capped grid strides over the table and splits it again at the true exponent. Either way thread 0 stores the
// true exponent as the side's next prediction and zeroes the set the next preparation accumulates into (no launch
// reads that one any more: the launches of the half it served precede this one on the stream).
template <int KP>
__global__ __launch_bounds__(256) void als_presplit_confirm(const float* __restrict__ src, unsigned* __restrict__ dst,
                                                           int64_t n_items, const uint32_t* __restrict__ set,
                                                           uint32_t* __restrict__ next_set, uint32_t* __restrict__ pred) {
    const int sc = split_exp(set[0]);
    const bool right = set[PREP_EXP] == (uint32_t)sc;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *pred = (uint32_t)sc;
        next_set[0] = 0;
        next_set[1] = 0;
    }
    if (right) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n_items; t += stride) presplit_item<KP>(src, dst, t, sc);
}
// In-block column indices in the order of the LDS-DMA gather: inside a 32-entry block, word 4 r + x (r = 0..7,
// x = 0..3) holds the column of entry k = 16 (x >> 1) + 8 (r >> 2) + 4 (x & 1) + (r & 3), so the 8 lanes of loader
// row r fetch the rows of their 4 DMA instructions with one 16-B load.
__global__ __launch_bounds__(256) void als_pack_cols_ps(const int32_t* __restrict__ col, int32_t* __restrict__ dst,
                                                       int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int w = (int)(i & 31), r = w >> 2, x = w & 3;
    const int k = 16 * (x >> 1) + 8 * (r >> 2) + 4 * (x & 1) + (r & 3);
    dst[i] = col[(i & ~(int64_t)31) + k];
}

// REDUCE = true: the launch of a half's REDUCE tasks (sum of partial slots + solve), compiled apart from the
// gather kernel so neither carries the other's code and registers.
// GRIDLOOP: a grid-stride loop over the tasks (the range guard's fallback launch, whose grid is capped: when the
// pre-split serves the half, as it nearly always does, its waves exit without a full-size grid's dispatch cost).
template <int KP, int MINW, bool SPLIT, bool PRESPLIT = false, bool REDUCE = false, bool GRIDLOOP = false>
__global__ __launch_bounds__(64 * mfma_waves<KP>(), MINW) void als_solve_mfma(SolveArgs a) {
    constexpr int C = KP / 16;
    constexpr int NW = mfma_waves<KP>();
    using Acc = MfmaAcc<C>;
    __shared__ __attribute__((aligned(16))) float sbuf[NW][KP];
    // KP = 128 keeps the solve's working tiles in per-wave LDS, except on the pre-split path: its solve keeps no copy
    // of the system (RowResidual), which leaves the registers for the tiles themselves (user half 11.4 -> 10.5 ms)
    constexpr bool TILES_LDS = tiles_in_lds<C>() && !(PRESPLIT && !REDUCE);
    constexpr int TL = TILES_LDS ? tile_lds_floats<C>() : 0;
    __shared__ __attribute__((aligned(16))) float tiles_lds[NW][TL > 0 ? TL : 1];
    (void)tiles_lds;
    // pre-split Gram: one block's LDS image per wave (LDS-DMA target)
    constexpr int STAGE = (PRESPLIT && !REDUCE) ? 2 * C * 1024 : 16;
    __shared__ __attribute__((aligned(1024))) unsigned char stage_lds[NW][STAGE];
    (void)stage_lds;

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the table-range guard (presplit_ok): a pre-split launch serves the half only in range, its guarded on-the-fly
    // fallback only out of range (one scalar load per wave; the other launch's waves exit here)
    if constexpr (!REDUCE && SPLIT) {
        if (PRESPLIT ? !presplit_ok(a.amax) : (a.presplit_fallback && presplit_ok(a.amax))) return;
    }
    // one task per wave (wave-uniform; no workgroup barriers are used below)
    auto task = [&](const int tid) {
        const Task tk = load_task(a.tasks + tid);
        float* buf = sbuf[wave];

        Acc acc;
#pragma unroll
        for (int p = 0; p < Acc::NT; ++p) acc.g[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) acc.rhs[c] = 0.f;
        f32x4 E[C];   // split paths: h m^T + h l^T of the diagonal tiles (fold_diag)
#pragma unroll
        for (int c = 0; c < C; ++c) E[c] = f32x4{0.f, 0.f, 0.f, 0.f};

        // the Gram and the RHS of the task, by one of the pipelines of als_slots.h / als_gram.h
        int ps_sc = 0;   // pre-split Gram: its sums are in units of 2^(2 ps_sc) (tiles) and 2^ps_sc (RHS)
        if constexpr (REDUCE) sum_partial_slots<C>(a, tk, acc, lane);
        else if constexpr (PRESPLIT) ps_sc = gram_presplit<KP>(a, tk, acc, E, stage_lds[uni(wave)], buf, lane);
        else if constexpr (SPLIT) gram_split<KP>(a, tk, acc, E, lane);
        else gram_f32<KP>(a, tk, acc, lane);

        if constexpr (SPLIT && !REDUCE) {
            if constexpr (PRESPLIT)
                // the image is free after the Gram; the fold's lane addresses are derived afresh (opaque: kept live
                // across the Gram loop, one of them spilled at 128 VGPRs)
                fold_diag_lds<C>(acc, E, opaque(lane), stage_lds[uni(wave)]);
            else
                fold_diag<C>(acc, E, lane);
        }

        float u = 1.f;   // the units of acc (rescale_presplit)
        if constexpr (PRESPLIT && !REDUCE) u = rescale_presplit<C>(tk, acc, ps_sc);
        if (!REDUCE && tk.kind == TASK_PARTIAL) {
            store_partial<C>(a, tk, acc, lane);
            return;
        }
        if (a.flags & SOLVE_FLAG_SKIP_SOLVE) {   // diagnostics (kbench): Gram only
            float* out = (float*)a.out + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)KP;
            if (lane < 16) {
#pragma unroll
                for (int b = 0; b < C; ++b) out[C * lane + b] = acc.g[tile_index<C>(b, b)][0] + acc.rhs[b];
            }
            return;
        }
        if constexpr (TILES_LDS) {
            LdsTiles T{tiles_lds[wave] + 4 * lane};
            RegStore<C> A0;
#pragma unroll
            for (int p = 0; p < Acc::NT; ++p) T.put(p, acc.g[p]);
            solve_tiles<C>(T, A0, acc.rhs, buf, tk, a, lane);
        } else if constexpr (PRESPLIT && !REDUCE) {
            RegTiles<C> T{acc.g};
            RowResidual A0;
            solve_tiles<C>(T, A0, acc.rhs, buf, tk, a, lane, u);
        } else {
            RegTiles<C> T{acc.g};
            RegStore<C> A0;
            solve_tiles<C>(T, A0, acc.rhs, buf, tk, a, lane);
        }
    };
    if constexpr (GRIDLOOP) {
        for (int tid = blockIdx.x * NW + wave; tid < a.n_tasks; tid += gridDim.x * NW) task(tid);
    } else {
        const int tid = blockIdx.x * NW + wave;
        if (tid < a.n_tasks) task(tid);
    }
}

// ---------------------------------------------------------------------------------------------------
// Short rows in entry space (fp32, split-bf16 MFMA)
// ---------------------------------------------------------------------------------------------------
// For a row with n <= 16 * CD entries (its 1 or 2 padded 32-entry blocks, CD = 2 or 4) the update
//   m = (Y^T Y + lambda n I_k)^{-1} Y^T r      (MFeatureCalculator.java:85-99, Y = the n x k gathered rows)
// equals  m = Y^T alpha  with  (Y Y^T + lambda n I_n) alpha = r  (push-through identity; the same nonzero
// spectrum and conditioning), an n x n system instead of k x k: at k = 128 a 64-entry user costs a 64 x 64
// solve instead of 128 x 128. The entry Gram Y Y^T needs no operand transposition: lane (g, i) loads the 32-B
// piece [32s + 8g, 32s + 8g + 8) of entry 16I + i's factor row, which is directly the A (and B) operand
// "row i, k = 8g..8g+7" of v_mfma_f32_16x16x32_bf16 for feature chunk s, split exactly into h/m/l bf16 terms
// as on the primal path. Entries are in physical (padded, block-interleaved) order; padding entries gather
// the zero sentinel row with rating 0 and get an identity row (solve_tiles<DUAL>), so alpha is 0 there.
template <int KP, int CD>
__global__ __launch_bounds__(64 * WAVES, CD <= 4 ? 2 : 1) void als_solve_dual(SolveArgs a) {
    constexpr int NS = KP / 32;      // 32-feature chunks = MFMA K steps
    constexpr int NF = KP / 64;      // output features per lane
    using Acc = MfmaAcc<CD>;
    __shared__ __attribute__((aligned(16))) float sbuf[WAVES][16 * CD];
    constexpr int TL = tile_lds_floats<CD>();
    __shared__ __attribute__((aligned(16))) float tiles_lds[WAVES][TL > 0 ? TL : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tid = blockIdx.x * WAVES + wave;
    if (tid >= a.n_tasks) return;   // wave-uniform; no workgroup barriers below
    const Task tk = load_task(a.tasks + tid);
    float* buf = sbuf[wave];
    const int g = lane >> 4, i = lane & 15;
    const float* opp = (const float*)a.opp;
    int cidx[CD];
    float rr[CD];
#pragma unroll
    for (int I = 0; I < CD; ++I) {
        cidx[I] = a.col[tk.begin + 16 * I + i];
        rr[I] = a.rat[tk.begin + 16 * I + i];
    }
    f32x4 acc[Acc::NT];
#pragma unroll
    for (int p = 0; p < Acc::NT; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char* obase = (const char*)(opp + 8 * g);
    auto load = [&](int s, f32x8 (&y)[CD]) {
#pragma unroll
        for (int I = 0; I < CD; ++I)
            y[I] = *(const f32x8*)(obase + (uint32_t)cidx[I] * (uint32_t)(KP * sizeof(float)) + s * 128);
    };
    f32x8 yc[CD], yn[CD];
    load(0, yc);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) load(s + 1, yn);
        u32x4 H[CD], M[CD], L[CD];
        split_operands<CD>([&](int I, int e) { return yc[I][e]; }, H, M, L);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int I = 0; I < CD; ++I)
#pragma unroll
            for (int J = I; J < CD; ++J)   // the full six products on the diagonal too (no E fold on this path)
                split_tile_mfma<false>(acc[tile_index<CD>(I, J)], nullptr, H[I], M[I], L[I], H[J], M[J], L[J]);
        MFMA_DRAIN();
        if (s + 1 < NS) {
#pragma unroll
            for (int I = 0; I < CD; ++I) yc[I] = yn[I];
        }
    }
    // right-hand side r in the per-lane partial layout of solve_tiles (element j of block b on row g = 0)
    float rhs[CD];
#pragma unroll
    for (int b = 0; b < CD; ++b) rhs[b] = g == 0 ? rr[b] : 0.f;
    if constexpr (tiles_in_lds<CD>()) {   // CD = 6: 21 working tiles in per-wave LDS, as the KP = 128 primal solve
        LdsTiles T{tiles_lds[wave] + 4 * lane};
        RegStore<CD> A0;
#pragma unroll
        for (int p = 0; p < Acc::NT; ++p) T.put(p, acc[p]);
        solve_tiles<CD, true>(T, A0, rhs, buf, tk, a, lane);
    } else {
        RegTiles<CD> T{acc};
        RegStore<CD> A0;
        solve_tiles<CD, true>(T, A0, rhs, buf, tk, a, lane);
    }
    wave_sync();
    // m = Y^T alpha: lane l owns features l + 64 f; entries with alpha = 0 (padding, or exactly 0) are skipped
    float xo[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) xo[f] = 0.f;
#pragma unroll
    for (int I = 0; I < CD; ++I)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float al = buf[16 * I + e];
            const int c = __builtin_amdgcn_readlane(cidx[I], e);
            const float* row = opp + (int64_t)c * KP + lane;
#pragma unroll
            for (int f = 0; f < NF; ++f) xo[f] += row[64 * f] * al;
        }
    float* out = (float*)a.out + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)KP + lane;
#pragma unroll
    for (int f = 0; f < NF; ++f) out[64 * f] = (lane + 64 * f < a.k) ? xo[f] : 0.f;
}

// ---------------------------------------------------------------------------------------------------
// VALU Gram path (LDS-staged rows), fp32 and fp64
// ---------------------------------------------------------------------------------------------------
template <class T, int KP>
__global__ __launch_bounds__(256) void als_solve_valu(SolveArgs a) {
    constexpr int LPR = 64 / KP;            // lanes per Gram row
    constexpr int E = KP / LPR;             // Gram entries per lane (= KP*KP/64)
    constexpr int NWORDS = E + 1;           // + RHS
    constexpr int VN = Vec16<T>::N;         // elements per 16-B vector
    constexpr int V = KP / VN;              // 16-B vectors per factor row
    using VT = typename Vec16<T>::type;
    using L = WaveLds<T, KP, Path::VALU>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tid = blockIdx.x * WAVES + wave;
    if (tid >= a.n_tasks) return;
    const Task tk = load_task(a.tasks + tid);
    unsigned char* wl = smem + wave * L::BYTES;
    T* G = (T*)wl;
    T* stage = (T*)wl;   // aliases G: staging is dead before the Gram is canonicalised
    T* rhs_l = (T*)(wl + L::RHS_OFF);
    T* bc = (T*)(wl + L::BC_OFF);
    int32_t* sidx = (int32_t*)(wl + L::SIDX_OFF);
    T* srat = (T*)(wl + L::SRAT_OFF);

    const int arow = lane / LPR, c0 = (lane % LPR) * E;
    T acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = T(0);
    T rhs = T(0);

    T* part = (T*)a.partials;
    constexpr int SLOT_WORDS = NWORDS + 1;   // + integrity check word (SlotCodec)
    if (tk.kind == TASK_REDUCE) {
        bool bad = false;
        int32_t bad_slot = -1;
        for (int s = 0; s < tk.nsteps; ++s) {
            const T* src = part + (int64_t)(tk.slot + s) * (SLOT_WORDS * 64) + lane;
            SlotCodec cd{slot_key(a.gen, tk.slot + s, lane)};
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] += cd.dec(src[e * 64], e);
            rhs += cd.dec(src[E * 64], E);
            const bool ok = cd.check_ok(src[NWORDS * 64], NWORDS);
            if (!ok && !bad) bad_slot = tk.slot + s;
            bad |= !ok;
        }
        report_bad_slot(a.integrity, a.gen, bad_slot, tk.row, bad, lane);
    } else {
        const T* opp = (const T*)a.opp;
        const int n = (tk.nsteps + BLOCK_SUBSTEPS - 1) / BLOCK_SUBSTEPS * BLOCK_ENTRIES;   // task span
        for (int base = 0; base < n; base += RSTAGE) {
            const int e = base + lane;
            int idx = a.sentinel;
            T r = T(0);
            if (e < n) {
                idx = a.col[tk.begin + e];
                r = (T)a.rat[tk.begin + e];
            }
            sidx[lane] = idx;
            srat[lane] = r;
            wave_sync();
#pragma unroll
            for (int q = 0; q < V; ++q) {       // RSTAGE * V vectors, 64 per instruction
                const int pair = q * 64 + lane;
                const int t = pair / V, v = pair % V;
                const int id = sidx[t];   // padding entries gather the sentinel zero row
                *(VT*)(stage + t * KP + v * VN) = *(const VT*)(opp + (int64_t)id * KP + v * VN);
            }
            wave_sync();
            const int nt = (n - base) < RSTAGE ? (n - base) : RSTAGE;
            for (int t = 0; t < nt; ++t) {
                const T ya = stage[t * KP + arow];
#pragma unroll
                for (int e2 = 0; e2 < E; ++e2) acc[e2] += ya * stage[t * KP + c0 + e2];
                rhs += srat[t] * ya;
            }
            wave_sync();
        }
    }

    if (tk.kind == TASK_PARTIAL) {
        T* dst = part + (int64_t)tk.slot * (SLOT_WORDS * 64) + lane;
        SlotCodec cd{slot_key(a.gen, tk.slot, lane)};
#pragma unroll
        for (int e = 0; e < E; ++e) dst[e * 64] = cd.enc(acc[e], e);
        dst[E * 64] = cd.enc(rhs, E);
        dst[NWORDS * 64] = cd.check_word<T>(NWORDS);
        return;
    }

#pragma unroll
    for (int e = 0; e < E; ++e)
        if (c0 + e <= arow) G[tri(arow, 0) + c0 + e] = acc[e];   // packed lower triangle
    if (lane % LPR == 0) rhs_l[arow] = rhs;
    wave_sync();
    solve_store<T, KP>(G, rhs_l, bc, tk, a, lane);
}

// ---------------------------------------------------------------------------------------------------
// Squared-error reduction over observed ratings (RMSE numerator; scripts/calculate_mse.py:78-90)
// ---------------------------------------------------------------------------------------------------
template <class T, int KP>
__global__ __launch_bounds__(256) void als_sq_error_kernel(SqErrArgs a) {
    constexpr int VN = Vec16<T>::N;
    constexpr int LPE = KP / VN;            // lanes per entry (one 16-B piece each)
    constexpr int EPS = 64 / LPE;           // entries per wave step
    using VT = typename Vec16<T>::type;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tid = blockIdx.x * WAVES + wave;
    if (tid >= a.n_tasks) return;
    const Task tk = load_task(a.tasks + tid);
    const int es = lane / LPE, v = lane % LPE;
    const T* self = (const T*)a.self + factor_row(a.row_offset, a.rows_per_chunk, a.chunk_stride, tk.row) * (int64_t)KP;
    const T* opp = (const T*)a.opp;
    const VT x = *(const VT*)(self + v * VN);
    const int n = (tk.nsteps + BLOCK_SUBSTEPS - 1) / BLOCK_SUBSTEPS * BLOCK_ENTRIES;   // task span
    double se = 0.0;
    for (int base = 0; base < n; base += EPS) {
        const int e = base + es;
        int idx = a.sentinel;
        float r = 0.f;
        if (e < n) {
            idx = a.col[tk.begin + e];
            r = a.rat[tk.begin + e];
        }
        const VT y = *(const VT*)(opp + (int64_t)idx * KP + v * VN);
        T dot = T(0);
#pragma unroll
        for (int c = 0; c < VN; ++c) dot += x[c] * y[c];
#pragma unroll
        for (int m = 1; m < LPE; m <<= 1) dot += __shfl_xor(dot, m);
        // logical entry index of physical position e (block_position inverse): skip the padding
        const int w = e % BLOCK_ENTRIES;
        const int logical = e - w + (w % BLOCK_SUBSTEPS) * 4 + w / BLOCK_SUBSTEPS;
        if (v == 0 && e < n && logical < tk.nent) {
            const double d = (double)r - (double)dot;
            se += d * d;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) se += __shfl_xor(se, m);
    if (lane == 0) a.task_se[tid] = se;
}

// ---------------------------------------------------------------------------------------------------
// Collector prediction matrix (FeatureCollector.java:90-101): P[u][m] = sum_f U[u][f] * M[m][f] in fp32 with
// Java float semantics -- each product and each partial sum rounded separately, features in order (EJML
// MatrixMatrixMult_FDRM.multTransB's sequential dot; no FMA contraction) -- so that the CSV digits are the
// reference's. 16 x 16 cells per workgroup, the 16 + 16 factor rows staged in LDS.
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void als_predict_kernel(const T* __restrict__ U, const T* __restrict__ M, int kp,
                                                          int k, const int64_t* __restrict__ urows, int64_t n_u,
                                                          const int64_t* __restrict__ mrows, int64_t n_m,
                                                          float* __restrict__ out) {
    __shared__ float su[16][129], sm[16][129];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t u0 = (int64_t)blockIdx.y * 16, m0 = (int64_t)blockIdx.x * 16;
    for (int i = threadIdx.x; i < 16 * k; i += 256) {
        const int r = i / k, f = i % k;
        su[r][f] = (u0 + r < n_u) ? (float)U[urows[u0 + r] * kp + f] : 0.f;   // f64 factors reach the
        sm[r][f] = (m0 + r < n_m) ? (float)M[mrows[m0 + r] * kp + f] : 0.f;   // collector as floats
    }
    __syncthreads();
    const int64_t u = u0 + ty, m = m0 + tx;
    if (u >= n_u || m >= n_m) return;
    float total = 0.f;
    {
#pragma clang fp contract(off)
        for (int f = 0; f < k; ++f) total = total + su[ty][f] * sm[tx][f];   // rounded product, rounded sum
    }
    out[u * n_m + m] = total;
}

int blocks_for(int n_tasks) { return (n_tasks + WAVES - 1) / WAVES; }

// hipFuncAttributeMaxDynamicSharedMemorySize of one kernel on the current device, raised to `bytes` when a launch
// needs more than was set there before (engines of several devices and host threads launch concurrently: the
// per-(kernel, device) high-water mark is kept under a lock).
hipError_t ensure_dyn_lds(const void* fn, int bytes) {
    constexpr int MAXDEV = 64;
    static std::mutex mu;
    static std::vector<std::pair<const void*, std::vector<int>>> tab;   // per kernel: bytes set per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAXDEV) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> g(mu);
    std::vector<int>* set = nullptr;
    for (auto& x : tab)
        if (x.first == fn) set = &x.second;
    if (!set) {
        tab.emplace_back(fn, std::vector<int>(MAXDEV, 0));
        set = &tab.back().second;
    }
    if (bytes <= (*set)[dev]) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) (*set)[dev] = bytes;
    return e;
}

template <class T, int KP, Path P, int MINW = 1, bool PRESPLIT = false>
hipError_t launch_solve_t(const SolveArgs& a, hipStream_t s, bool reduce) {
    if (a.n_tasks <= 0) return hipSuccess;
    constexpr int bytes = WAVES * WaveLds<T, KP, P>::BYTES;
    if constexpr (P == Path::MFMA || P == Path::MFMA_SPLIT) {
        static_assert(std::is_same<T, float>::value, "MFMA paths are fp32");
        constexpr int nw = mfma_waves<KP>();
        const unsigned grid = (unsigned)((a.n_tasks + nw - 1) / nw);
        const size_t dyn = (size_t)a.extra_lds;   // debug build only: unused LDS per workgroup (occupancy sweeps)
        constexpr bool SPLIT = P == Path::MFMA_SPLIT;
        if (reduce) {   // one REDUCE kernel per KP: the partial slots have the same layout on every Gram path
            als_solve_mfma<KP, MINW, false, false, true><<<grid, 64 * nw, 0, s>>>(a);
        } else if constexpr (!PRESPLIT && SPLIT) {
            if (a.presplit_fallback)   // the range guard's fallback: grid-stride over a capped grid
                als_solve_mfma<KP, MINW, true, false, false, true>
                    <<<std::min<unsigned>(grid, (unsigned)std::max(1, a.grid_cap)), 64 * nw, dyn, s>>>(a);
            else
                als_solve_mfma<KP, MINW, true, false><<<grid, 64 * nw, dyn, s>>>(a);
        } else {
            als_solve_mfma<KP, MINW, SPLIT, PRESPLIT><<<grid, 64 * nw, dyn, s>>>(a);
        }
    } else {
        hipError_t e = ensure_dyn_lds((const void*)als_solve_valu<T, KP>, bytes);
        if (e != hipSuccess) return e;
        als_solve_valu<T, KP><<<blocks_for(a.n_tasks), 256, bytes, s>>>(a);
    }
    return hipGetLastError();
}

template <class T, int KP>
hipError_t launch_sq_t(const SqErrArgs& a, hipStream_t s) {
    if (a.n_tasks <= 0) return hipSuccess;
    als_sq_error_kernel<T, KP><<<blocks_for(a.n_tasks), 256, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace

// dst block i <- src block perm[i]: 32 columns + 32 ratings per block, one 64-lane wave per block (16 B per lane)
__global__ __launch_bounds__(256) void als_permute_blocks(const int32_t* __restrict__ col, const float* __restrict__ rat,
                                                         int32_t* __restrict__ col_out, float* __restrict__ rat_out,
                                                         const int32_t* __restrict__ perm, int64_t n_blocks) {
    const int64_t blk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= n_blocks) return;
    const int l = threadIdx.x & 63;
    const int64_t src = (int64_t)perm[blk] * BLOCK_ENTRIES;
    const int64_t dst = blk * BLOCK_ENTRIES;
    if (l < 8) ((u32x4*)(col_out + dst))[l] = ((const u32x4*)(col + src))[l];
    else if (l < 16) ((u32x4*)(rat_out + dst))[l - 8] = ((const u32x4*)(rat + src))[l - 8];
}
hipError_t launch_permute_blocks(const int32_t* col, const float* rat, int32_t* col_out, float* rat_out,
                                 const int32_t* perm, int64_t n_blocks, hipStream_t s) {
    if (n_blocks <= 0) return hipSuccess;
    als_permute_blocks<<<(unsigned)((n_blocks + 3) / 4), 256, 0, s>>>(col, rat, col_out, rat_out, perm, n_blocks);
    return hipGetLastError();
}


bool variant_available(int precision, int kp, Path path) {
    if (path == Path::GENERIC) return kp % 16 == 0 && kp <= 1024;
    if (precision == 0) {
        if (path == Path::MFMA || path == Path::MFMA_SPLIT) return kp == 32 || kp == 64 || kp == 128;
        return kp == 16 || kp == 32 || kp == 64;
    }
    return path == Path::VALU && (kp == 16 || kp == 32 || kp == 64);
}

int partial_words_per_lane(int precision, int kp, Path path) {
    if (path == Path::GENERIC) return 0;   // rows are never split on the generic path
    if (path == Path::MFMA || path == Path::MFMA_SPLIT) {
        const int c = kp / 16;
        return (c * (c + 1) / 2) * 4 + c + 1;   // accumulators + RHS + check word
    }
    return kp * kp / 64 + 1 + 1;
}

hipError_t launch_predict(int precision, const void* U, const void* M, int kp, int k, const int64_t* urows,
                          int64_t n_u, const int64_t* mrows, int64_t n_m, float* out, hipStream_t s) {
    if (n_u <= 0 || n_m <= 0) return hipSuccess;
    if (k > 128) {   // generic path: one thread per cell
        const int64_t cells = n_u * n_m;
        if ((cells + 255) / 256 > INT32_MAX) return hipErrorInvalidValue;
        const unsigned g = (unsigned)((cells + 255) / 256);
        if (precision == 0)
            als_predict_generic<float><<<g, 256, 0, s>>>((const float*)U, (const float*)M, kp, k, urows, n_u, mrows, n_m, out);
        else
            als_predict_generic<double><<<g, 256, 0, s>>>((const double*)U, (const double*)M, kp, k, urows, n_u, mrows,
                                                           n_m, out);
        return hipGetLastError();
    }
    if ((n_m + 15) / 16 > INT32_MAX || (n_u + 15) / 16 > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n_m + 15) / 16), (unsigned)((n_u + 15) / 16));
    if (precision == 0)
        als_predict_kernel<float><<<grid, 256, 0, s>>>((const float*)U, (const float*)M, kp, k, urows, n_u, mrows, n_m, out);
    else
        als_predict_kernel<double><<<grid, 256, 0, s>>>((const double*)U, (const double*)M, kp, k, urows, n_u, mrows, n_m,
                                                        out);
    return hipGetLastError();
}

// Host <-> device factor-table copies as KERNEL accesses: each lane moves 16 B between pinned host memory
// (zero-copy, non-temporal) and device memory, so the factor tables are only ever written and read through
// the same cache path as the solve kernels' own accesses (no SDMA engine in between). This keeps every access
// to a factor table on one documented ordering path: kernels on the engine's stream.
__global__ __launch_bounds__(256) void copy16(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int64_t n,
                                              int to_host) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (to_host) __builtin_nontemporal_store(src[i], dst + i);
        else dst[i] = __builtin_nontemporal_load(src + i);
    }
}

hipError_t launch_copy(const void* src, void* dst, size_t bytes, int to_host, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (bytes % 16 != 0) return hipErrorInvalidValue;
    const int64_t n = (int64_t)(bytes / 16);
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    copy16<<<(unsigned)blocks, 256, 0, s>>>((const u32x4*)src, (u32x4*)dst, n, to_host);
    return hipGetLastError();
}
hipError_t launch_upload(const void* host_pinned, void* dst, size_t bytes, hipStream_t s) {
    return launch_copy(host_pinned, dst, bytes, 0, s);
}
hipError_t launch_download(const void* src, void* host_pinned, size_t bytes, hipStream_t s) {
    return launch_copy(src, host_pinned, bytes, 1, s);
}

// r = rh + rm with rh = f16_rn(r), rm = r - rh: both exact fp16 for integers |r| <= 2^22 (every Java short)
__global__ __launch_bounds__(256) void als_pack_ratings(const float* __restrict__ rat, uint32_t* __restrict__ dst,
                                                        int64_t n_pairs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    unsigned h, m;
    split2(rat[2 * i], rat[2 * i + 1], h, m);
    dst[i] = h;
    dst[n_pairs + i] = m;
}
hipError_t launch_pack_ratings(const float* rat, uint32_t* dst, int64_t n_pairs, hipStream_t s) {
    if (n_pairs <= 0) return hipSuccess;
    als_pack_ratings<<<(unsigned)((n_pairs + 255) / 256), 256, 0, s>>>(rat, dst, n_pairs);
    return hipGetLastError();
}
template <int KP>
hipError_t launch_prepare_t(const float* src, void* dst, int64_t n_items, uint32_t* set, uint32_t* next_set,
                            uint32_t* pred, int cu_count, hipStream_t s) {
    const int cu = std::max(1, cu_count);
    // the scan: two 1024-thread workgroups per CU fill it (8 waves per SIMD), so at most 2 cu atomics per word
    const unsigned gs = (unsigned)std::min<int64_t>((n_items + 1023) / 1024, 2 * cu);
    als_presplit_scan<KP><<<gs, 1024, 0, s>>>(src, (unsigned*)dst, n_items, pred, set);
    // confirm / repair: a capped grid, as the range guard's fallback (its waves nearly always exit at once)
    const unsigned gc = (unsigned)std::min<int64_t>((n_items + 255) / 256, 4 * cu);
    als_presplit_confirm<KP><<<gc, 256, 0, s>>>(src, (unsigned*)dst, n_items, set, next_set, pred);
    return hipGetLastError();
}
hipError_t launch_presplit_prepare(int kp, const float* src, void* dst, int64_t n_rows, uint32_t* set,
                                   uint32_t* next_set, uint32_t* pred, int cu_count, hipStream_t s) {
    if (n_rows <= 0) return hipErrorInvalidValue;   // the sentinel row is always there
    const int64_t n_items = n_rows * 2 * (kp / 16);
    if (kp == 64) return launch_prepare_t<64>(src, dst, n_items, set, next_set, pred, cu_count, s);
    if (kp == 128) return launch_prepare_t<128>(src, dst, n_items, set, next_set, pred, cu_count, s);
    return hipErrorInvalidValue;   // the pre-split Gram is built for KP = 64 and 128
}
hipError_t launch_pack_cols_ps(const int32_t* col, int32_t* dst, int64_t n_entries, hipStream_t s) {
    if (n_entries <= 0) return hipSuccess;
    if (n_entries % BLOCK_ENTRIES) return hipErrorInvalidValue;
    als_pack_cols_ps<<<(unsigned)((n_entries + 255) / 256), 256, 0, s>>>(col, dst, n_entries);
    return hipGetLastError();
}

hipError_t launch_dual(int kp, int cd, const SolveArgs& a, hipStream_t s) {
    if (a.n_tasks <= 0) return hipSuccess;
    const unsigned grid = (unsigned)blocks_for(a.n_tasks);
    if (kp == 64 && cd == 2) als_solve_dual<64, 2><<<grid, 64 * WAVES, 0, s>>>(a);
    else if (kp == 128 && cd == 2) als_solve_dual<128, 2><<<grid, 64 * WAVES, 0, s>>>(a);
    else if (kp == 128 && cd == 4) als_solve_dual<128, 4><<<grid, 64 * WAVES, 0, s>>>(a);
    else if (kp == 128 && cd == 6) als_solve_dual<128, 6><<<grid, 64 * WAVES, 0, s>>>(a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_solve(int precision, int kp, Path path, const SolveArgs& a, hipStream_t s, bool presplit,
                        bool reduce) {
    if (path == Path::GENERIC) return reduce ? hipErrorInvalidValue : launch_generic(precision, kp, a, s);
    if (precision == 0) {
        // occupancy (waves per SIMD) per variant: KP <= 64 two, the pre-split KP = 64 Gram four (PS64_WAVES),
        // KP = 128 one
        if (path == Path::MFMA) {
            if (kp == 32) return launch_solve_t<float, 32, Path::MFMA, 2>(a, s, reduce);
            if (kp == 64) return launch_solve_t<float, 64, Path::MFMA, 2>(a, s, reduce);
            if (kp == 128) return launch_solve_t<float, 128, Path::MFMA, 1>(a, s, reduce);
        } else if (path == Path::MFMA_SPLIT) {
            if (kp == 32) return launch_solve_t<float, 32, Path::MFMA_SPLIT, 2>(a, s, reduce);
            if (kp == 64 && presplit) return launch_solve_t<float, 64, Path::MFMA_SPLIT, PS64_WAVES, true>(a, s, reduce);
            if (kp == 64) return launch_solve_t<float, 64, Path::MFMA_SPLIT, 2>(a, s, reduce);
            if (kp == 128 && presplit) return launch_solve_t<float, 128, Path::MFMA_SPLIT, 1, true>(a, s, reduce);
            if (kp == 128) return launch_solve_t<float, 128, Path::MFMA_SPLIT, 1>(a, s, reduce);
        } else {
            if (kp == 16) return launch_solve_t<float, 16, Path::VALU>(a, s, reduce);
            if (kp == 32) return launch_solve_t<float, 32, Path::VALU>(a, s, reduce);
            if (kp == 64) return launch_solve_t<float, 64, Path::VALU>(a, s, reduce);
        }
    } else if (path == Path::VALU) {
        if (kp == 16) return launch_solve_t<double, 16, Path::VALU>(a, s, reduce);
        if (kp == 32) return launch_solve_t<double, 32, Path::VALU>(a, s, reduce);
        if (kp == 64) return launch_solve_t<double, 64, Path::VALU>(a, s, reduce);
    }
    return hipErrorInvalidValue;
}

template <class T, bool L>
hipError_t launch_generic_t(const GenericPlan& p, int kp, const SolveArgs& a, hipStream_t s) {
    hipError_t e = ensure_dyn_lds((const void*)als_solve_generic<T, L>, (int)p.lds_bytes);
    if (e != hipSuccess) return e;
    int64_t grid = std::min<int64_t>(a.n_tasks, 4096);
    if (!L) grid = std::min<int64_t>(grid, a.scratch_slabs);
    if (grid <= 0) return hipErrorInvalidValue;
    als_solve_generic<T, L><<<(unsigned)grid, 256, (size_t)p.lds_bytes, s>>>(a, kp, p.batch, (T*)a.partials,
                                                                             p.slab_elems);
    return hipGetLastError();
}

hipError_t launch_generic(int precision, int kp, const SolveArgs& a, hipStream_t s) {
    if (a.n_tasks <= 0) return hipSuccess;
    if (kp > GENERIC_MAX_KP || kp % 16) return hipErrorInvalidValue;
    const GenericPlan p = generic_plan(precision, kp);
    if (precision == 0)
        return p.g_in_lds ? launch_generic_t<float, true>(p, kp, a, s) : launch_generic_t<float, false>(p, kp, a, s);
    return p.g_in_lds ? launch_generic_t<double, true>(p, kp, a, s) : launch_generic_t<double, false>(p, kp, a, s);
}

hipError_t launch_sq_error(int precision, int kp, const SqErrArgs& a, hipStream_t s) {
    if (kp > 128 || (precision == 1 && kp > 64)) {   // generic path
        if (a.n_tasks <= 0) return hipSuccess;
        if (precision == 0) als_sq_error_generic<float><<<blocks_for(a.n_tasks), 256, 0, s>>>(a, kp);
        else als_sq_error_generic<double><<<blocks_for(a.n_tasks), 256, 0, s>>>(a, kp);
        return hipGetLastError();
    }
    if (precision == 0) {
        if (kp == 16) return launch_sq_t<float, 16>(a, s);
        if (kp == 32) return launch_sq_t<float, 32>(a, s);
        if (kp == 64) return launch_sq_t<float, 64>(a, s);
        if (kp == 128) return launch_sq_t<float, 128>(a, s);
    } else {
        if (kp == 16) return launch_sq_t<double, 16>(a, s);
        if (kp == 32) return launch_sq_t<double, 32>(a, s);
        if (kp == 64) return launch_sq_t<double, 64>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace cfk
