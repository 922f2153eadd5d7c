// Private part of als_kernels.hip: the partial slots of split rows -- the keyed word codec with its check word,
// the integrity report, and the MFMA paths' slot store and fixed-order slot sum.
#pragma once

#include "als_mfma.h"

namespace cfk {
namespace {

// ---------------------------------------------------------------------------------------------------
// Partial-slot integrity. A PARTIAL task stores word w of lane l of slot s as bits ^ key(gen, s, l, w) plus
// one check word (the wrap-around sum of the plain words); its REDUCE task decodes with the SAME launch
// generation and re-sums. A slot line the REDUCE cannot see freshly written -- never written, left over
// from an earlier launch (which, on identical inputs, would hold identical numbers and be invisible to any
// comparison of results), or torn -- decodes to noise and fails the check; the failure is counted in
// SolveArgs::integrity and the engine's next synchronising call reports it (ALS_ERR_INTEGRITY).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t slot_key(uint32_t gen, int32_t slot, int lane) {
    return mix32(gen * 0x9e3779b1u ^ mix32((uint32_t)slot * 64u + (uint32_t)lane));
}
constexpr uint32_t WORD_KEY_STEP = 0x632be5abu;
struct SlotCodec {
    uint32_t key, sum = 0;
    __device__ __forceinline__ float enc(float v, int w) {
        const uint32_t b = __float_as_uint(v);
        sum += b;
        return __uint_as_float(b ^ (key + (uint32_t)w * WORD_KEY_STEP));
    }
    __device__ __forceinline__ float dec(float v, int w) {
        const uint32_t b = __float_as_uint(v) ^ (key + (uint32_t)w * WORD_KEY_STEP);
        sum += b;
        return __uint_as_float(b);
    }
    __device__ __forceinline__ double enc(double v, int w) {
        const uint64_t b = (uint64_t)__double_as_longlong(v);
        sum += (uint32_t)b + (uint32_t)(b >> 32);
        const uint64_t k = key + (uint32_t)w * WORD_KEY_STEP;
        return __longlong_as_double((long long)(b ^ (k | (k << 32))));
    }
    __device__ __forceinline__ double dec(double v, int w) {
        const uint64_t k = key + (uint32_t)w * WORD_KEY_STEP;
        const uint64_t b = (uint64_t)__double_as_longlong(v) ^ (k | (k << 32));
        sum += (uint32_t)b + (uint32_t)(b >> 32);
        return __longlong_as_double((long long)b);
    }
    // check word (element w of the slot), stored keyed like the data words
    template <class T>
    __device__ __forceinline__ T check_word(int w) const {
        const uint32_t c = sum ^ (key + (uint32_t)w * WORD_KEY_STEP);
        if constexpr (sizeof(T) == 4) return __uint_as_float(c);
        else return __longlong_as_double((long long)(uint64_t)c);
    }
    template <class T>
    __device__ __forceinline__ bool check_ok(T stored, int w) const {
        uint32_t c;
        if constexpr (sizeof(T) == 4) c = __float_as_uint(stored);
        else c = (uint32_t)(uint64_t)__double_as_longlong(stored);
        return (c ^ (key + (uint32_t)w * WORD_KEY_STEP)) == sum;
    }
};
// Vector-memory atomics only, from the first failing lane (slot = the first slot that lane found bad).
__device__ __forceinline__ void report_bad_slot(uint32_t* rec, uint32_t gen, int32_t slot, int32_t row, bool bad,
                                                int lane) {
    const uint64_t m = __ballot(bad);
    if (m == 0) return;
    if (lane == (int)__builtin_ctzll(m)) {
        const uint32_t n = atomicAdd(rec, 1u);
        if (n == 0) {
            atomicExch(rec + 1, gen);
            atomicExch(rec + 2, (uint32_t)slot);
            atomicExch(rec + 3, (uint32_t)row);
        }
    }
}

// A PARTIAL task's raw accumulators -> its partial slot ([word][lane], keyed words + check word, SlotCodec).
template <int C>
__device__ __forceinline__ void store_partial(const SolveArgs& a, const Task& tk, const MfmaAcc<C>& acc, int lane) {
    using Acc = MfmaAcc<C>;
    constexpr int SLOT_WORDS = Acc::NWORDS + 1;   // + integrity check word
    float* dst = (float*)a.partials + (int64_t)tk.slot * (SLOT_WORDS * 64) + lane;
    SlotCodec cd{slot_key(a.gen, tk.slot, lane)};
#pragma unroll
    for (int p = 0; p < Acc::NT; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(p * 4 + r) * 64] = cd.enc(acc.g[p][r], p * 4 + r);
#pragma unroll
    for (int c = 0; c < C; ++c) dst[(Acc::NT * 4 + c) * 64] = cd.enc(acc.rhs[c], Acc::NT * 4 + c);
    dst[Acc::NWORDS * 64] = cd.check_word<float>(Acc::NWORDS);
}

// A REDUCE task: fixed-order sum of the row's partial slots ([word][lane] layout, coalesced) into acc, each decoded
// and checked.
template <int C>
__device__ __forceinline__ void sum_partial_slots(const SolveArgs& a, const Task& tk, MfmaAcc<C>& acc, int lane) {
    using Acc = MfmaAcc<C>;
    constexpr int SLOT_WORDS = Acc::NWORDS + 1;   // + integrity check word
    float* part = (float*)a.partials;
    bool bad = false;
    int32_t bad_slot = -1;
    for (int s = 0; s < tk.nsteps; ++s) {
        const float* src = part + (int64_t)(tk.slot + s) * (SLOT_WORDS * 64) + lane;
        SlotCodec cd{slot_key(a.gen, tk.slot + s, lane)};
        // the whole slot's loads are issued before the first use: left to the scheduler under the KP = 128
        // register pressure they went out one at a time (load, wait, add: 0.44 ms for 974 rows). Streaming loads: a
        // slot is read once, by this wave alone (the k = 64 movie REDUCE 0.049 -> 0.045 ms; the stores of
        // store_partial measured no gain with the same policy and keep the default)
        float w[SLOT_WORDS];
#pragma unroll
        for (int q = 0; q < SLOT_WORDS; ++q) w[q] = load_stream<CachePolicy::slot_loads>(src + q * 64);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < Acc::NT; ++p)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc.g[p][r] += cd.dec(w[p * 4 + r], p * 4 + r);
#pragma unroll
        for (int c = 0; c < C; ++c) acc.rhs[c] += cd.dec(w[Acc::NT * 4 + c], Acc::NT * 4 + c);
        const bool ok = cd.check_ok(w[Acc::NWORDS], Acc::NWORDS);
        if (!ok && !bad) bad_slot = tk.slot + s;
        bad |= !ok;
    }
    report_bad_slot(a.integrity, a.gen, bad_slot, tk.row, bad, lane);
}

}  // namespace
}  // namespace cfk
