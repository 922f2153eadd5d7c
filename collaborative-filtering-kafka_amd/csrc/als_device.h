// Private part of als_kernels.hip: the wave-level vocabulary every kernel uses -- vector types, same-wave LDS
// hand-off, lane broadcasts, static_for, the optimiser fences opaque / pin, and the wave-uniform task load.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "als_internal.h"

namespace cfk {
namespace {

constexpr int WAVES = 4;       // waves (tasks) per 256-thread workgroup
constexpr int RSTAGE = 64;     // VALU path: rows staged per LDS block

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <class T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<double> { typedef f64x2 type; static constexpr int N = 2; };

template <int C> struct VecC;
template <> struct VecC<2> { typedef f32x2 type; };
template <> struct VecC<4> { typedef f32x4 type; };
template <> struct VecC<8> { typedef f32x8 type; };

// Same-wave LDS hand-off: the hardware keeps one wave's DS operations in order; this only stops the
// compiler from moving LDS accesses across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float bcast(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}
__device__ __forceinline__ double bcast(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(unsigned)(b & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// Compile-time loop: f(std::integral_constant<int, i>) for i in [B, E). Every index derived from i is a
// constant expression, so register arrays are never indexed dynamically (no scratch).
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}
// Fresh copy of a per-lane value the optimizer cannot see through: stops LLVM from CSE-ing the 3*KP
// lane-vs-step comparisons of the unrolled solve into live SGPR masks (which spill).
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
// Materialise a value here: keeps LLVM from sinking a step's rank-1 updates into deferred FMA chains at the
// next use (MachineSink ignores sched_barrier), which multiplies live registers in the unrolled solve.
__device__ __forceinline__ void pin(float& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(double& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(unsigned& v) { asm volatile("" : "+v"(v)); }

// A load of data its launch touches exactly once, under the buffer's policy (CachePolicy, als_internal.h): STREAM sets
// the access's `nt` bit and nothing else -- width, alignment and address form are those of the plain load.
template <bool STREAM, class T>
__device__ __forceinline__ T load_stream(const T* p) {
    if constexpr (STREAM) return __builtin_nontemporal_load(p);
    else return *p;
}

__device__ __forceinline__ Task load_task(const Task* p) {
    Task t = *p;
    t.begin = ((int64_t)uni((int)(t.begin >> 32)) << 32) | (int64_t)(uint32_t)uni((int)(uint32_t)t.begin);
    t.nsteps = uni(t.nsteps);
    t.row = uni(t.row);
    t.slot = uni(t.slot);
    t.ndeg = uni(t.ndeg);
    t.kind = uni(t.kind);
    return t;
}

}  // namespace
}  // namespace cfk
