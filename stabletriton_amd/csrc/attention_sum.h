// The weighted sum over key/value segments that the regional kernel (attention_regions.hip) and the ragged segmented kernel
// (attention_segments.hip) share: which elements of st_attention's fp16 epilogue are rounded once from the exact product, and the
// single-rounding conversion that gives those bits back (see the file comment of attention_regions.hip).  Internal to csrc/.
#pragma once
#include "attention_core.h"

constexpr int REGIONS_MAX = 8;             // segments per launch, both kernels

// elements (of every four consecutive head-dim values a lane stores) that st_attention's fp16 epilogue rounds once from the exact
// product o * inv
template <typename E> struct RegionsOut { static constexpr bool fused(int) { return false; } };
template <> struct RegionsOut<f16> { static constexpr bool fused(int e) { return e == 0 || e == 3; } };

// binary16(a + c) with ONE rounding: v_fma_mixlo_f16 on fp32 sources
__device__ __forceinline__ f16 fma_mix_f16(float a, float c) {
    unsigned r = 0;
    asm("v_fma_mixlo_f16 %0, %1, %2, %3" : "+v"(r) : "v"(a), "v"(1.0f), "v"(c));
    return __builtin_bit_cast(f16, (unsigned short)r);
}
template <typename E> __device__ __forceinline__ E regions_round(float a, float c);
template <> __device__ __forceinline__ bf16 regions_round<bf16>(float a, float) { return (bf16)a; }
template <> __device__ __forceinline__ f16 regions_round<f16>(float a, float c) { return fma_mix_f16(a, c); }

// acc += w * (o * inv) for the lane's 16 values of one segment, with the products' residuals for the fused fp16 elements.
// (The regional kernel keeps these statements and the store below inline: routed through these functions it compiled to another
// register allocation and schedule, and its instruction stream is pinned.  Same arithmetic, statement for statement.)
template <typename E>
__device__ __forceinline__ void regions_accumulate(f32x4 (&acc)[4], f32x4 (&res)[4], const f32x4 (&o)[5], float inv, float w) {
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = o[db][e] * inv;
            acc[db][e] = __builtin_fmaf(w, x, acc[db][e]);
            if constexpr (RegionsOut<E>::fused(0) || RegionsOut<E>::fused(1) || RegionsOut<E>::fused(2) || RegionsOut<E>::fused(3))
                if (RegionsOut<E>::fused(e)) res[db][e] = __builtin_fmaf(w, __builtin_fmaf(o[db][e], inv, -x), res[db][e]);
        }
}

// the lane's 16 values, rounded once, to row `orow` (head offset applied) of the output
template <typename E>
__device__ __forceinline__ void regions_store(E* orow, const f32x4 (&acc)[4], const f32x4 (&res)[4], int g) {
    typedef typename V16<E>::x4 E4;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        E4 a_;
#pragma unroll
        for (int e = 0; e < 4; ++e) a_[e] = RegionsOut<E>::fused(e) ? regions_round<E>(acc[db][e], res[db][e]) : (E)acc[db][e];
        *reinterpret_cast<E4*>(orow + 16 * db + 4 * g) = a_;
    }
}
