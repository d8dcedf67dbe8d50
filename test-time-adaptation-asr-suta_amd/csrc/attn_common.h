// Device helpers shared by the flash attention kernels (attn.hip: head dim 64; attn_wide.hip: head dims 72 .. 128).
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

typedef __bf16 fbf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 fbf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ fbf16x8 cvt8(f32x4 lo, f32x4 hi) {
    fbf16x8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = (__bf16)lo[j];
        v[4 + j] = (__bf16)hi[j];
    }
    return v;
}

// accumulator register v of a 32x32 MFMA tile holds row r8(v, h) of column (lane & 31)
__device__ __forceinline__ int r8(int v, int h) { return 8 * (v >> 2) + 4 * h + (v & 3); }

// 1-D XCD-aware renumbering (cdna_hip_programming.md T1, bijective): consecutive logical blocks (the
// query or key blocks of one head) run on one XCD and share its L2.
__device__ __forceinline__ int xcd_block() {
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// max / sum with the other half-wave's value (lane l and l ^ 32) through v_permlane32_swap (no LDS round trip, as
// __shfl_xor's ds_bpermute is): swapping two copies of x leaves {x[l], x[l + 32]} in the lower half's pair and
// {x[l - 32], x[l]} in the upper's, so one op of the pair is op(x[l], x[l ^ 32]) -- bitwise the shuffle form (fmax
// and a two-term sum are commutative)
__device__ __forceinline__ float half_swap_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_swap_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

constexpr float LOG2E = 1.4426950408889634f;

}  // namespace
