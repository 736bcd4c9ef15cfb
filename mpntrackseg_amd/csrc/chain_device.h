// Device helpers shared by the chain kernels of both families (edge_chain.hip, edge_chain_bf16_common.h, row_stage.h): the vector
// types of the MFMA operands and the masked 16-byte row pieces.  (The constexpr min / max: chain_layout.h.)
#pragma once
#include <hip/hip_runtime.h>

namespace mpnhip {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// 16-byte piece of a feature row at column n (n % 4 == 0, dim % 4 == 0): zero beyond the real width
template <bool EXACT>
__device__ __forceinline__ float4 ldrow(const float* row, int n, int dim) {
    if (EXACT) return ldg4(row + n);  // widths are multiples of 32: nothing to mask
    const bool ok = n < dim;
    float4 v = ldg4(row + (ok ? n : 0));
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
}
template <bool EXACT>
__device__ __forceinline__ void strow(float* row, int n, int dim, float4 v, bool ok) {
    if (ok && (EXACT || n < dim)) *reinterpret_cast<float4*>(row + n) = v;
}

// the same through a (scalar) base pointer and a 32-bit element offset: one address register per row instead of two
template <bool EXACT>
__device__ __forceinline__ float4 ldrow(const float* base, unsigned off, int n, int dim) {
    // (base + zext(off)) + n: scalar base, 32-bit register offset, n in the instruction's immediate field
    if (EXACT) return ldg4(base + (size_t)off + n);
    const bool ok = n < dim;
    float4 v = ldg4(base + (size_t)off + (ok ? n : 0));
    v.x = ok ? v.x : 0.f; v.y = ok ? v.y : 0.f; v.z = ok ? v.z : 0.f; v.w = ok ? v.w : 0.f;
    return v;
}
template <bool EXACT>
__device__ __forceinline__ void strow(float* base, unsigned off, int n, int dim, float4 v, bool ok) {
    // (plain stores: a row's 128-byte lines are completed by several wave instructions and L2 merges the pieces; non-temporal
    // stores / loads here took the bf16 forward kernel from 0.63 to 0.92 ms at cfg-E)
    if (ok && (EXACT || n < dim)) *reinterpret_cast<float4*>(base + (size_t)off + n) = v;
}

// D tile rows of register group g (registers 4g..4g+3): n = 8g + 4h + (0..3)
__device__ __forceinline__ float4 get4(const f32x16& a, int g) {
    return make_float4(a[4 * g + 0], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]);
}
__device__ __forceinline__ void relu16(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = fmaxf(a[r], 0.f);
}

}  // namespace

}  // namespace mpnhip
