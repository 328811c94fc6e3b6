// The FP32 matrix-core tile vocabulary shared by the GEMM-shaped kernels (mlp_head.hip, deform.hip).
#pragma once

namespace bds {

// One 32 x 32 D tile of v_mfma_f32_32x32x2_f32 over the wave: lane l holds column l & 31; its register r holds row
// d_row(r, l >> 5) -- four consecutive rows per register group, the two lane halves interleaved in groups of four.
typedef float acc16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ constexpr int d_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

__device__ __forceinline__ acc16 zero16() {
  acc16 z;
#pragma unroll
  for (int r = 0; r < 16; r++) z[r] = 0.f;
  return z;
}

// D = A B + C, two k steps: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
__device__ __forceinline__ acc16 mfma(float a, float b, acc16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

}  // namespace bds
