// Positional encoding of the deformation network (models/modules.py:874-922 `get_embedder` / `Embedder`), shared by
// csrc/deform.hip and the host shim tests/hostmath_deform_shim.hip.
//   [v, sin(2^0 v), cos(2^0 v), sin(2^1 v), cos(2^1 v), ...] with every function applied to all D input dims together.
// The argument is v * 2^k (exact in fp32: the frequencies 2.**linspace(0, L-1, L) are exact powers of two), so it is the one torch
// forms; sinf / cosf are the accurate library functions (full range reduction), never __sinf / v_sin_f32 and never a double-angle
// recursion (its error doubles with every octave; arguments reach 512 |v|).
#pragma once
#include <math.h>

namespace bds {

constexpr int kDfMultires = 10;                          // x_multires = t_multires = 10 (every shipped config)
constexpr int kDfXEmb = 3 * (1 + 2 * kDfMultires);       // 63
constexpr int kDfTEmb = 1 * (1 + 2 * kDfMultires);       // 21

// column c of the encoding of a D-dim input v (c < D * (1 + 2 L))
template <int D>
__host__ __device__ inline float df_embed_col(const float *v, int c) {
  if (c < D) return v[c];
  const int k = (c - D) / (2 * D), r = (c - D) % (2 * D);
  const float a = v[r % D] * (float)(1 << k);
  return r < D ? sinf(a) : cosf(a);
}

}  // namespace bds
