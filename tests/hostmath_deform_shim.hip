// TEST-ONLY host shim of the deformation network's positional encoding (csrc/deform_math.h df_embed_col, the function the kernels
// of csrc/deform.hip run) on the CPU, so that tests/test_deform_network_cpu.py can compare it with float64 without a GPU.  Not part of
// libbds.so, never loaded by the product.
#include "../bilateral_driving_amd/csrc/deform_math.h"

using namespace bds;

// v [n, dims] (dims 3: x, 1: t) -> out [n, dims * 21]
extern "C" void hm_deform_embed(int n, int dims, const float *v, float *out) {
  const int cols = dims * (1 + 2 * kDfMultires);
  for (int i = 0; i < n; i++)
    for (int c = 0; c < cols; c++) out[i * cols + c] = dims == 3 ? df_embed_col<3>(v + i * 3, c) : df_embed_col<1>(v + i, c);
}
