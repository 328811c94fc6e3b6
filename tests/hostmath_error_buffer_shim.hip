// TEST-ONLY host shim of the error-driven sampler's pixel formula (csrc/error_buffer_math.h, the function the kernel of
// csrc/error_buffer.hip runs) on the CPU, so that tests/test_error_buffer_cpu.py can compare it with the numpy restatement and the
// reference's recorded maps without a GPU.  Not part of libbds.so, never loaded by the product.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/error_buffer_math.h"

using namespace bds;

// pred, gt [n,3], dyn [n] or NULL -> e [n]
extern "C" void hm_eb_map(int64_t n, const float *pred, const float *gt, const float *dyn, float *e) {
  for (int64_t i = 0; i < n; i++)
    e[i] = eb_pixel(pred[3 * i], pred[3 * i + 1], pred[3 * i + 2], gt[3 * i], gt[3 * i + 1], gt[3 * i + 2], dyn != nullptr,
                    dyn != nullptr ? dyn[i] : 0.0f);
}

// the kernel's running minimum and maximum over e [n], from +inf and -inf
extern "C" void hm_eb_range(int64_t n, const float *e, float *lo, float *hi) {
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = 0; i < n; i++) {
    mn = eb_min(mn, e[i]);
    mx = eb_max(mx, e[i]);
  }
  *lo = mn;
  *hi = mx;
}
