// TEST-ONLY host shim of the evaluation metrics' per-pixel math (csrc/metrics_math.h, the functions the kernels of csrc/metrics.hip run)
// on the CPU, so that tests/test_metrics_cpu.py can compare the SSIM map with the float64 restatement without a GPU.  Not part of
// libbds.so, never loaded by the product.  The sums are taken in the kernel's order: seven taps along a row, then seven row sums down a
// column.
#include "../bilateral_driving_amd/csrc/metrics_math.h"

using namespace bds;

extern "C" void hm_metrics_map(int H, int W, const float *pred, const float *gt, float *map) {
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++)
      for (int ch = 0; ch < 3; ch++) {
        double m[kSsimMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int r = -kSsimPad; r <= kSsimPad; r++) {
          double row[kSsimMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
          const int sy = metrics_reflect(y + r, H);
          for (int c = -kSsimPad; c <= kSsimPad; c++) {
            const long o = ((long)sy * W + metrics_reflect(x + c, W)) * 3 + ch;
            metrics_tap(pred[o], gt[o], row);
          }
          for (int j = 0; j < kSsimMoments; j++) m[j] += row[j];
        }
        map[((long)y * W + x) * 3 + ch] = metrics_ssim(m);
      }
}

extern "C" int hm_metrics_reflect(int i, int n) { return metrics_reflect(i, n); }
extern "C" double hm_metrics_psnr(double sq_err, double n_values) { return metrics_psnr(sq_err, n_values); }
