// TEST-ONLY host shim of a view's input preparation (csrc/pixels_math.h, the functions the kernels of csrc/pixels.hip run) on the CPU,
// so that tests/test_get_image_cpu.py can compare the rays, the coordinates and the two resizes with the numpy restatement and the
// reference's recorded results without a GPU.  Not part of libbds.so, never loaded by the product.  The loops follow the kernels:
// the resize runs the width pass for every input row, then the height pass, each sum tap by tap.
#include <stdint.h>

#include <vector>

#include "../bilateral_driving_amd/csrc/pixels_math.h"

using namespace bds;

// one view: viewdirs, origins [H,W,3], norm [H,W], coords [H,W,2], intrinsics_out [9]
extern "C" void hm_px_view(const float *c2w, const float *K, float scale, int H, int W, float *origins, float *viewdirs, float *norm,
                           float *coords, float *intrinsics_out) {
  const PxCamera c = px_camera(c2w, K, scale);
  for (int k = 0; k < 9; k++) intrinsics_out[k] = px_scaled_intrinsic(K, scale, k);
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const long long p = (long long)y * W + x;
      px_ray(c, x, y, viewdirs + 3 * p, norm + p);
      px_coords(x, y, H, W, coords + 2 * p);
      for (int i = 0; i < 3; i++) origins[3 * p + i] = c.t[i];
    }
}

// the window of output i: returns n, *lo its first tap, w [px_aa_max_taps(scale)] its normalised weights
extern "C" int hm_px_aa_window(int i, double factor, int in, int *lo, float *w) {
  const float scale = (float)(1.0 / factor);
  return px_aa_weights(i, scale, in, px_aa_max_taps(scale), lo, w);
}

extern "C" int hm_px_aa_max_taps(double factor) { return px_aa_max_taps((float)(1.0 / factor)); }

// bds_image_resize_aa on host arrays: in [H,W,3] -> out [Ho,Wo,3]
extern "C" void hm_px_resize_aa(int H, int W, int Ho, int Wo, double factor, const float *in, float *out) {
#pragma clang fp contract(off)
  const float scale = (float)(1.0 / factor);
  const int cap = px_aa_max_taps(scale);
  std::vector<float> w(cap), mid((size_t)H * Wo * 3);
  for (int ox = 0; ox < Wo; ox++) {
    int lo;
    const int n = px_aa_weights(ox, scale, W, cap, &lo, w.data());
    for (int r = 0; r < H; r++)
      for (int ch = 0; ch < 3; ch++) {
        float acc = 0.0f;
        for (int j = 0; j < n; j++) acc += w[j] * in[((size_t)r * W + lo + j) * 3 + ch];
        mid[((size_t)r * Wo + ox) * 3 + ch] = acc;
      }
  }
  for (int oy = 0; oy < Ho; oy++) {
    int lo;
    const int n = px_aa_weights(oy, scale, H, cap, &lo, w.data());
    for (int e = 0; e < Wo * 3; e++) {
      float acc = 0.0f;
      for (int j = 0; j < n; j++) acc += w[j] * mid[(size_t)(lo + j) * Wo * 3 + e];
      out[(size_t)oy * Wo * 3 + e] = acc;
    }
  }
}

// bds_masks_resize_nearest for one mask
extern "C" void hm_px_resize_nearest(int H, int W, int Ho, int Wo, double factor, const float *in, float *out) {
  const float scale = (float)(1.0 / factor);
  for (int oy = 0; oy < Ho; oy++)
    for (int ox = 0; ox < Wo; ox++) out[(size_t)oy * Wo + ox] = in[(size_t)px_nearest(oy, scale, H) * W + px_nearest(ox, scale, W)];
}
