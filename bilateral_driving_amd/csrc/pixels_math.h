// Per-element math of a view's input preparation (CameraData.get_image, datasets/base/pixel_source.py:477-657, get_rays :38-75 and
// ScenePixelSource.prepare_novel_view_render_data :1070-1132), used by csrc/pixels.hip and by the host shim
// tests/hostmath_pixels_shim.hip.  All of it is float32, every operation rounded on its own (no fused multiply-add): the host shim
// gives the kernels' bits.
//   camera     fx = K[0][0] scale, fy = K[1][1] scale, cx = K[0][2] scale, cy = K[1][2] scale, as ``intrinsics * downscale_factor``
//              (:625); the returned intrinsics are K scale with [2][2] = 1 (:626)
//   ray        dx = ((x - cx) + 0.5) / fx, dy = ((y - cy) + 0.5) / fy, dz = 1 (:59-60); dir_i = (dx R[i][0] + dy R[i][1]) + R[i][2]
//              (:69); n = sqrt((d0 d0 + d1 d1) + d2 d2) (:72); viewdirs = dir / (n + 1e-8) (:74); origins = c2w[:3,3] (:70)
//   coords     (float(y) / float(H), float(x) / float(W)): row first (:515-519)
//   aa window  torch's antialiased resize of one axis (:492-502): scale = 1 / s, support = 2 scale, c = scale (i + 0.5),
//              lo = max(0, int(c - support + 0.5)), n = min(in, int(c + support + 0.5)) - lo, weight j = cubic((j + lo - c + 0.5) / scale)
//              with Keys' a = -0.5, divided by the window's sum
//   nearest    source index min(int(floorf(dst scale)), in - 1) (:523-579, torch's mode="nearest" with a scale_factor)
#pragma once
#include <math.h>

#include "gs_math.h"

namespace bds {

constexpr float kPxNormEps = 1e-8f;      // pixel_source.py:74

struct PxCamera {
  float fx, fy, cx, cy;
  float R[9];      // c2w[:3,:3], row-major
  float t[3];      // c2w[:3,3]
};

// c2w: row-major [4,4]; K: row-major [3,3], unscaled
BDS_HD PxCamera px_camera(const float *c2w, const float *K, float scale) {
#pragma clang fp contract(off)
  PxCamera c;
  c.fx = K[0] * scale;
  c.fy = K[4] * scale;
  c.cx = K[2] * scale;
  c.cy = K[5] * scale;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) c.R[3 * i + j] = c2w[4 * i + j];
    c.t[i] = c2w[4 * i + 3];
  }
  return c;
}

BDS_HD float px_scaled_intrinsic(const float *K, float scale, int k) {
#pragma clang fp contract(off)
  return k == 8 ? 1.0f : K[k] * scale;
}

// viewdirs [3] and the direction's norm of pixel (x = column, y = row)
BDS_HD void px_ray(const PxCamera &c, int x, int y, float *viewdir, float *norm) {
#pragma clang fp contract(off)
  const float dx = (((float)x - c.cx) + 0.5f) / c.fx;
  const float dy = (((float)y - c.cy) + 0.5f) / c.fy;
  float d[3];
  for (int i = 0; i < 3; i++) {
    const float a = dx * c.R[3 * i], b = dy * c.R[3 * i + 1];
    d[i] = (a + b) + c.R[3 * i + 2];
  }
  const float q0 = d[0] * d[0], q1 = d[1] * d[1], q2 = d[2] * d[2];
  const float n = sqrtf((q0 + q1) + q2);
  const float den = n + kPxNormEps;
  viewdir[0] = d[0] / den;
  viewdir[1] = d[1] / den;
  viewdir[2] = d[2] / den;
  *norm = n;
}

BDS_HD void px_coords(int x, int y, int H, int W, float *rc) {
  rc[0] = (float)y / (float)H;
  rc[1] = (float)x / (float)W;
}

// Keys' cubic convolution kernel, a = -0.5, in the form torch evaluates it
BDS_HD float px_cubic(float x) {
#pragma clang fp contract(off)
  const float A = -0.5f;
  x = fabsf(x);
  if (x < 1.0f) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  if (x < 2.0f) return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  return 0.0f;
}

// the taps [lo, lo + n) of output i on an axis of ``in`` samples; scale = (float)(1 / s) >= 1
BDS_HD void px_aa_window(int i, float scale, int in, int *lo, int *n) {
#pragma clang fp contract(off)
  const float support = 2.0f * scale;
  const float c = scale * ((float)i + 0.5f);
  const int a = (int)((c - support) + 0.5f), b = (int)((c + support) + 0.5f);
  *lo = a > 0 ? a : 0;
  *n = (b < in ? b : in) - *lo;
}

// an upper bound of n for any output of the axis: what the kernels size their weight rows by
BDS_HD int px_aa_max_taps(float scale) { return (int)(4.0f * scale) + 3; }

// the unnormalised weight of tap j of output i's window
BDS_HD float px_aa_weight(int i, int j, int lo, float scale) {
#pragma clang fp contract(off)
  const float c = scale * ((float)i + 0.5f);
  return px_cubic(((((float)(j + lo)) - c) + 0.5f) / scale);
}

// the n normalised weights of output i into w (n <= cap; a longer window is cut: the kernels never write past a row)
BDS_HD int px_aa_weights(int i, float scale, int in, int cap, int *lo_out, float *w) {
#pragma clang fp contract(off)
  int lo, n;
  px_aa_window(i, scale, in, &lo, &n);
  n = n < 0 ? 0 : (n > cap ? cap : n);
  float total = 0.0f;
  for (int j = 0; j < n; j++) {
    w[j] = px_aa_weight(i, j, lo, scale);
    total += w[j];
  }
  for (int j = 0; j < n; j++) w[j] = w[j] / total;
  *lo_out = lo;
  return n;
}

BDS_HD int px_nearest(int dst, float scale, int in) {
#pragma clang fp contract(off)
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

}  // namespace bds
