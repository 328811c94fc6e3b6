// Per-element math of the lidar scene preparation (datasets/driving_dataset.py:280-416, 496-603, 644-727 and
// datasets/base/pixel_source.py:77-92), used by csrc/lidar.hip and by the host shim tests/hostmath_lidar_shim.hip.
//   row        one row of a [3,4] matrix against [p;1]: ((m0*x + m1*y) + m2*z) + m3, every product and sum rounded on its own (no
//              fused multiply-add), so that the three passes of the projection take the same pixel for a point and the host shim
//              gives the kernels' bits
//   project    q = M[p;1], z = q.z, u = q.x / (z + 1e-6f), v = q.y / (z + 1e-6f); valid iff 0 <= u < W and 0 <= v < H and z > 0;
//              the pixel is ((int)v, (int)u), truncation as torch's .long()
//   box        o = w2o[p;1]; inside iff -half < o < half on every axis (strict, as the reference's mask)
//   window     output cell i of an area resize H -> Ho covers [floor(i H / Ho), ceil((i + 1) H / Ho))
//   downsample (sum / n) / (cnt / n) over a window of n = kh * kw values, sum over all of them in row-major order, cnt those above
//              1e-3; 0 where cnt is 0.  Each division by n is taken as / kh / kw, as torch's adaptive average pool takes it on the
//              host: bit-equal to the reference there
#pragma once
#include "gs_math.h"

namespace bds {

constexpr float kLidarDepthEps = 1e-6f;      // driving_dataset.py:594,691
constexpr float kLidarHitMin = 1e-3f;        // pixel_source.py:86

BDS_HD float lidar_row(const float *m, float x, float y, float z) {
#pragma clang fp contract(off)
  const float a = m[0] * x, b = m[1] * y, c = m[2] * z;
  return ((a + b) + c) + m[3];
}

// M: row-major [3,4].  Returns the validity; *px, *py the pixel (defined only when valid), *depth = z.
BDS_HD bool lidar_project(const float *M, float x, float y, float z, int W, int H, int *px, int *py, float *depth) {
#pragma clang fp contract(off)
  const float qx = lidar_row(M, x, y, z), qy = lidar_row(M + 4, x, y, z), qz = lidar_row(M + 8, x, y, z);
  const float den = qz + kLidarDepthEps;
  const float u = qx / den, v = qy / den;
  *depth = qz;
  const bool valid = u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H && qz > 0.0f;      // (false for a NaN)
  *px = valid ? (int)u : 0;
  *py = valid ? (int)v : 0;
  return valid;
}

// w2o: row-major [3,4], half: [3].  o receives the point in the box's frame.
BDS_HD bool lidar_in_box(const float *w2o, const float *half, float x, float y, float z, float *o) {
  o[0] = lidar_row(w2o, x, y, z);
  o[1] = lidar_row(w2o + 4, x, y, z);
  o[2] = lidar_row(w2o + 8, x, y, z);
  return o[0] > -half[0] && o[0] < half[0] && o[1] > -half[1] && o[1] < half[1] && o[2] > -half[2] && o[2] < half[2];
}

BDS_HD int lidar_window_start(int i, int in, int out) { return (int)(((long long)i * in) / out); }
BDS_HD int lidar_window_end(int i, int in, int out) { return (int)((((long long)i + 1) * in + out - 1) / out); }

// One output cell of the sparse depth-map downsampler.  map: [H,W] row-major.
BDS_HD float lidar_downsample_cell(const float *map, int H, int W, int Ho, int Wo, int i, int j) {
#pragma clang fp contract(off)
  const int r0 = lidar_window_start(i, H, Ho), r1 = lidar_window_end(i, H, Ho);
  const int c0 = lidar_window_start(j, W, Wo), c1 = lidar_window_end(j, W, Wo);
  float sum = 0.0f, cnt = 0.0f;
  for (int r = r0; r < r1; r++)
    for (int c = c0; c < c1; c++) {
      const float v = map[(long long)r * W + c];
      sum += v;
      cnt += v > kLidarHitMin ? 1.0f : 0.0f;
    }
  const float kh = (float)(r1 - r0), kw = (float)(c1 - c0);
  return cnt > 0.0f ? ((sum / kh) / kw) / ((cnt / kh) / kw) : 0.0f;
}

}  // namespace bds
