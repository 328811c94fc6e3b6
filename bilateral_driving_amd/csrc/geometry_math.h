// Per-element math of the evaluation geometry metrics (models/video_utils.py:363-536, utils/chamfer_distance.py:34-75), used by
// csrc/geometry.hip and by the host shim tests/hostmath_geometry_shim.hip.
//   validity   hit = gt > 0 and not egocar; valid = hit and 0.01 < gt < 80 and 1e-4 < pred < 80 (float32 comparisons, as torch
//              compares a float32 tensor with a Python number)
//   unproject  pixel (v, u), depth z -> ((u - cx) z / fx, (v - cy) z / fy, z, 1) through camera_to_world, float32, true division
//   pair       the squared Euclidean distance (norm 2) or the sum of absolute differences (norm 1) from the coordinate DIFFERENCES:
//              the expanded form |x|^2 + |y|^2 - 2 x.y loses centimetres at world coordinates of 10^2 - 10^3 m
//   trim       k = int(n * q) as Python forms it (one IEEE double product, truncated); the mean of the k smallest of non-negative
//              floats from a rank select on their bit patterns: sum(values below the threshold) + (k - count below) * threshold
#pragma once
#include "gs_math.h"

namespace bds {

constexpr int kGeoClasses = 5;      // sky, dynamic, human, vehicle, background
constexpr int kGeoGroups = 1 + kGeoClasses;      // the whole frame, then the classes
constexpr int kGeoTrims = 3;        // 0.99, 0.97, 0.95

BDS_HD bool geo_valid(float pred, float gt, bool egocar) {
  const bool hit = gt > 0.0f && !egocar;
  return hit && gt > 0.01f && gt < 80.0f && pred > 0.0001f && pred < 80.0f;
}

// bit 0: valid; bits 1..5: valid and in the class (background = in none of the four masks)
BDS_HD unsigned geo_flags(bool valid, bool sky, bool dynamic, bool human, bool vehicle) {
  if (!valid) return 0u;
  const bool background = !(sky || dynamic || human || vehicle);
  return 1u | (sky ? 2u : 0u) | (dynamic ? 4u : 0u) | (human ? 8u : 0u) | (vehicle ? 16u : 0u) | (background ? 32u : 0u);
}

// K: the row-major 3x3 intrinsics; c2w: the row-major 4x4 camera-to-world (its first three rows are read)
BDS_HD void geo_unproject(int u, int v, float z, const float *K, const float *c2w, float *out) {
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float x = ((float)u - cx) * z / fx, y = ((float)v - cy) * z / fy;
#pragma unroll
  for (int r = 0; r < 3; r++) out[r] = fmaf(c2w[4 * r + 2], z, fmaf(c2w[4 * r + 1], y, c2w[4 * r] * x)) + c2w[4 * r + 3];
}

template <int NORM>
BDS_HD float geo_pair(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  if (NORM == 1) return (fabsf(dx) + fabsf(dy)) + fabsf(dz);
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// int(n * q) for q = 0.99, 0.97, 0.95 (which = 0, 1, 2)
BDS_HD long long geo_trim_count(long long n, int which) {
  const double q = which == 0 ? 0.99 : (which == 1 ? 0.97 : 0.95);
  return (long long)((double)n * q);
}

BDS_HD unsigned geo_bits(float v) {
  union { float f; unsigned u; } c;
  c.f = v;
  return c.u;
}
BDS_HD float geo_from_bits(unsigned u) {
  union { float f; unsigned u; } c;
  c.u = u;
  return c.f;
}

// One step of the radix select over 8-bit digits, most significant first: `hist` counts the digit at `shift` among the values whose
// higher digits equal `prefix`; the element of rank `rank` (0-based, among those values) lies in the returned digit, and `rank`
// becomes its rank inside that digit.
BDS_HD unsigned geo_select_digit(const unsigned *hist, unsigned long long *rank) {
  unsigned long long r = *rank;
  unsigned d = 0;
  while (d < 255u && r >= hist[d]) r -= hist[d++];
  *rank = r;
  return d;
}

// sum and sum of squares of the k smallest from those strictly below the threshold (sum_below, sq_below, count_below)
BDS_HD void geo_trimmed(double sum_below, double sq_below, unsigned long long count_below, unsigned long long k, float threshold,
                        double *sum, double *sq) {
  const double t = (double)threshold, m = (double)(k - count_below);
  *sum = k > count_below ? sum_below + m * t : sum_below;
  *sq = k > count_below ? sq_below + m * (t * t) : sq_below;
}

}  // namespace bds
