// Per-element math of the pseudo-lidar generation (generate_lidar/generate_lidar_from_depth.py:42-162, generate_lidar/depth2lidar.py:41-90),
// used by csrc/pseudo_lidar.hip and by the host shim tests/hostmath_pseudo_lidar_shim.hip.
//   unproject  xc = ((u - cx) * d) / fx, yc = ((v - cy) * d) / fy, zc = d in float32, every operation rounded on its own (the
//              reference's expression order, :134-136); valid iff d > 0 && d < max_depth (false for a NaN, :128)
//   to lidar   one [3,4] float32 matrix through lidar_row (no fused multiply-add): the bin pass and the resolve pass, and the host
//              shim, get the same bits
//   crop       lo <= p < hi on every axis (:152-157); the limits are doubles, the widened float32 coordinate is compared
//   beam       in double from the widened float32 coordinates, as the reference's numpy part (:56-82, :13-30):
//              d = sqrt((x x + y y) + z z), r = sqrt(x x + y y), each 1e-6 where it is 0; phi = rad45 - asin(y / r),
//              column = trunc(phi / dphi) clamped to [0, W-1]; vertical: theta = asin(z / d), kept iff theta0 <= theta <= fov_up,
//              row = trunc((theta - theta0) / dtheta) clamped to [0, H-1]; classic: theta = theta0 - asin(z / d), row =
//              trunc(theta / dtheta) clamped, no filter.  Divisions stay divisions, by the caller's own doubles; the clamp is taken in
//              double, in front of the conversion.
#pragma once
#include <math.h>

#include "lidar_math.h"

namespace bds {

// the table of doubles every entry takes (include/bds.h BDS_PSEUDO_LIDAR_BEAMS)
enum { kPlRad45 = 0, kPlDphi, kPlTheta0, kPlFovUp, kPlDtheta, kPlCrop /* x0 x1 y0 y1 z0 z1 */, kPlMaxDepth = kPlCrop + 6, kPlBeams };
enum { kPlVertical = 0, kPlClassic = 1 };
constexpr int kPlCamFloats = 16;      // fx fy cx cy | the [3,4] camera-to-lidar matrix

BDS_HD bool pl_unproject(const float *cam, int u, int v, float d, double max_depth, float *pc) {
#pragma clang fp contract(off)
  const float a = ((float)u - cam[2]) * d, b = ((float)v - cam[3]) * d;
  pc[0] = a / cam[0];
  pc[1] = b / cam[1];
  pc[2] = d;
  return d > 0.0f && (double)d < max_depth;
}

BDS_HD void pl_to_lidar(const float *cam, const float *pc, float *p) {
  p[0] = lidar_row(cam + 4, pc[0], pc[1], pc[2]);
  p[1] = lidar_row(cam + 8, pc[0], pc[1], pc[2]);
  p[2] = lidar_row(cam + 12, pc[0], pc[1], pc[2]);
}

BDS_HD bool pl_crop(const double *beams, const float *p) {
  const double *c = beams + kPlCrop;
  return p[0] >= c[0] && p[0] < c[1] && p[1] >= c[2] && p[1] < c[3] && p[2] >= c[4] && p[2] < c[5];
}

BDS_HD int pl_clamp_trunc(double t, int n) {      // trunc(t) clamped to [0, n-1]; a NaN goes to 0
  const double hi = (double)(n - 1);
  t = !(t >= 0.0) ? 0.0 : (t > hi ? hi : t);
  return (int)t;
}

// -> the beam's cell row * W + col, or -1 for a point the vertical rule drops
BDS_HD int pl_beam(const double *beams, int H, int W, int mode, const float *p) {
#pragma clang fp contract(off)
  const double x = p[0], y = p[1], z = p[2];
  const double xx = x * x, yy = y * y, zz = z * z;
  double d = sqrt((xx + yy) + zz), r = sqrt(xx + yy);
  if (d == 0.0) d = 0.000001;
  if (r == 0.0) r = 0.000001;
  const double phi = beams[kPlRad45] - asin(y / r);
  const int col = pl_clamp_trunc(phi / beams[kPlDphi], W);
  const double el = asin(z / d);
  int row;
  if (mode == kPlVertical) {
    if (!(el >= beams[kPlTheta0] && el <= beams[kPlFovUp])) return -1;
    row = pl_clamp_trunc((el - beams[kPlTheta0]) / beams[kPlDtheta], H);
  } else {
    row = pl_clamp_trunc((beams[kPlTheta0] - el) / beams[kPlDtheta], H);
  }
  return row * W + col;
}

// A depth pixel's whole way: -> its cell or -1; p the lidar coordinates (defined for a valid depth)
BDS_HD int pl_pixel_cell(const float *cam, const double *beams, int H, int W, int mode, int u, int v, float d, float *p) {
  float pc[3];
  if (!pl_unproject(cam, u, v, d, beams[kPlMaxDepth], pc)) return -1;
  pl_to_lidar(cam, pc, p);
  if (!pl_crop(beams, p)) return -1;
  return pl_beam(beams, H, W, mode, p);
}

// A cloud row's way: p = (x, y, z, intensity)
BDS_HD int pl_point_cell(const double *beams, int crop, int H, int W, int mode, const float *p) {
  if (crop && !pl_crop(beams, p)) return -1;
  return pl_beam(beams, H, W, mode, p);
}

}  // namespace bds
