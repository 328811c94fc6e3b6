// Per-pixel math of the lens undistortion (cv2.undistort as CameraData.load_images, load_egocar_mask, load_dynamic_masks and
// load_sky_masks call it, datasets/base/pixel_source.py:249-256,273-278,296-303,319-326,342-349,366-373), used by csrc/undistort.hip
// and by the host shim tests/hostmath_undistort_shim.hip.  OpenCV 4.x's published algorithm, restated: initUndistortRectifyMap's
// map in double, remap's INTER_LINEAR on the 1/32-pixel grid with 15-bit integer weights, a constant 0 border.  PARITY UNPINNED: no
// OpenCV where this is built.  Every double operation is rounded on its own (no fused multiply-add) and the divisions are IEEE, so
// the host shim gives the kernel's bits.
//   cam [18]   fx, fy, u0, v0 | k1, k2, p1, p2, k3 | ir[0..8] = inverse(new camera matrix), row-major, formed on the host
//   map        (_x, _y, _w) = ir (j, i, 1);  x = _x / _w, y = _y / _w;  r2 = x x + y y;  kr = 1 + ((k3 r2 + k2) r2 + k1) r2
//              xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x);  yd = y kr + p1 (r2 + 2 y y) + p2 (2 x y);  u = fx xd + u0, v = fy yd + v0
//   grid       iu = rint(32 u), iv = rint(32 v), half to even, saturated to int32; sx = iu >> 5, ax = iu & 31 (floor and its rest,
//              also for a negative iu), the same for sy, ay
//   weights    w00 = (32 - ay)(32 - ax) 32, w01 = (32 - ay) ax 32, w10 = ay (32 - ax) 32, w11 = ay ax 32: they sum to 32768
//   value      (S00 w00 + S01 w01 + S10 w10 + S11 w11 + 16384) >> 15 per channel; a tap outside the image is 0, and so is the pixel
//              when sx >= W, sx + 1 < 0, sy >= H or sy + 1 < 0
#pragma once
#include <math.h>
#include <stdint.h>

#include "gs_math.h"

namespace bds {

constexpr int kUdCamDoubles = 18;
constexpr int kUdMaxExtent = 32767;      // H and W at most: a source coordinate beyond that counts as outside

// the source position (u = column, v = row) of output pixel (row i, column j)
BDS_HD void ud_map(const double *cam, int i, int j, double *u, double *v) {
#pragma clang fp contract(off)
  const double fx = cam[0], fy = cam[1], u0 = cam[2], v0 = cam[3];
  const double k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7], k3 = cam[8];
  const double *ir = cam + 9;
  const double dj = (double)j, di = (double)i;
  const double _x = (dj * ir[0] + di * ir[1]) + ir[2];
  const double _y = (dj * ir[3] + di * ir[4]) + ir[5];
  double x = _x, y = _y;
  if (!(ir[6] == 0.0 && ir[7] == 0.0 && ir[8] == 1.0)) {      // (an affine new matrix: _w is 1 exactly, and t / 1 = t; the same for every
    const double _w = (dj * ir[6] + di * ir[7]) + ir[8];      // pixel of a frame, so a wave never diverges here)
    x = _x / _w;
    y = _y / _w;
  }
  const double x2 = x * x, y2 = y * y;
  const double r2 = x2 + y2, _2xy = (2.0 * x) * y;
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy;
  *u = fx * xd + u0;
  *v = fy * yd + v0;
}

// rint(32 t), half to even, saturated to int32 (a NaN: the lowest value, far outside)
BDS_HD int32_t ud_fixed(double t) {
#pragma clang fp contract(off)
  const double s = rint(t * 32.0);
  if (!(s > -2147483648.0)) return INT32_MIN;
  if (s >= 2147483647.0) return INT32_MAX;
  return (int32_t)s;
}

struct UdTaps {
  int32_t sx, sy;                 // the upper left tap
  int32_t w00, w01, w10, w11;     // (row, column) = (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)
};

BDS_HD UdTaps ud_taps(double u, double v) {
  const int32_t iu = ud_fixed(u), iv = ud_fixed(v);
  const int32_t ax = iu & 31, ay = iv & 31;
  UdTaps t;
  t.sx = iu >> 5;
  t.sy = iv >> 5;
  t.w00 = (32 - ay) * (32 - ax) * 32;
  t.w01 = (32 - ay) * ax * 32;
  t.w10 = ay * (32 - ax) * 32;
  t.w11 = ay * ax * 32;
  return t;
}

// no tap of the window lies inside a W x H image
BDS_HD bool ud_outside(const UdTaps &t, int H, int W) { return t.sx >= W || t.sx + 1 < 0 || t.sy >= H || t.sy + 1 < 0; }

BDS_HD int32_t ud_blend(const UdTaps &t, int32_t s00, int32_t s01, int32_t s10, int32_t s11) {
  return (s00 * t.w00 + s01 * t.w01 + s10 * t.w10 + s11 * t.w11 + 16384) >> 15;
}

// the C channels of a pixel that is not ud_outside: frame [H,W,C] bytes, zero border.  H, W <= kUdMaxExtent and C <= 3, so a byte's
// offset inside its frame fits 32 bits (unsigned: the arithmetic may pass through a wrapped value for a tap that is not read).
template <int C>
BDS_HD void ud_sample(const UdTaps &t, const uint8_t *frame, int H, int W, int32_t *value) {
  const bool x0 = t.sx >= 0, x1 = t.sx + 1 < W;      // (not outside: sx in [-1, W - 1], sy in [-1, H - 1])
  const bool y0 = t.sy >= 0, y1 = t.sy + 1 < H;
  const uint32_t p00 = ((uint32_t)t.sy * (uint32_t)W + (uint32_t)t.sx) * C, p10 = p00 + (uint32_t)W * C;
  for (int ch = 0; ch < C; ch++) {
    const int32_t s00 = (y0 && x0) ? frame[p00 + ch] : 0;
    const int32_t s01 = (y0 && x1) ? frame[p00 + C + ch] : 0;
    const int32_t s10 = (y1 && x0) ? frame[p10 + ch] : 0;
    const int32_t s11 = (y1 && x1) ? frame[p10 + C + ch] : 0;
    value[ch] = ud_blend(t, s00, s01, s10, s11);
  }
}

// the three output forms of a blended value 0..255
// the image stack's ``/ 255``: the correctly rounded quotient (float)value / 255.0f, formed without a division -- the rounded
// reciprocal's product, its exact remainder by one fused multiply-add, one correction (equal for all 256 values: tested)
BDS_HD float ud_unit(int32_t value) {
#pragma clang fp contract(off)
  const float v = (float)value, r = 1.0f / 255.0f;
  const float q = v * r;
  return fmaf(fmaf(-q, 255.0f, v), r, q);
}
BDS_HD float ud_mask(int32_t value) { return value > 0 ? 1.0f : 0.0f; }    // the masks' ``> 0`` then ``.float()``

}  // namespace bds
