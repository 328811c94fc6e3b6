// The one pixel formula of the error-driven image sampler (CameraData.update_image_error_maps, datasets/base/pixel_source.py:431-449,
// behind render_images' clamp of every rgb result, models/video_utils.py:185-187), used by csrc/error_buffer.hip and by the host shim
// tests/hostmath_error_buffer_shim.hip.  All of it is float32, every operation rounded on its own: the host shim gives the kernel's bits.
//   pixel   e = ((|g0 - c0| + |g1 - c1|) + |g2 - c2|) / 3 with c = clamp(p, 0, 1): ``abs(gt - pred).mean(-1)`` of the clamped render;
//           gt is not clamped; e * 5 where dyn > 0.1f, strictly (:446).  A NaN in p or g gives a NaN e, as torch.clamp and abs do.
//   min/max propagate a NaN from either side, as torch's do.
#pragma once
#include <math.h>

#include "gs_math.h"

namespace bds {

constexpr float kEbDynThreshold = 0.1f;      // pixel_source.py:446
constexpr float kEbDynBoost = 5.0f;

BDS_HD float eb_clamp01(float p) { return p < 0.0f ? 0.0f : (p > 1.0f ? 1.0f : p); }      // (both compares false for a NaN: it stays)

// p, g: the pixel's three channels; has_dyn: whether the view has a dynamic opacity at all
BDS_HD float eb_pixel(float p0, float p1, float p2, float g0, float g1, float g2, bool has_dyn, float dyn) {
#pragma clang fp contract(off)
  float e = ((fabsf(g0 - eb_clamp01(p0)) + fabsf(g1 - eb_clamp01(p1))) + fabsf(g2 - eb_clamp01(p2))) / 3.0f;
  if (has_dyn && dyn > kEbDynThreshold) e = e * kEbDynBoost;
  return e;
}

BDS_HD float eb_min(float a, float b) { return (a != a || a < b) ? a : b; }
BDS_HD float eb_max(float a, float b) { return (a != a || a > b) ? a : b; }

}  // namespace bds
