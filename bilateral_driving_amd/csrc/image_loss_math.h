// Per-pixel math of the trainer's image loss in one pass each way (BasicTrainer.compute_losses, models/trainers/base.py:518-585,
// 638-652, with the loss functions of models/losses.py:33-178), used by the image-loss section of csrc/loss.hip and by the host shim
// tests/hostmath_image_loss_shim.hip.  valid = 1 - egocar (or 1).  The six terms:
//   0 rgb L1 (:533-540)              |pixels*valid - rgb*valid|, mean over 3P
//   1 sky opacity (:536-550)         x = opacity*valid, y = (1 - sky)*valid; torch's binary_cross_entropy (losses.py:81-83: logs clamped
//                                    at -100, backward (x - y) / max((1 - x) x, 1e-12)) or SafeBCE (losses.py:33-79), mean over P
//   2 lidar depth (:552-565)         DepthLoss (losses.py:91-178): hit = (lidar > 0)*valid, pred = depth*hit, gt = lidar*hit, over
//                                    {gt > 0.01, gt < max_depth, pred > 1e-4}: optional clamp(d / max_depth, 1e-6, 1), optional 1 / d, then
//                                    l1 / l2 / smooth_l1 (beta 1); mean over the set, over P, or the sum
//   3 opacity entropy (:568-573)     p = clamp(opacity, 1e-6, 1 - 1e-6); -p log p, mean over P
//   4 inverse-depth smoothness (:576-585)  kornia.losses.inverse_depth_smoothness_loss -- an external package, PARITY UNPINNED, restated from
//                                    its published definition: id = 1 / (depth + 1e-5); mean |(id[x] - id[x+1]) * exp(-mean_c |img[x] -
//                                    img[x+1]|)| over (H, W-1) + the same along y over (H-1, W); the reference repeats id to three equal
//                                    channels (:575-582), which leaves the mean unchanged
//   5 dynamic-region L1 (:638-652)   |pixels*valid - rgb*valid| over {dyn_opacity > threshold (detached), valid != 0}, mean over 3 x their
//                                    count
// A torch.clamp passes the gradient on its closed range; |t| has derivative sign(t) with sign(0) = 0.
// losses.pixel_loss is terms 0-2 as the trainer's defaults build them (:230-250: binary_cross_entropy, DepthLoss(normalize=False,
// use_inverse_depth=False, reduction="mean_on_hit")), PINNED by tests/golden/pixel_loss_*.npz (generated with the reference's own
// functions); losses.reg_losses is terms 3-5 unweighted (:566-585, 638-659).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef BDS_HD
#define BDS_HD __host__ __device__ __forceinline__
#endif

namespace bds {

enum ImageLossMask { kIlMaskOff = 0, kIlMaskBce = 1, kIlMaskSafeBce = 2 };
enum ImageLossDepth { kIlDepthL1 = 0, kIlDepthL2 = 1, kIlDepthSmoothL1 = 2 };
enum ImageLossReduction { kIlMeanOnHit = 0, kIlMeanOnHw = 1, kIlSum = 2 };
constexpr int kIlTerms = 6;
// a row of sums: [0] rgb, [1] mask, [2] depth numerator, [3] entropy, [4] x-smoothness, [5] y-smoothness, [6] dynamic numerator,
// [7] depth count, [8] dynamic count (the two counts are int32 bit patterns in the workgroups' rows and floats in the finished row)
constexpr int kIlSums = 9, kIlFloatSums = 7, kIlDepthCount = 7, kIlDynCount = 8;

struct ImageLossArgs {
  const float *rgb, *pixels, *opacity, *depth, *sky, *lidar, *egocar, *dyn_opacity;
  int H, W;
  int mask_kind;                              // ImageLossMask
  float ln_limit, limit, one_minus_limit;     // SafeBCE: ln(limit), exp(ln(limit)) and 1 - that, each formed in double and rounded once
  int depth_type, normalize, inverse, reduction;
  float max_depth;
  int entropy, smoothness;
  float dyn_threshold;
  float w[kIlTerms];
};

BDS_HD float il_sign(float t) { return t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f); }
BDS_HD float il_clip(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- term 1 -----------------------------------------------------------------------------------------------------------------------
BDS_HD float il_bce(float x, float y) { return (y - 1.f) * fmaxf(logf(1.f - x), -100.f) - y * fmaxf(logf(x), -100.f); }
BDS_HD float il_bce_grad(float x, float y) { return (x - y) / fmaxf((1.f - x) * x, 1e-12f); }

BDS_HD float il_safe_bce(float x, float y, float ln_limit) {
  x = il_clip(x, 0.f, 1.f);
  y = il_clip(y, 0.f, 1.f);
  return -(y == 0.f ? fmaxf(logf(1.f - x), ln_limit) : fmaxf(logf(x), ln_limit));
}
// SafeBCE.backward: x re-clipped to [0, 1 - limit] where y == 0 and to [limit, 1] otherwise; zero only where that x equals y
BDS_HD float il_safe_bce_grad(float x, float y, float limit, float one_minus_limit) {
  x = il_clip(x, 0.f, 1.f);
  y = il_clip(y, 0.f, 1.f);
  x = y == 0.f ? il_clip(x, 0.f, one_minus_limit) : il_clip(x, limit, 1.f);
  const float g = y == 0.f ? 1.f / (1.f - x) : -1.f / x;
  return x == y ? 0.f : g;
}

BDS_HD float il_mask(const ImageLossArgs &a, float x, float y) {
  return a.mask_kind == kIlMaskSafeBce ? il_safe_bce(x, y, a.ln_limit) : il_bce(x, y);
}
BDS_HD float il_mask_grad(const ImageLossArgs &a, float x, float y) {
  return a.mask_kind == kIlMaskSafeBce ? il_safe_bce_grad(x, y, a.limit, a.one_minus_limit) : il_bce_grad(x, y);
}

// ---- term 2 -----------------------------------------------------------------------------------------------------------------------
// normalize / inverse of one depth -> the value the error is taken of; *dd = its derivative to d
BDS_HD float il_depth_form(const ImageLossArgs &a, float d, float *dd) {
  float g = 1.f;
  if (a.normalize) {
    const float q = d / a.max_depth;
    g = (q >= 1e-6f && q <= 1.f) ? 1.f / a.max_depth : 0.f;
    d = il_clip(q, 1e-6f, 1.f);
  }
  if (a.inverse) {
    const float r = 1.f / d;
    g *= -(r * r);
    d = r;
  }
  *dd = g;
  return d;
}
// one pixel of the depth term: false outside the valid set; *value the error's loss, *grad its derivative to depth[i]
BDS_HD bool il_depth(const ImageLossArgs &a, float depth, float lidar, float valid, float *value, float *grad) {
  const float hit = (lidar > 0.f ? 1.f : 0.f) * valid, pred = depth * hit, gt = lidar * hit;
  if (!(gt > 0.01f && gt < a.max_depth && pred > 0.0001f)) return false;
  float dp, dg;
  const float e = il_depth_form(a, pred, &dp) - il_depth_form(a, gt, &dg);
  float v, g;
  if (a.depth_type == kIlDepthL2) {
    v = e * e;
    g = 2.f * e;
  } else if (a.depth_type == kIlDepthSmoothL1 && fabsf(e) < 1.f) {
    v = 0.5f * e * e;
    g = e;
  } else {
    v = fabsf(e) - (a.depth_type == kIlDepthSmoothL1 ? 0.5f : 0.f);
    g = il_sign(e);
  }
  *value = v;
  *grad = g * dp * hit;
  return true;
}

// ---- term 3 -----------------------------------------------------------------------------------------------------------------------
BDS_HD float il_entropy(float o) {
  const float p = il_clip(o, 1e-6f, 1.f - 1e-6f);
  return -p * logf(p);
}
BDS_HD float il_entropy_grad(float o) { return (o >= 1e-6f && o <= 1.f - 1e-6f) ? -(logf(o) + 1.f) : 0.f; }

// ---- term 4 -----------------------------------------------------------------------------------------------------------------------
BDS_HD float il_inv_depth(const float *depth, int p) { return 1.f / (depth[p] + 1e-5f); }
// exp(-mean_c |img[p] - img[q]|)
BDS_HD float il_edge_weight(const float *pixels, int p, int q) {
  const float *a = pixels + (int64_t)p * 3, *b = pixels + (int64_t)q * 3;
  return expf(-((fabsf(a[0] - b[0]) + fabsf(a[1] - b[1]) + fabsf(a[2] - b[2])) / 3.f));
}
// pixel p = (y, x): its forward differences along x and y (0 at the last column / row)
BDS_HD void il_smooth(const ImageLossArgs &a, int p, int y, int x, float *sx, float *sy) {
  const float id = il_inv_depth(a.depth, p);
  *sx = x + 1 < a.W ? fabsf((id - il_inv_depth(a.depth, p + 1)) * il_edge_weight(a.pixels, p, p + 1)) : 0.f;
  *sy = y + 1 < a.H ? fabsf((id - il_inv_depth(a.depth, p + a.W)) * il_edge_weight(a.pixels, p, p + a.W)) : 0.f;
}
// derivative to depth[p] of gx * (sum of the x differences) + gy * (sum of the y differences): the four differences p takes part in
BDS_HD float il_smooth_grad(const ImageLossArgs &a, int p, int y, int x, float gx, float gy) {
  const float id = il_inv_depth(a.depth, p);
  float vid = 0.f;
  if (x + 1 < a.W) { const float w = il_edge_weight(a.pixels, p, p + 1); vid += gx * il_sign((id - il_inv_depth(a.depth, p + 1)) * w) * w; }
  if (x > 0) { const float w = il_edge_weight(a.pixels, p - 1, p); vid -= gx * il_sign((il_inv_depth(a.depth, p - 1) - id) * w) * w; }
  if (y + 1 < a.H) { const float w = il_edge_weight(a.pixels, p, p + a.W); vid += gy * il_sign((id - il_inv_depth(a.depth, p + a.W)) * w) * w; }
  if (y > 0) { const float w = il_edge_weight(a.pixels, p - a.W, p); vid -= gy * il_sign((il_inv_depth(a.depth, p - a.W) - id) * w) * w; }
  return -vid * id * id;
}

// ---- one pixel, forward: adds to the float sums s[kIlFloatSums] and the two counts ----------------------------------------------------
BDS_HD void image_loss_pixel_fwd(const ImageLossArgs &a, int p, float *s, int *n_depth, int *n_dyn) {
  const float valid = a.egocar ? 1.f - a.egocar[p] : 1.f;
  const float *rgb = a.rgb + (int64_t)p * 3, *pix = a.pixels + (int64_t)p * 3;
  const float l1 = fabsf(pix[0] * valid - rgb[0] * valid) + fabsf(pix[1] * valid - rgb[1] * valid) + fabsf(pix[2] * valid - rgb[2] * valid);
  s[0] += l1;
  if (a.mask_kind != kIlMaskOff) s[1] += il_mask(a, a.opacity[p] * valid, (1.f - a.sky[p]) * valid);
  if (a.lidar) {
    float v, g;
    if (il_depth(a, a.depth[p], a.lidar[p], valid, &v, &g)) {
      s[2] += v;
      *n_depth += 1;
    }
  }
  if (a.entropy) s[3] += il_entropy(a.opacity[p]);
  if (a.smoothness) {
    const int y = p / a.W;
    float sx, sy;
    il_smooth(a, p, y, p - y * a.W, &sx, &sy);
    s[4] += sx;
    s[5] += sy;
  }
  if (a.dyn_opacity && a.dyn_opacity[p] > a.dyn_threshold && valid != 0.f) {   // dynamic_pred_mask & valid_loss_mask.bool()
    s[6] += l1;
    *n_dyn += 1;
  }
}

// the six weighted terms from the finished row of sums
BDS_HD void image_loss_terms(const ImageLossArgs &a, const float *sums, float *terms) {
  const float P = (float)a.H * (float)a.W;
  terms[0] = a.w[0] * (sums[0] / (3.f * P));
  terms[1] = a.mask_kind != kIlMaskOff ? a.w[1] * (sums[1] / P) : 0.f;
  float d = 0.f;
  if (a.lidar) {   // mean_on_hit over an empty set: 0 / 0 = NaN, as torch's mean of an empty tensor
    const float den = a.reduction == kIlMeanOnHit ? sums[kIlDepthCount] : (a.reduction == kIlMeanOnHw ? P : 1.f);
    d = a.w[2] * (sums[2] / den);
  }
  terms[2] = d;
  terms[3] = a.entropy ? a.w[3] * (sums[3] / P) : 0.f;
  // (a mean over an empty tensor, W = 1 or H = 1, is NaN in the reference, too)
  terms[4] = a.smoothness ? a.w[4] * (sums[4] / ((float)a.H * (float)(a.W - 1)) + sums[5] / ((float)(a.H - 1) * (float)a.W)) : 0.f;
  terms[5] = (a.dyn_opacity && sums[kIlDynCount] > 0.f) ? a.w[5] * (sums[6] / (3.f * sums[kIlDynCount])) : 0.f;
}

// per-term factors of the backward: upstream gradient x weight / denominator
struct ImageLossScales { float rgb, mask, depth, entropy, sx, sy, dyn; };
BDS_HD ImageLossScales image_loss_scales(const ImageLossArgs &a, const float *sums, const float *v_terms) {
  const float P = (float)a.H * (float)a.W;
  ImageLossScales g;
  g.rgb = v_terms[0] * a.w[0] / (3.f * P);
  g.mask = v_terms[1] * a.w[1] / P;
  g.depth = v_terms[2] * a.w[2] / (a.reduction == kIlMeanOnHit ? sums[kIlDepthCount] : (a.reduction == kIlMeanOnHw ? P : 1.f));
  g.entropy = v_terms[3] * a.w[3] / P;
  g.sx = v_terms[4] * a.w[4] / ((float)a.H * (float)(a.W - 1));
  g.sy = v_terms[4] * a.w[4] / ((float)(a.H - 1) * (float)a.W);
  g.dyn = sums[kIlDynCount] > 0.f ? v_terms[5] * a.w[5] / (3.f * sums[kIlDynCount]) : 0.f;
  return g;
}

// ---- one pixel, backward: each output (where its pointer is given) is written once, the sum of the terms that reach it ---------------
BDS_HD void image_loss_pixel_bwd(const ImageLossArgs &a, const ImageLossScales &g, int p, float *v_rgb, float *v_opacity, float *v_depth) {
  const float valid = a.egocar ? 1.f - a.egocar[p] : 1.f;
  if (v_rgb) {
    const float *rgb = a.rgb + (int64_t)p * 3, *pix = a.pixels + (int64_t)p * 3;
    float k = g.rgb;
    if (a.dyn_opacity && a.dyn_opacity[p] > a.dyn_threshold && valid != 0.f) k += g.dyn;
    float *o = v_rgb + (int64_t)p * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = il_sign(rgb[c] * valid - pix[c] * valid) * k * valid;
  }
  if (v_opacity) {
    float v = 0.f;
    if (a.mask_kind != kIlMaskOff) v = g.mask * il_mask_grad(a, a.opacity[p] * valid, (1.f - a.sky[p]) * valid) * valid;
    if (a.entropy) v += g.entropy * il_entropy_grad(a.opacity[p]);
    v_opacity[p] = v;
  }
  if (v_depth) {
    float v = 0.f, val, gd;
    if (a.lidar && il_depth(a, a.depth[p], a.lidar[p], valid, &val, &gd)) v = g.depth * gd;
    if (a.smoothness) {
      const int y = p / a.W;
      v += il_smooth_grad(a, p, y, p - y * a.W, g.sx, g.sy);
    }
    v_depth[p] = v;
  }
}

}  // namespace bds
