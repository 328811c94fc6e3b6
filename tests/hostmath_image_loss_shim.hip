// TEST-ONLY host shim of the fused image loss (csrc/image_loss_math.h, the per-pixel functions the image-loss kernels of csrc/loss.hip
// run) on the CPU, so that tests/test_image_loss_cpu.py can compare them with float64 without a GPU.  Not part of libbds.so, never
// loaded by the product.  The loops follow the kernels: one pixel at a time; the sums the kernels form per workgroup and then over the
// workgroups' rows are formed in a like shape here (256 pixels a row, in pixel order; the rows dealt to 64 partial sums, halved
// pairwise), the two counts as integers.
#include <math.h>

#include "../bilateral_driving_amd/csrc/image_loss_math.h"

using namespace bds;

namespace {

struct Sum {
  float row = 0.0f, lanes[64] = {};
  int n = 0, rows = 0;
  void flush() {
    lanes[rows++ % 64] += row;
    row = 0.0f;
    n = 0;
  }
  void next() {
    if (++n == 256) flush();
  }
  float total() {
    if (n) flush();
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; l++) lanes[l] += lanes[l + o];
    return lanes[0];
  }
};

ImageLossArgs args(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth, const float *sky,
                   const float *lidar, const float *egocar, const float *dyn, int mask_kind, double safe_limit, int depth_type, int normalize,
                   int inverse, float max_depth, int reduction, int entropy, int smoothness, float dyn_threshold, const float *weights) {
  ImageLossArgs a;
  a.rgb = rgb; a.pixels = pixels; a.opacity = opacity; a.depth = depth; a.sky = sky; a.lidar = lidar; a.egocar = egocar; a.dyn_opacity = dyn;
  a.H = H; a.W = W; a.mask_kind = mask_kind;
  const double ln_limit = mask_kind == kIlMaskSafeBce ? log(safe_limit) : 0.0, limit = exp(ln_limit);
  a.ln_limit = (float)ln_limit; a.limit = (float)limit; a.one_minus_limit = (float)(1.0 - limit);
  a.depth_type = depth_type; a.normalize = normalize; a.inverse = inverse; a.reduction = reduction; a.max_depth = max_depth;
  a.entropy = entropy; a.smoothness = smoothness; a.dyn_threshold = dyn_threshold;
  for (int k = 0; k < kIlTerms; k++) a.w[k] = weights[k];
  return a;
}

}  // namespace

extern "C" void hm_image_loss_fwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                                  const float *sky, const float *lidar, const float *egocar, const float *dyn, int mask_kind,
                                  double safe_limit, int depth_type, int normalize, int inverse, float max_depth, int reduction, int entropy,
                                  int smoothness, float dyn_threshold, const float *weights, float *terms, float *sums) {
  const ImageLossArgs a = args(H, W, rgb, pixels, opacity, depth, sky, lidar, egocar, dyn, mask_kind, safe_limit, depth_type, normalize,
                               inverse, max_depth, reduction, entropy, smoothness, dyn_threshold, weights);
  Sum acc[kIlFloatSums];
  int n_depth = 0, n_dyn = 0;
  for (int p = 0; p < H * W; p++) {
    float s[kIlFloatSums] = {};
    image_loss_pixel_fwd(a, p, s, &n_depth, &n_dyn);
    for (int k = 0; k < kIlFloatSums; k++) {
      acc[k].row += s[k];
      acc[k].next();
    }
  }
  for (int k = 0; k < kIlFloatSums; k++) sums[k] = acc[k].total();
  sums[kIlDepthCount] = (float)n_depth;
  sums[kIlDynCount] = (float)n_dyn;
  image_loss_terms(a, sums, terms);
}

extern "C" void hm_image_loss_bwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                                  const float *sky, const float *lidar, const float *egocar, const float *dyn, int mask_kind,
                                  double safe_limit, int depth_type, int normalize, int inverse, float max_depth, int reduction, int entropy,
                                  int smoothness, float dyn_threshold, const float *weights, const float *sums, const float *v_terms,
                                  float *v_rgb, float *v_opacity, float *v_depth) {
  const ImageLossArgs a = args(H, W, rgb, pixels, opacity, depth, sky, lidar, egocar, dyn, mask_kind, safe_limit, depth_type, normalize,
                               inverse, max_depth, reduction, entropy, smoothness, dyn_threshold, weights);
  const ImageLossScales g = image_loss_scales(a, sums, v_terms);
  for (int p = 0; p < H * W; p++) image_loss_pixel_bwd(a, g, p, v_rgb, v_opacity, v_depth);
}
