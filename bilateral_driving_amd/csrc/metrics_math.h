// Per-pixel math of the evaluation image metrics (models/video_utils.py:29-44, 273-361: compute_psnr and
// skimage.metrics.structural_similarity(data_range=1.0, channel_axis=-1) at its defaults), used by csrc/metrics.hip and by the host
// shim tests/hostmath_metrics_shim.hip.  skimage's SSIM of one channel, as it forms it:
//   the five 7x7 uniform-window means ux, uy, uxx, uyy, uxy (scipy.ndimage.uniform_filter, mode="reflect": d c b a | a b c d | d c b a)
//   NP = 49, cov_norm = NP / (NP - 1):  vx = cov_norm (uxx - ux ux), vy, vxy likewise;  C1 = 0.01^2, C2 = 0.03^2 (data range 1)
//   S = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2))
// uxx - ux ux cancels in float32 where the image is flat against its level (up to 1e-4 per map element on an image flat to 1e-3), so
// the window sums and the expression are taken in double -- a product of two float32 samples is exact there -- and S is rounded to
// float32 once, the precision skimage returns for float32 images.
#pragma once
#include "gs_math.h"

namespace bds {

constexpr int kSsimWin = 7, kSsimPad = kSsimWin / 2;        // skimage's default win_size; its crop of the mean is (win_size - 1) / 2
constexpr int kSsimMoments = 5;                             // x, y, xx, yy, xy
constexpr double kSsimC1 = 0.01 * 0.01, kSsimC2 = 0.03 * 0.03;

// index i of an axis of n >= kSsimWin samples under mode="reflect" (the edge sample repeated); exact for -n <= i < 2 n.  The clamp
// only keeps indices no output depends on (the halo of a partial tile beyond the image's own halo) inside the array.
BDS_HD int metrics_reflect(int i, int n) {
  const int r = i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
  return r < 0 ? 0 : (r >= n ? n - 1 : r);
}

// adds one sample pair to the five sums
BDS_HD void metrics_tap(float xf, float yf, double *m) {
  const double x = (double)xf, y = (double)yf;
  m[0] += x;
  m[1] += y;
  m[2] += x * x;
  m[3] += y * y;
  m[4] += x * y;
}

// S of one pixel from the five 7x7 window SUMS m
BDS_HD float metrics_ssim(const double *m) {
  constexpr double inv = 1.0 / (kSsimWin * kSsimWin), cov_norm = (double)(kSsimWin * kSsimWin) / (kSsimWin * kSsimWin - 1);
  const double ux = m[0] * inv, uy = m[1] * inv;
  const double vx = cov_norm * (m[2] * inv - ux * ux), vy = cov_norm * (m[3] * inv - uy * uy), vxy = cov_norm * (m[4] * inv - ux * uy);
  const double a1 = 2.0 * ux * uy + kSsimC1, a2 = 2.0 * vxy + kSsimC2;
  const double b1 = ux * ux + uy * uy + kSsimC1, b2 = vx + vy + kSsimC2;
  return (float)((a1 * a2) / (b1 * b2));
}

// the finished values from the sums (double throughout): -10 log10(mse) is +inf for identical images, as the reference's expression
BDS_HD double metrics_psnr(double sq_err, double n_values) { return -10.0 * log10(sq_err / n_values); }

}  // namespace bds
