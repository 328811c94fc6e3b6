// Photometric L1 of the training step: mean |a - b| over an image, forward and backward.
// models/trainers/base.py:518-529 (rgb loss, losses.rgb.w = 0.8 L1 part) -- the step right after the hot path
// (SURVEY.md 8f rank 1).  One streaming pass each way instead of the ~8 framework kernels of
// (a - b).abs().mean() and its autograd graph; HBM-bound (8 B/element forward, 12 B/element backward).
#include "bds_common.h"
#include "image_loss_math.h"

namespace bds {

constexpr int kLossBlock = 256;

__global__ __launch_bounds__(kLossBlock) void l1_mean_fwd_kernel(int64_t n4, int64_t n, const float4 *__restrict__ a4,
                                                                const float4 *__restrict__ b4, const float *__restrict__ a,
                                                                const float *__restrict__ b, float scale,
                                                                float *__restrict__ out) {
  __shared__ float red[kLossBlock / kWave];
  float s = 0.f;
  const int64_t stride = (int64_t)gridDim.x * kLossBlock;
  int64_t i = (int64_t)blockIdx.x * kLossBlock + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {   // 8 independent 16-byte loads in flight per lane
    float4 x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { x[u] = a4[i + u * stride]; y[u] = b4[i + u * stride]; }
#pragma unroll
    for (int u = 0; u < 4; u++)
      s += fabsf(x[u].x - y[u].x) + fabsf(x[u].y - y[u].y) + fabsf(x[u].z - y[u].z) + fabsf(x[u].w - y[u].w);
  }
  for (; i < n4; i += stride) {
    const float4 x = a4[i], y = b4[i];
    s += fabsf(x.x - y.x) + fabsf(x.y - y.y) + fabsf(x.z - y.z) + fabsf(x.w - y.w);
  }
  if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {  // tail (n not a multiple of 4)
    const int64_t i = n4 * 4 + threadIdx.x;
    s += fabsf(a[i] - b[i]);
  }
  s = wave_sum_to_lane63(s);
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) red[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < kLossBlock / kWave; w++) t += red[w];
    atomicAdd(out, t * scale);
  }
}

__global__ __launch_bounds__(kLossBlock) void l1_mean_bwd_kernel(int64_t n, const float *__restrict__ a,
                                                                const float *__restrict__ b, float scale,
                                                                const float *__restrict__ v_out, float *__restrict__ v_a) {
  const float g = *v_out * scale;
  for (int64_t i = (int64_t)blockIdx.x * kLossBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLossBlock) {
    const float d = a[i] - b[i];
    v_a[i] = d > 0.f ? g : (d < 0.f ? -g : 0.f);   // torch: sign(0) = 0
  }
}

// ---- SSIM (11x11 Gaussian window, sigma 1.5, VALID region, K = (0.01, 0.03), data range 1) -----------------------
// pytorch_msssim 1.0.0 `SSIM(data_range=1.0, size_average=True, channel=3)` as used at models/trainers/base.py:114,541
// (external package, parity unpinned: oracle/loss_oracle.py).  Images are [H,W,CH] as the path produces them (the
// reference permutes to [1,CH,H,W] first).  One workgroup = one 16x16 tile of OUTPUT pixels of one channel: the
// 26x26 input patch is staged in LDS, the five windowed moments are taken separably (row pass into LDS, column pass in
// registers), and next to the SSIM value the three partial derivatives with respect to the moments of `pred` that the
// backward needs are written out, so that the backward is ONE more separable pass (the adjoint of the valid filter).
constexpr int kSsimWin = 11, kSsimTile = 16, kSsimIn = kSsimTile + kSsimWin - 1;  // 26
struct SsimWindow { float w[kSsimWin]; };

__global__ __launch_bounds__(kSsimTile * kSsimTile) void ssim_fwd_kernel(int H, int W, int CH, const float *__restrict__ x,
                                                                        const float *__restrict__ y, SsimWindow win, float C1,
                                                                        float C2, float scale, float *__restrict__ out,
                                                                        float *__restrict__ dmaps) {
  __shared__ float sx[kSsimIn][kSsimIn + 1], sy[kSsimIn][kSsimIn + 1];
  __shared__ float hb[5][kSsimIn][kSsimTile + 1];
  __shared__ float red[kSsimTile * kSsimTile / kWave];
  const int Ho = H - (kSsimWin - 1), Wo = W - (kSsimWin - 1);
  const int c = blockIdx.z, oi0 = blockIdx.y * kSsimTile, oj0 = blockIdx.x * kSsimTile, tid = threadIdx.x;
  for (int e = tid; e < kSsimIn * kSsimIn; e += kSsimTile * kSsimTile) {
    const int r = e / kSsimIn, q = e - r * kSsimIn, i = oi0 + r, j = oj0 + q;
    const bool in = i < H && j < W;
    const int64_t o = ((int64_t)i * W + j) * CH + c;
    sx[r][q] = in ? x[o] : 0.f;
    sy[r][q] = in ? y[o] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < kSsimIn * kSsimTile; e += kSsimTile * kSsimTile) {   // row pass
    const int r = e / kSsimTile, j = e - r * kSsimTile;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
    for (int b = 0; b < kSsimWin; b++) {
      const float xv = sx[r][j + b], yv = sy[r][j + b], w = win.w[b];
      a0 += w * xv; a1 += w * yv; a2 += w * xv * xv; a3 += w * yv * yv; a4 += w * xv * yv;
    }
    hb[0][r][j] = a0; hb[1][r][j] = a1; hb[2][r][j] = a2; hb[3][r][j] = a3; hb[4][r][j] = a4;
  }
  __syncthreads();
  const int ti = tid / kSsimTile, tj = tid - ti * kSsimTile;
  float m1 = 0.f, m2 = 0.f, e1 = 0.f, e2 = 0.f, e12 = 0.f;
#pragma unroll
  for (int a = 0; a < kSsimWin; a++) {   // column pass
    const float w = win.w[a];
    m1 += w * hb[0][ti + a][tj]; m2 += w * hb[1][ti + a][tj];
    e1 += w * hb[2][ti + a][tj]; e2 += w * hb[3][ti + a][tj]; e12 += w * hb[4][ti + a][tj];
  }
  const int oi = oi0 + ti, oj = oj0 + tj;
  const bool valid = oi < Ho && oj < Wo;
  const float s1 = e1 - m1 * m1, s2 = e2 - m2 * m2, s12 = e12 - m1 * m2;
  const float A = 2.f * m1 * m2 + C1, B = m1 * m1 + m2 * m2 + C1, Cn = 2.f * s12 + C2, D = s1 + s2 + C2;
  const float lum = A / B, cs = Cn / D;
  float S = valid ? lum * cs : 0.f;
  if (valid && dmaps != nullptr) {
    // S as a function of (m2, e2, e12) with s2 = e2 - m2^2, s12 = e12 - m1 m2
    const float d_lum = (2.f * m1 * B - A * 2.f * m2) / (B * B);
    const float d_cs = (-2.f * m1 * D + 2.f * m2 * Cn) / (D * D);
    const int64_t plane = (int64_t)Ho * Wo, o = ((int64_t)c * Ho + oi) * Wo + oj;
    dmaps[o] = d_lum * cs + lum * d_cs;                       // dS / d mu_pred
    dmaps[(int64_t)CH * plane + o] = -lum * Cn / (D * D);     // dS / d E[pred^2]
    dmaps[2 * (int64_t)CH * plane + o] = lum * 2.f / D;       // dS / d E[gt * pred]
  }
  S = wave_sum_to_lane63(S);
  if ((tid & (kWave - 1)) == kWave - 1) red[tid / kWave] = S;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < kSsimTile * kSsimTile / kWave; w++) t += red[w];
    atomicAdd(out, t * scale);
  }
}

__global__ __launch_bounds__(kSsimTile * kSsimTile) void ssim_bwd_kernel(int H, int W, int CH, const float *__restrict__ x,
                                                                        const float *__restrict__ y, SsimWindow win, float scale,
                                                                        const float *__restrict__ v_out,
                                                                        const float *__restrict__ dmaps, float *__restrict__ v_y) {
  __shared__ float sd[3][kSsimIn][kSsimIn + 1];
  __shared__ float hb[3][kSsimIn][kSsimTile + 1];
  const int Ho = H - (kSsimWin - 1), Wo = W - (kSsimWin - 1);
  const int c = blockIdx.z, i0 = blockIdx.y * kSsimTile, j0 = blockIdx.x * kSsimTile, tid = threadIdx.x;
  const int64_t plane = (int64_t)Ho * Wo;
  // output pixels whose window covers input pixel (i,j): (i-a, j-b), a, b = 0..10
  for (int e = tid; e < kSsimIn * kSsimIn; e += kSsimTile * kSsimTile) {
    const int r = e / kSsimIn, q = e - r * kSsimIn, oi = i0 - (kSsimWin - 1) + r, oj = j0 - (kSsimWin - 1) + q;
    const bool in = oi >= 0 && oi < Ho && oj >= 0 && oj < Wo;
    const int64_t o = ((int64_t)c * Ho + (in ? oi : 0)) * Wo + (in ? oj : 0);
#pragma unroll
    for (int k = 0; k < 3; k++) sd[k][r][q] = in ? dmaps[(int64_t)k * CH * plane + o] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < kSsimIn * kSsimTile; e += kSsimTile * kSsimTile) {
    const int r = e / kSsimTile, j = e - r * kSsimTile;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int b = 0; b < kSsimWin; b++) {
      const float w = win.w[b];
      const int q = j + (kSsimWin - 1) - b;
      a0 += w * sd[0][r][q]; a1 += w * sd[1][r][q]; a2 += w * sd[2][r][q];
    }
    hb[0][r][j] = a0; hb[1][r][j] = a1; hb[2][r][j] = a2;
  }
  __syncthreads();
  const int ti = tid / kSsimTile, tj = tid - ti * kSsimTile, i = i0 + ti, j = j0 + tj;
  if (i >= H || j >= W) return;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;
#pragma unroll
  for (int a = 0; a < kSsimWin; a++) {
    const float w = win.w[a];
    const int r = ti + (kSsimWin - 1) - a;
    c0 += w * hb[0][r][tj]; c1 += w * hb[1][r][tj]; c2 += w * hb[2][r][tj];
  }
  const int64_t o = ((int64_t)i * W + j) * CH + c;
  v_y[o] = v_out[0] * scale * (c0 + 2.f * y[o] * c1 + x[o] * c2);
}

// ---- the whole image loss in one pass each way (csrc/image_loss_math.h: the six terms, per pixel) -----------------------------------
// BasicTrainer.compute_losses, models/trainers/base.py:518-585 and :638-652, at every option of models/losses.py:33-178.  HBM-bound: the
// forward reads 48 B a pixel (rgb, pixels, opacity, sky, depth, lidar, egocar, dyn_opacity; the smoothness term's neighbours come from
// the cache), the backward those and writes 20 B (v_rgb, v_opacity, v_depth, each ONCE: the sum of the terms that reach it).  Whether a
// term is on is a kernel argument: uniform branches.  No floating-point atomics: each forward workgroup writes its row of kIlSums sums
// (the two counts as integers), a one-workgroup finish adds the rows in a fixed order, keeps the finished row for the backward and forms
// the six weighted terms: bit-identical run to run.
constexpr int kIlBlock = 256, kIlMaxBlocks = 2048;   // the forward strides a grid of at most 2048 x 256 threads: the finish reads <= 2048 rows

__global__ __launch_bounds__(kIlBlock) void image_loss_fwd_kernel(ImageLossArgs a, float *__restrict__ partials) {
  __shared__ float red[kIlBlock / kWave][kIlSums];
  float s[kIlFloatSums] = {};
  int n[2] = {0, 0};
  const int64_t P = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * kIlBlock + threadIdx.x; i < P; i += (int64_t)gridDim.x * kIlBlock)
    image_loss_pixel_fwd(a, (int)i, s, &n[0], &n[1]);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kIlFloatSums; k++) {
    const float t = wave_sum_all(s[k]);
    if (lane == 0) red[wave][k] = t;
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    int t = n[k];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) red[wave][kIlFloatSums + k] = __int_as_float(t);
  }
  __syncthreads();
  if (threadIdx.x < kIlSums) {
    const int k = threadIdx.x;
    float out;
    if (k < kIlFloatSums) {
      out = red[0][k];
#pragma unroll
      for (int w = 1; w < kIlBlock / kWave; w++) out += red[w][k];
    } else {
      int t = 0;
#pragma unroll
      for (int w = 0; w < kIlBlock / kWave; w++) t += __float_as_int(red[w][k]);
      out = __int_as_float(t);
    }
    partials[(int64_t)blockIdx.x * kIlSums + k] = out;
  }
}

// one workgroup of kIlSums waves: wave k adds column k of the rows (lanes stride the rows with four sums each, then the butterfly)
__global__ __launch_bounds__(kIlSums *kWave) void image_loss_finish_kernel(ImageLossArgs a, const float *__restrict__ partials, int blocks,
                                                                          float *__restrict__ sums, float *__restrict__ terms) {
  __shared__ float tot[kIlSums];
  const int lane = threadIdx.x & (kWave - 1), k = threadIdx.x / kWave;
  float total;
  if (k < kIlFloatSums) {
    float s[4] = {};
    for (int b = lane; b < blocks; b += 4 * kWave) {
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (b + u * kWave < blocks) s[u] += partials[(int64_t)(b + u * kWave) * kIlSums + k];
    }
    total = wave_sum_all((s[0] + s[1]) + (s[2] + s[3]));
  } else {
    int64_t t = 0;
    for (int b = lane; b < blocks; b += kWave) t += __float_as_int(partials[(int64_t)b * kIlSums + k]);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) t += __shfl_xor(t, o);
    total = (float)t;
  }
  if (lane == 0) {
    tot[k] = total;
    sums[k] = total;
  }
  __syncthreads();
  if (threadIdx.x < kIlTerms) {
    float t[kIlTerms];
    image_loss_terms(a, tot, t);
    terms[threadIdx.x] = t[threadIdx.x];
  }
}

__global__ __launch_bounds__(kIlBlock) void image_loss_bwd_kernel(ImageLossArgs a, const float *__restrict__ sums,
                                                                 const float *__restrict__ v_terms, float *__restrict__ v_rgb,
                                                                 float *__restrict__ v_opacity, float *__restrict__ v_depth) {
  const int64_t i = (int64_t)blockIdx.x * kIlBlock + threadIdx.x;
  if (i >= (int64_t)a.H * a.W) return;
  image_loss_pixel_bwd(a, image_loss_scales(a, sums, v_terms), (int)i, v_rgb, v_opacity, v_depth);
}

}  // namespace bds

using namespace bds;

extern "C" int bds_l1_mean_fwd(int64_t n, const float *a, const float *b, float *out, bds_stream_t stream) {
  BDS_REQUIRE(n >= 0 && out);
  if (n == 0) return BDS_OK;
  BDS_REQUIRE(a && b);
  const bool vec = aligned16(a) && aligned16(b);
  const int64_t n4 = vec ? n / 4 : 0;
  int64_t blocks = cdiv(n4 > 0 ? n4 : 1, kLossBlock * 4);
  if (blocks > 512) blocks = 512;   // one atomic per workgroup on ONE address: keep them few
  BDS_REQUIRE(vec);  // 16-byte aligned buffers (torch allocations are)
  hipLaunchKernelGGL(l1_mean_fwd_kernel, dim3((unsigned)blocks), dim3(kLossBlock), 0, as_stream(stream), n4, n,
                     reinterpret_cast<const float4 *>(a), reinterpret_cast<const float4 *>(b), a, b, 1.0f / (float)n, out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_l1_mean_bwd(int64_t n, const float *a, const float *b, const float *v_out, float *v_a,
                               bds_stream_t stream) {
  BDS_REQUIRE(n >= 0);
  if (n == 0) return BDS_OK;
  BDS_REQUIRE(a && b && v_out && v_a);
  int64_t blocks = cdiv(n, kLossBlock * 4);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(l1_mean_bwd_kernel, dim3((unsigned)blocks), dim3(kLossBlock), 0, as_stream(stream), n, a, b,
                     1.0f / (float)n, v_out, v_a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

static SsimWindow ssim_window() {   // _fspecial_gauss_1d(11, 1.5) in float arithmetic
  SsimWindow w;
  float sum = 0.f;
  for (int i = 0; i < kSsimWin; i++) {
    const float cidx = (float)(i - kSsimWin / 2);
    w.w[i] = expf(-(cidx * cidx) / (2.f * 1.5f * 1.5f));
    sum += w.w[i];
  }
  for (int i = 0; i < kSsimWin; i++) w.w[i] /= sum;
  return w;
}

extern "C" size_t bds_ssim_workspace_bytes(int H, int W, int CH) {
  if (H < kSsimWin || W < kSsimWin || CH < 1) return 0;
  return sizeof(float) * 3 * (size_t)CH * (size_t)(H - kSsimWin + 1) * (size_t)(W - kSsimWin + 1);
}

extern "C" int bds_ssim_fwd(int H, int W, int CH, const float *target, const float *pred, float *ssim_out, void *ws,
                            size_t ws_bytes, bds_stream_t stream) {
  BDS_REQUIRE(H >= kSsimWin && W >= kSsimWin && CH >= 1 && CH <= 65535 && target && pred && ssim_out);
  if (ws != nullptr && ws_bytes < bds_ssim_workspace_bytes(H, W, CH)) return BDS_EWORKSPACE;
  const int Ho = H - kSsimWin + 1, Wo = W - kSsimWin + 1;
  const dim3 grid((unsigned)cdiv(Wo, kSsimTile), (unsigned)cdiv(Ho, kSsimTile), (unsigned)CH);
  const float scale = 1.0f / ((float)Ho * (float)Wo * (float)CH);
  hipLaunchKernelGGL(ssim_fwd_kernel, grid, dim3(kSsimTile * kSsimTile), 0, as_stream(stream), H, W, CH, target, pred,
                     ssim_window(), 0.01f * 0.01f, 0.03f * 0.03f, scale, ssim_out, static_cast<float *>(ws));
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_ssim_bwd(int H, int W, int CH, const float *target, const float *pred, const void *ws, size_t ws_bytes,
                            const float *v_ssim, float *v_pred, bds_stream_t stream) {
  BDS_REQUIRE(H >= kSsimWin && W >= kSsimWin && CH >= 1 && CH <= 65535 && target && pred && ws && v_ssim && v_pred);
  if (ws_bytes < bds_ssim_workspace_bytes(H, W, CH)) return BDS_EWORKSPACE;
  const int Ho = H - kSsimWin + 1, Wo = W - kSsimWin + 1;
  const dim3 grid((unsigned)cdiv(W, kSsimTile), (unsigned)cdiv(H, kSsimTile), (unsigned)CH);
  const float scale = 1.0f / ((float)Ho * (float)Wo * (float)CH);
  hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(kSsimTile * kSsimTile), 0, as_stream(stream), H, W, CH, target, pred,
                     ssim_window(), scale, v_ssim, static_cast<const float *>(ws), v_pred);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

static int64_t image_loss_blocks(int H, int W) {
  const int64_t b = cdiv((int64_t)H * W, kIlBlock);
  return b < kIlMaxBlocks ? b : kIlMaxBlocks;
}

static int image_loss_args(ImageLossArgs &a, int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                           const float *sky_masks, const float *lidar, const float *egocar, const float *dyn_opacity, int mask_kind,
                           double safe_limit, int depth_type, int depth_normalize, int depth_inverse, float max_depth, int depth_reduction,
                           int entropy, int smoothness, float dyn_threshold, const float *weights) {
  BDS_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX && rgb && pixels && weights);
  BDS_REQUIRE(mask_kind >= kIlMaskOff && mask_kind <= kIlMaskSafeBce && (sky_masks != nullptr) == (mask_kind != kIlMaskOff));
  BDS_REQUIRE(mask_kind == kIlMaskOff || opacity);
  BDS_REQUIRE(mask_kind != kIlMaskSafeBce || (safe_limit > 0.0 && safe_limit < 1.0));
  BDS_REQUIRE(depth_type >= kIlDepthL1 && depth_type <= kIlDepthSmoothL1 && depth_reduction >= kIlMeanOnHit && depth_reduction <= kIlSum);
  BDS_REQUIRE(lidar == nullptr || (depth && max_depth > 0.f));
  BDS_REQUIRE((!entropy || opacity) && (!smoothness || depth));
  a.rgb = rgb; a.pixels = pixels; a.opacity = opacity; a.depth = depth; a.sky = sky_masks; a.lidar = lidar; a.egocar = egocar;
  a.dyn_opacity = dyn_opacity;
  a.H = H; a.W = W; a.mask_kind = mask_kind;
  const double ln_limit = mask_kind == kIlMaskSafeBce ? log(safe_limit) : 0.0, limit = exp(ln_limit);   // SafeBCE: np.log, then np.exp of it
  a.ln_limit = (float)ln_limit; a.limit = (float)limit; a.one_minus_limit = (float)(1.0 - limit);
  a.depth_type = depth_type; a.normalize = depth_normalize ? 1 : 0; a.inverse = depth_inverse ? 1 : 0; a.reduction = depth_reduction;
  a.max_depth = max_depth; a.entropy = entropy ? 1 : 0; a.smoothness = smoothness ? 1 : 0; a.dyn_threshold = dyn_threshold;
  for (int k = 0; k < kIlTerms; k++) a.w[k] = weights[k];
  return BDS_OK;
}

extern "C" size_t bds_image_loss_temp_bytes(int H, int W) {
  if (H < 1 || W < 1) return 0;
  return sizeof(float) * kIlSums * (size_t)image_loss_blocks(H, W);
}

extern "C" int bds_image_loss_fwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                                  const float *sky_masks, const float *lidar, const float *egocar, const float *dyn_opacity, int mask_kind,
                                  double safe_limit, int depth_type, int depth_normalize, int depth_inverse, float max_depth,
                                  int depth_reduction, int entropy, int smoothness, float dyn_threshold, const float *weights, float *terms,
                                  float *sums, void *temp, size_t temp_bytes, bds_stream_t stream) {
  ImageLossArgs a;
  int rc = image_loss_args(a, H, W, rgb, pixels, opacity, depth, sky_masks, lidar, egocar, dyn_opacity, mask_kind, safe_limit, depth_type,
                           depth_normalize, depth_inverse, max_depth, depth_reduction, entropy, smoothness, dyn_threshold, weights);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(terms && sums && temp && temp_bytes >= bds_image_loss_temp_bytes(H, W));
  const int blocks = (int)image_loss_blocks(H, W);
  hipLaunchKernelGGL(image_loss_fwd_kernel, dim3((unsigned)blocks), dim3(kIlBlock), 0, as_stream(stream), a, static_cast<float *>(temp));
  hipLaunchKernelGGL(image_loss_finish_kernel, dim3(1), dim3(kIlSums * kWave), 0, as_stream(stream), a, static_cast<const float *>(temp),
                     blocks, sums, terms);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_image_loss_bwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                                  const float *sky_masks, const float *lidar, const float *egocar, const float *dyn_opacity, int mask_kind,
                                  double safe_limit, int depth_type, int depth_normalize, int depth_inverse, float max_depth,
                                  int depth_reduction, int entropy, int smoothness, float dyn_threshold, const float *weights,
                                  const float *sums, const float *v_terms, float *v_rgb, float *v_opacity, float *v_depth,
                                  bds_stream_t stream) {
  ImageLossArgs a;
  int rc = image_loss_args(a, H, W, rgb, pixels, opacity, depth, sky_masks, lidar, egocar, dyn_opacity, mask_kind, safe_limit, depth_type,
                           depth_normalize, depth_inverse, max_depth, depth_reduction, entropy, smoothness, dyn_threshold, weights);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(sums && v_terms);
  if (!v_rgb && !v_opacity && !v_depth) return BDS_OK;
  hipLaunchKernelGGL(image_loss_bwd_kernel, dim3((unsigned)cdiv((int64_t)H * W, kIlBlock)), dim3(kIlBlock), 0, as_stream(stream), a, sums,
                     v_terms, v_rgb, v_opacity, v_depth);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
