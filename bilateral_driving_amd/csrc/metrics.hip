// Evaluation image metrics of one frame in one pass (models/video_utils.py:29-44, 273-361): PSNR, skimage's SSIM (7x7 uniform window,
// sample covariance, reflected borders, mean over the cropped interior) and both of them under up to four pixel masks, where the
// reference calls structural_similarity up to five times on the host and indexes the same map four times.  The per-pixel math lives
// in metrics_math.h.
//   tile    one workgroup per 16x16 tile of output pixels, all three channels: the reflected 22x22 patch of both images goes to LDS
//           as it is, per channel the five 7-tap row sums go to LDS in double (metrics_math.h on why) and the column sums stay in
//           registers; S per pixel and channel, optionally stored as the [H,W,3] map (skimage's full=True).  The
//           tile's 16 partial sums -- squared error, S over the cropped interior per channel, and per mask slot {pixels, squared
//           error, S over all three channels, uncropped} -- are reduced in double in a fixed order and stored as one workspace row.
//   reduce  one workgroup adds the rows in a fixed order in double and writes the finished row of BDS_IMAGE_METRICS_ROW doubles.
// No atomics anywhere: bit-identical run to run, whatever order the workgroups retire in.
#include "bds_common.h"
#include "metrics_math.h"

namespace bds {

constexpr int kMetTile = 16, kMetPatch = kMetTile + 2 * kSsimPad, kMetPatchN = kMetPatch * kMetPatch;
constexpr int kMetBlock = kMetTile * kMetTile, kMetWaves = kMetBlock / kWave;
constexpr int kMetSlots = 4, kMetVals = 4 + 3 * kMetSlots;      // partial sums per tile
constexpr int kMetRedBlock = 1024, kMetRedGroups = kMetRedBlock / kMetVals;
static_assert(kMetVals == 16 && BDS_IMAGE_METRICS_ROW == 2 + 3 * kMetSlots, "row layouts");

struct MetMasks {
  const void *p[kMetSlots];     // [H,W], NULL = slot unused
  int invert[kMetSlots];        // the slot holds the complement of the pixels to score (the sky mask)
  int kind;                     // 0: one byte per pixel, 1: float32; non-zero = true, as astype(bool)
};

__device__ __forceinline__ bool met_mask(const void *p, int kind, int invert, int64_t pix) {
  if (p == nullptr) return false;
  const bool b = kind ? static_cast<const float *>(p)[pix] != 0.0f : static_cast<const uint8_t *>(p)[pix] != 0;
  return b != (invert != 0);
}

__global__ __launch_bounds__(kMetBlock) void metrics_tile_kernel(int H, int W, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                 MetMasks mk, float *__restrict__ map, double *__restrict__ ws) {
  __shared__ float s_x[3][kMetPatchN], s_y[3][kMetPatchN];
  __shared__ double s_r[kSsimMoments][kMetPatch][kMetTile];
  __shared__ double s_w[kMetWaves][kMetVals];
  __shared__ float s_S[3][kMetBlock];
  const int tid = threadIdx.x, tx0 = blockIdx.x * kMetTile, ty0 = blockIdx.y * kMetTile;

  for (int idx = tid; idx < kMetPatchN; idx += kMetBlock) {
    const int r = idx / kMetPatch, c = idx - r * kMetPatch;
    const int sy = metrics_reflect(ty0 + r - kSsimPad, H), sx = metrics_reflect(tx0 + c - kSsimPad, W);
    const int64_t o = ((int64_t)sy * W + sx) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      s_x[k][idx] = pred[o + k];
      s_y[k][idx] = gt[o + k];
    }
  }
  __syncthreads();

  const int oy = tid / kMetTile, ox = tid % kMetTile;
#pragma unroll 1      // (one channel's sums live at a time: the unrolled form needs twice the registers)
  for (int ch = 0; ch < 3; ch++) {
    for (int idx = tid; idx < kMetPatch * kMetTile; idx += kMetBlock) {
      const int r = idx / kMetTile, c = idx % kMetTile;
      double m[kSsimMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kSsimWin; k++) metrics_tap(s_x[ch][r * kMetPatch + c + k], s_y[ch][r * kMetPatch + c + k], m);
#pragma unroll
      for (int j = 0; j < kSsimMoments; j++) s_r[j][r][c] = m[j];
    }
    __syncthreads();
    double m[kSsimMoments] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kSsimWin; k++)
#pragma unroll
      for (int j = 0; j < kSsimMoments; j++) m[j] += s_r[j][oy + k][ox];
    s_S[ch][tid] = metrics_ssim(m);
    __syncthreads();
  }
  const float S[3] = {s_S[0][tid], s_S[1][tid], s_S[2][tid]};      // (the thread's own stores)

  double v[kMetVals];
#pragma unroll
  for (int j = 0; j < kMetVals; j++) v[j] = 0.0;
  const int y = ty0 + oy, x = tx0 + ox;
  if (y < H && x < W) {
    const int64_t pix = (int64_t)y * W + x, o = pix * 3;
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int c = (oy + kSsimPad) * kMetPatch + ox + kSsimPad;      // the pixel's own samples, staged above
      const double d = (double)s_x[k][c] - (double)s_y[k][c];
      se += d * d;
    }
    v[0] = se;
    if (y >= kSsimPad && y < H - kSsimPad && x >= kSsimPad && x < W - kSsimPad) {
#pragma unroll
      for (int k = 0; k < 3; k++) v[1 + k] = (double)S[k];
    }
    const double ssum = ((double)S[0] + (double)S[1]) + (double)S[2];
#pragma unroll
    for (int s = 0; s < kMetSlots; s++) {
      if (met_mask(mk.p[s], mk.kind, mk.invert[s], pix)) {
        v[4 + 3 * s] = 1.0;
        v[5 + 3 * s] = se;
        v[6 + 3 * s] = ssum;
      }
    }
    if (map != nullptr) {
#pragma unroll
      for (int k = 0; k < 3; k++) map[o + k] = S[k];
    }
  }
#pragma unroll
  for (int j = 0; j < kMetVals; j++) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v[j] += __shfl_xor(v[j], off);
  }
  if ((tid & (kWave - 1)) == 0) {
#pragma unroll
    for (int j = 0; j < kMetVals; j++) s_w[tid / kWave][j] = v[j];
  }
  __syncthreads();
  if (tid < kMetVals) {
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    ws[tile * kMetVals + tid] = (s_w[0][tid] + s_w[1][tid]) + (s_w[2][tid] + s_w[3][tid]);
  }
}

// out: {psnr, ssim, (psnr, ssim) of slot 0..3, valid of slot 0..3}; an empty or unused slot: NaN, NaN, 0
__global__ __launch_bounds__(kMetRedBlock) void metrics_reduce_kernel(int H, int W, int64_t tiles, const double *__restrict__ ws,
                                                                      double *__restrict__ out) {
  __shared__ double s[kMetRedGroups][kMetVals];
  const int tid = threadIdx.x, j = tid % kMetVals, g = tid / kMetVals;
  double acc = 0.0;
  for (int64_t r = g; r < tiles; r += kMetRedGroups) acc += ws[r * kMetVals + j];
  s[g][j] = acc;
  __syncthreads();
  if (tid < kMetVals) {
    double a = 0.0;
    for (int q = 0; q < kMetRedGroups; q++) a += s[q][tid];
    s[0][tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    const double n = (double)H * (double)W, nc = (double)(H - 2 * kSsimPad) * (double)(W - 2 * kSsimPad);
    out[0] = metrics_psnr(s[0][0], 3.0 * n);
    out[1] = (s[0][1] / nc + s[0][2] / nc + s[0][3] / nc) / 3.0;
    for (int q = 0; q < kMetSlots; q++) {
      const double cnt = s[0][4 + 3 * q];
      const bool ok = cnt > 0.0;
      out[2 + 2 * q] = ok ? metrics_psnr(s[0][5 + 3 * q], 3.0 * cnt) : (double)NAN;
      out[3 + 2 * q] = ok ? s[0][6 + 3 * q] / (3.0 * cnt) : (double)NAN;
      out[2 + 2 * kMetSlots + q] = ok ? 1.0 : 0.0;
    }
  }
}

static int64_t met_tiles(int H, int W) { return cdiv(H, kMetTile) * cdiv(W, kMetTile); }
constexpr int kMetMaxExtent = 1 << 19;     // tile rows fit the grid's y extent

}  // namespace bds

using namespace bds;

extern "C" size_t bds_image_metrics_workspace_bytes(int H, int W) {
  if (H < kSsimWin || W < kSsimWin || H > kMetMaxExtent || W > kMetMaxExtent) return 0;
  return align_up((size_t)met_tiles(H, W) * kMetVals * sizeof(double), 256);
}

extern "C" int bds_image_metrics(int H, int W, const float *pred, const float *gt, const void *mask0, const void *mask1, const void *mask2,
                                 const void *mask3, int invert_bits, int mask_kind, float *ssim_map, double *out, void *ws, size_t ws_bytes,
                                 bds_stream_t stream) {
  BDS_REQUIRE(H >= kSsimWin && W >= kSsimWin && H <= kMetMaxExtent && W <= kMetMaxExtent);     // (skimage raises below 7 too)
  BDS_REQUIRE(pred && gt && out && (reinterpret_cast<uintptr_t>(out) & 7u) == 0);
  BDS_REQUIRE((mask_kind == 0 || mask_kind == 1) && invert_bits >= 0 && invert_bits < (1 << kMetSlots));
  MetMasks mk;
  const void *masks[kMetSlots] = {mask0, mask1, mask2, mask3};
  for (int s = 0; s < kMetSlots; s++) {
    mk.p[s] = masks[s];
    mk.invert[s] = (invert_bits >> s) & 1;
    BDS_REQUIRE(masks[s] != nullptr || !mk.invert[s]);
    BDS_REQUIRE(mask_kind == 0 || (reinterpret_cast<uintptr_t>(masks[s]) & 3u) == 0);
  }
  mk.kind = mask_kind;
  BDS_REQUIRE(ws && aligned16(ws));
  if (ws_bytes < bds_image_metrics_workspace_bytes(H, W)) return BDS_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)cdiv(W, kMetTile), (unsigned)cdiv(H, kMetTile));
  hipLaunchKernelGGL(metrics_tile_kernel, grid, dim3(kMetBlock), 0, st, H, W, pred, gt, mk, ssim_map, static_cast<double *>(ws));
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(1), dim3(kMetRedBlock), 0, st, H, W, met_tiles(H, W), static_cast<const double *>(ws), out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
