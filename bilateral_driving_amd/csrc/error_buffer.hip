// The error maps of the error-driven image sampler (CameraData.update_image_error_maps, datasets/base/pixel_source.py:431-449, and the
// per-image means of ScenePixelSource.update_image_error_maps :948-983) for B rendered views in one pass: where the reference copies
// every view to the host, stacks the lists per camera, forms the maps there and copies them back, the views stay on the device.  The
// per-pixel formula lives in error_buffer_math.h.
//   maps    view b is cut into P(h w) workgroups of 256 lanes (the same P for every view of a call: it depends on h w alone).  A lane
//           takes four neighbouring pixels at a time: three 16-byte loads of the render, three of the ground truth, one of the dynamic
//           opacity, one 16-byte store of the map -- the pass moves 28 + 4 bytes per pixel and does nothing else.  A view whose four
//           bases are not all 16-byte aligned (a [5,7] view behind another one, an offset tensor) takes the same pixels with 4-byte
//           accesses: the lanes, and with them the order of every sum, are the same on both paths.  The h w % 4 last pixels go to the
//           first lanes of the view's first workgroup.  Each workgroup leaves {sum in double, min, max} of its pixels in the workspace.
//   stats   one workgroup per view adds the P partials in a fixed order in double and writes {mean, min, max}: the mean is the double
//           sum divided by h w, rounded to float32 once.
// No atomics: bit-identical run to run, whatever order the workgroups retire in.  A slot outside [0, F) or an image id outside
// [0, num_imgs) -- both are read on the device -- drops that view's map or statistics; nothing is written out of bounds.
#include "bds_common.h"
#include "error_buffer_math.h"

namespace bds {

constexpr int kEbBlock = 256, kEbWaves = kEbBlock / kWave, kEbQuad = 4, kEbMaxParts = 1024;

struct alignas(16) EbPartial {
  double sum;
  float mn, mx;
};
static_assert(sizeof(EbPartial) == 16, "one 16-byte store per workgroup");

struct EbAcc {
  double sum;
  float mn, mx;
};

__device__ __forceinline__ void eb_take(EbAcc &a, float e) {
  a.sum += (double)e;
  a.mn = eb_min(a.mn, e);
  a.mx = eb_max(a.mx, e);
}

// the workgroup's lanes combined in a fixed order; the result is valid in lane 0 of wave 0
__device__ __forceinline__ EbAcc eb_block_reduce(EbAcc a, EbAcc (&s)[kEbWaves]) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    a.sum += __shfl_xor(a.sum, off);
    a.mn = eb_min(a.mn, __shfl_xor(a.mn, off));
    a.mx = eb_max(a.mx, __shfl_xor(a.mx, off));
  }
  const int tid = threadIdx.x;
  if ((tid & (kWave - 1)) == 0) s[tid / kWave] = a;
  __syncthreads();
  EbAcc r = s[0];
#pragma unroll
  for (int k = 1; k < kEbWaves; k++) {
    r.sum += s[k].sum;
    r.mn = eb_min(r.mn, s[k].mn);
    r.mx = eb_max(r.mx, s[k].mx);
  }
  return r;
}

// pixels [4 q, 4 q + 4) of one view; VEC: every base is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void eb_quad(int64_t q, const float *__restrict__ p, const float *__restrict__ g, const float *__restrict__ d,
                                        float *__restrict__ m, EbAcc &acc) {
  float pv[12], gv[12], dv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, e[4];
  if (VEC) {
    const float4 *p4 = reinterpret_cast<const float4 *>(p) + 3 * q, *g4 = reinterpret_cast<const float4 *>(g) + 3 * q;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float4 a = p4[k], b = g4[k];
      pv[4 * k] = a.x, pv[4 * k + 1] = a.y, pv[4 * k + 2] = a.z, pv[4 * k + 3] = a.w;
      gv[4 * k] = b.x, gv[4 * k + 1] = b.y, gv[4 * k + 2] = b.z, gv[4 * k + 3] = b.w;
    }
    if (d != nullptr) {
      const float4 a = reinterpret_cast<const float4 *>(d)[q];
      dv[0] = a.x, dv[1] = a.y, dv[2] = a.z, dv[3] = a.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) {
      pv[k] = p[12 * q + k];
      gv[k] = g[12 * q + k];
    }
    if (d != nullptr) {
#pragma unroll
      for (int k = 0; k < 4; k++) dv[k] = d[4 * q + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    e[k] = eb_pixel(pv[3 * k], pv[3 * k + 1], pv[3 * k + 2], gv[3 * k], gv[3 * k + 1], gv[3 * k + 2], d != nullptr, dv[k]);
    eb_take(acc, e[k]);
  }
  if (m != nullptr) {
    if (VEC) {
      reinterpret_cast<float4 *>(m)[q] = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) m[4 * q + k] = e[k];
    }
  }
}

__device__ __forceinline__ bool eb_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// grid: B * P workgroups; n = h w >= 1
__global__ __launch_bounds__(kEbBlock) void error_maps_kernel(int n, int P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                              const float *__restrict__ dyn, const int64_t *__restrict__ slots, int F,
                                                              float *__restrict__ maps, EbPartial *__restrict__ ws) {
  __shared__ EbAcc s[kEbWaves];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / P;
  const int blk = blockIdx.x - (int)b * P;
  const int64_t base = b * n;
  const float *p = pred + 3 * base, *g = gt + 3 * base;
  const float *d = dyn != nullptr ? dyn + base : nullptr;
  const int64_t slot = slots[b];
  float *m = (slot >= 0 && slot < F) ? maps + slot * n : nullptr;

  EbAcc acc = {0.0, INFINITY, -INFINITY};
  const int64_t nq = n / kEbQuad, step = (int64_t)P * kEbBlock;
  if (eb_aligned16(p) && eb_aligned16(g) && eb_aligned16(d) && eb_aligned16(m)) {
    for (int64_t q = (int64_t)blk * kEbBlock + tid; q < nq; q += step) eb_quad<true>(q, p, g, d, m, acc);
  } else {
    for (int64_t q = (int64_t)blk * kEbBlock + tid; q < nq; q += step) eb_quad<false>(q, p, g, d, m, acc);
  }
  const int64_t i = nq * kEbQuad + tid;      // the h w % 4 last pixels
  if (blk == 0 && i < n) {
    const float e = eb_pixel(p[3 * i], p[3 * i + 1], p[3 * i + 2], g[3 * i], g[3 * i + 1], g[3 * i + 2], d != nullptr, d != nullptr ? d[i] : 0.0f);
    eb_take(acc, e);
    if (m != nullptr) m[i] = e;
  }
  const EbAcc r = eb_block_reduce(acc, s);
  if (tid == 0) {
    EbPartial out;
    out.sum = r.sum, out.mn = r.mn, out.mx = r.mx;
    ws[blockIdx.x] = out;
  }
}

// grid: B workgroups.  n = 0 (P = 0): the mean of nothing, NaN, and with it the minimum and the maximum
__global__ __launch_bounds__(kEbBlock) void error_stats_kernel(int n, int P, const EbPartial *__restrict__ ws, const int64_t *__restrict__ img_ids,
                                                               int num_imgs, float *__restrict__ stats) {
  __shared__ EbAcc s[kEbWaves];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  EbAcc acc = {0.0, INFINITY, -INFINITY};
  for (int k = tid; k < P; k += kEbBlock) {
    const EbPartial part = ws[b * P + k];
    acc.sum += part.sum;
    acc.mn = eb_min(acc.mn, part.mn);
    acc.mx = eb_max(acc.mx, part.mx);
  }
  const EbAcc r = eb_block_reduce(acc, s);
  const int64_t id = img_ids[b];
  if (tid == 0 && id >= 0 && id < num_imgs) {
    float *row = stats + 3 * id;
    row[0] = n > 0 ? (float)(r.sum / (double)n) : NAN;
    row[1] = n > 0 ? r.mn : NAN;
    row[2] = n > 0 ? r.mx : NAN;
  }
}

static int eb_parts(int64_t n) {
  const int64_t p = cdiv(cdiv(n, kEbQuad), kEbBlock);
  return (int)(p < 1 ? 1 : (p > kEbMaxParts ? kEbMaxParts : p));
}
static bool eb_extents_ok(int B, int h, int w) {
  return B >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX && (int64_t)B * ((int64_t)h * w) <= INT32_MAX;
}

}  // namespace bds

using namespace bds;

extern "C" size_t bds_error_maps_workspace_bytes(int B, int h, int w) {
  if (!eb_extents_ok(B, h, w)) return 0;
  const int64_t n = (int64_t)h * w;
  if (B == 0 || n == 0) return 16;
  return align_up((size_t)B * eb_parts(n) * sizeof(EbPartial), 256);
}

extern "C" int bds_error_maps(int B, int h, int w, const float *pred, const float *gt, const float *dyn, const int64_t *slots,
                              const int64_t *img_ids, float *maps, int F, float *stats, int num_imgs, void *ws, size_t ws_bytes,
                              bds_stream_t stream) {
  BDS_REQUIRE(eb_extents_ok(B, h, w) && F >= 0 && num_imgs >= 0);
  if (B == 0) return BDS_OK;
  const int n = h * w;
  hipStream_t st = as_stream(stream);
  if (n == 0) {      // nothing to read; the views' statistics rows become NaN where the caller names them
    if (stats == nullptr || img_ids == nullptr) return BDS_OK;
    BDS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 3u) == 0 && (reinterpret_cast<uintptr_t>(img_ids) & 7u) == 0);
    hipLaunchKernelGGL(error_stats_kernel, dim3((unsigned)B), dim3(kEbBlock), 0, st, 0, 0, static_cast<const EbPartial *>(nullptr), img_ids,
                       num_imgs, stats);
    BDS_LAUNCH_CHECK();
    return BDS_OK;
  }
  BDS_REQUIRE(pred && gt && slots && img_ids && maps && stats && ws && aligned16(ws));
  BDS_REQUIRE(((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(dyn) |
                reinterpret_cast<uintptr_t>(maps) | reinterpret_cast<uintptr_t>(stats)) & 3u) == 0);
  BDS_REQUIRE(((reinterpret_cast<uintptr_t>(slots) | reinterpret_cast<uintptr_t>(img_ids)) & 7u) == 0);
  BDS_REQUIRE(ws_bytes >= bds_error_maps_workspace_bytes(B, h, w));
  const int P = eb_parts(n);
  BDS_REQUIRE((int64_t)B * P < (1 << 24));      // (a launch holds fewer than 2^32 lanes)
  hipLaunchKernelGGL(error_maps_kernel, dim3((unsigned)((int64_t)B * P)), dim3(kEbBlock), 0, st, n, P, pred, gt, dyn, slots, F, maps,
                     static_cast<EbPartial *>(ws));
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(error_stats_kernel, dim3((unsigned)B), dim3(kEbBlock), 0, st, n, P, static_cast<const EbPartial *>(ws), img_ids, num_imgs,
                     stats);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
