// A view's input preparation on the device (include/bds.h: bds_view_fields, bds_image_resize_aa, bds_masks_resize_nearest): what
// CameraData.get_image (datasets/base/pixel_source.py:477-657, with get_rays :38-75) does in front of every training step and every
// evaluation render, and ScenePixelSource.prepare_novel_view_render_data (:1070-1132) for a novel trajectory.
//
// view_fields_kernel is write-bound: 64 bytes per pixel, no LDS, no atomics.  The B views' pixels lie flat, [B, H W]; a lane owns four
// consecutive pixels whose first has a flat index divisible by four, so every store is 16 bytes and 16-byte aligned (48 bytes of a
// 3-float field, 32 of an int64 field); the up to three pixels in front of a view's first such group and the up to three behind its
// last go one pixel per lane through scalar stores.  blockIdx.y is the view: pose, intrinsics, time and ids are wave-uniform loads.
// image_resize_aa_kernel: a workgroup owns an output tile, computes its column and row windows with their normalised weights into
// LDS, runs the width pass for the input rows the tile needs into LDS and the height pass from there.
#include "bds_common.h"
#include "pixels_math.h"

namespace bds {

constexpr int kPxBlock = 256;
constexpr int64_t kPxMaxRows = 2147483647LL - 256;      // flat pixels are 32-bit; the grid's last block may overhang
constexpr int kPxMaxMasks = BDS_PIXELS_MAX_MASKS;
constexpr int kPxTileH = 8, kPxTileW = 32;              // the resize's largest output tile
constexpr size_t kPxLdsBudget = 48 * 1024;              // three workgroups per CU

struct ViewFieldsArgs {
  int H, W, n_intr;
  float scale;
  float *origins, *viewdirs, *norm, *coords, *time_out, *intr_out;
  int64_t *img, *frame, *cam;
};

__device__ __forceinline__ void px_store4(float *dst, const float *v) {
  *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void px_fill4(int64_t *dst, int64_t v) {
  const longlong2 q = make_longlong2(v, v);
  reinterpret_cast<longlong2 *>(dst)[0] = q;
  reinterpret_cast<longlong2 *>(dst)[1] = q;
}

// The inputs are parameters of their own, const and __restrict__: nothing the kernel stores can alias them, so the compiler takes the
// view's pose, intrinsics, time and ids with scalar loads, once per wave, into SGPRs (a member of the struct next to the outputs is
// reloaded per lane with vector loads of one address).
__global__ __launch_bounds__(kPxBlock) void view_fields_kernel(ViewFieldsArgs a, const float *__restrict__ c2w, const float *__restrict__ intr,
                                                               const float *__restrict__ time_in, const int64_t *__restrict__ ids) {
  const int b = blockIdx.y;
  const uint32_t P = (uint32_t)a.H * (uint32_t)a.W;
  const uint32_t g0 = (uint32_t)b * P;                 // the view's first flat pixel
  uint32_t head = (4u - (g0 & 3u)) & 3u;               // pixels in front of the first aligned group
  head = head < P ? head : P;
  const uint32_t groups = (P - head) >> 2, tail = (P - head) & 3u;
  const uint32_t k = blockIdx.x * (uint32_t)kPxBlock + threadIdx.x;
  const float *K = intr + (a.n_intr > 1 ? 9 * (int64_t)b : 0);
  if (a.intr_out != nullptr && k < 9) a.intr_out[9 * (int64_t)b + k] = px_scaled_intrinsic(K, a.scale, (int)k);
  if (k >= groups + head + tail) return;
  const PxCamera c = px_camera(c2w + 16 * (int64_t)b, K, a.scale);
  const float tm = a.time_out != nullptr ? time_in[b] : 0.0f;
  const int64_t id_img = a.img != nullptr ? ids[3 * (int64_t)b] : 0;
  const int64_t id_frame = a.frame != nullptr ? ids[3 * (int64_t)b + 1] : 0;
  const int64_t id_cam = a.cam != nullptr ? ids[3 * (int64_t)b + 2] : 0;
  if (k < groups) {
    const uint32_t p = head + 4u * k;
    const int64_t g = (int64_t)g0 + p;                 // divisible by four
    int y = (int)(p / (uint32_t)a.W), x = (int)(p - (uint32_t)y * (uint32_t)a.W);
    float dirs[12], nrm[4], rc[8];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      px_ray(c, x, y, dirs + 3 * q, nrm + q);
      px_coords(x, y, a.H, a.W, rc + 2 * q);
      if (++x == a.W) {
        x = 0;
        y++;
      }
    }
    if (a.viewdirs != nullptr) {
      px_store4(a.viewdirs + 3 * g, dirs);
      px_store4(a.viewdirs + 3 * g + 4, dirs + 4);
      px_store4(a.viewdirs + 3 * g + 8, dirs + 8);
    }
    if (a.origins != nullptr) {
      const float o0[4] = {c.t[0], c.t[1], c.t[2], c.t[0]}, o1[4] = {c.t[1], c.t[2], c.t[0], c.t[1]}, o2[4] = {c.t[2], c.t[0], c.t[1], c.t[2]};
      px_store4(a.origins + 3 * g, o0);
      px_store4(a.origins + 3 * g + 4, o1);
      px_store4(a.origins + 3 * g + 8, o2);
    }
    if (a.norm != nullptr) px_store4(a.norm + g, nrm);
    if (a.coords != nullptr) {
      px_store4(a.coords + 2 * g, rc);
      px_store4(a.coords + 2 * g + 4, rc + 4);
    }
    if (a.time_out != nullptr) {
      const float t4[4] = {tm, tm, tm, tm};
      px_store4(a.time_out + g, t4);
    }
    if (a.img != nullptr) px_fill4(a.img + g, id_img);
    if (a.frame != nullptr) px_fill4(a.frame + g, id_frame);
    if (a.cam != nullptr) px_fill4(a.cam + g, id_cam);
    return;
  }
  // one pixel of the view's unaligned head or tail
  const uint32_t j = k - groups;
  const uint32_t p = j < head ? j : head + 4u * groups + (j - head);
  const int64_t g = (int64_t)g0 + p;
  const int y = (int)(p / (uint32_t)a.W), x = (int)(p - (uint32_t)y * (uint32_t)a.W);
  float dir[3], nrm, rc[2];
  px_ray(c, x, y, dir, &nrm);
  px_coords(x, y, a.H, a.W, rc);
  for (int i = 0; i < 3; i++) {
    if (a.viewdirs != nullptr) a.viewdirs[3 * g + i] = dir[i];
    if (a.origins != nullptr) a.origins[3 * g + i] = c.t[i];
  }
  if (a.norm != nullptr) a.norm[g] = nrm;
  if (a.coords != nullptr) {
    a.coords[2 * g] = rc[0];
    a.coords[2 * g + 1] = rc[1];
  }
  if (a.time_out != nullptr) a.time_out[g] = tm;
  if (a.img != nullptr) a.img[g] = id_img;
  if (a.frame != nullptr) a.frame[g] = id_frame;
  if (a.cam != nullptr) a.cam[g] = id_cam;
}

// The LDS of one resize workgroup: the windows' starts, lengths and weight sums, the weight rows, the width pass's result.
struct ResizePlan {
  int th, tw, taps, rows;      // output tile, a weight row's length, input rows the tile can need
  size_t bytes;
};

static ResizePlan resize_plan(float scale) {
  ResizePlan p;
  p.th = kPxTileH;
  p.tw = kPxTileW;
  p.taps = px_aa_max_taps(scale);
  for (;;) {
    p.rows = (int)((float)(p.th - 1) * scale) + p.taps + 2;      // the last window's start - the first's, plus one window
    p.bytes = ((size_t)3 * (p.tw + p.th) + (size_t)(p.tw + p.th) * p.taps + (size_t)p.rows * p.tw * 3) * 4;
    if (p.bytes <= kPxLdsBudget || (p.th == 1 && p.tw == 1)) return p;
    if (p.th > 1)
      p.th >>= 1;
    else
      p.tw >>= 1;
  }
}

__global__ __launch_bounds__(kPxBlock) void image_resize_aa_kernel(int H, int W, int Ho, int Wo, float scale, ResizePlan plan,
                                                                   const float *__restrict__ in, float *__restrict__ out) {
  extern __shared__ __align__(16) unsigned char px_lds[];
  const int th = plan.th, tw = plan.tw;
  const int nw = tw + th;      // the tile's windows: its columns, then its rows
  int *win_lo = reinterpret_cast<int *>(px_lds), *win_n = win_lo + nw;
  float *total = reinterpret_cast<float *>(win_n + nw), *wcol = total + nw, *wrow = wcol + tw * plan.taps, *mid = wrow + th * plan.taps;
  const int *col_lo = win_lo, *col_n = win_n, *row_lo = win_lo + tw, *row_n = win_n + tw;
  const int ox0 = blockIdx.x * tw, oy0 = blockIdx.y * th, t = threadIdx.x;
  // windows: one lane each; their weights: one lane per tap; the sums in tap order, as px_aa_weights takes them: one lane each
  for (int i = t; i < nw; i += kPxBlock) {
    const int o = i < tw ? ox0 + i : oy0 + (i - tw);
    int lo = 0, n = 0;
    if (o < (i < tw ? Wo : Ho)) {
      px_aa_window(o, scale, i < tw ? W : H, &lo, &n);
      n = n < 0 ? 0 : (n > plan.taps ? plan.taps : n);
    }
    win_lo[i] = lo;
    win_n[i] = n;
  }
  __syncthreads();
  for (int e = t; e < nw * plan.taps; e += kPxBlock) {
    const int i = e / plan.taps, j = e - i * plan.taps;
    if (j < win_n[i]) wcol[e] = px_aa_weight(i < tw ? ox0 + i : oy0 + (i - tw), j, win_lo[i], scale);
  }
  __syncthreads();
  for (int i = t; i < nw; i += kPxBlock) {
    float sum = 0.0f;
    for (int j = 0; j < win_n[i]; j++) sum += wcol[i * plan.taps + j];
    total[i] = sum;
  }
  __syncthreads();
  for (int e = t; e < nw * plan.taps; e += kPxBlock) {
    const int i = e / plan.taps;
    if (e - i * plan.taps < win_n[i]) wcol[e] = wcol[e] / total[i];
  }
  __syncthreads();
  // the input rows of the tile: the windows' starts and ends do not decrease with the output row
  const int last = (Ho - oy0 < th ? Ho - oy0 : th) - 1;
  const int r0 = row_lo[0];
  int nrows = row_lo[last] + row_n[last] - r0;
  nrows = nrows < plan.rows ? nrows : plan.rows;
  const int line = tw * 3;
  for (int i = t; i < nrows * line; i += kPxBlock) {
    const int r = i / line, e = i - r * line, cx = e / 3, ch = e - cx * 3;
    const int n = col_n[cx];
    const float *src = in + ((int64_t)(r0 + r) * W + col_lo[cx]) * 3 + ch, *w = wcol + cx * plan.taps;
    float acc = 0.0f;
    {
#pragma clang fp contract(off)
      for (int j = 0; j < n; j++) acc += w[j] * src[3 * j];
    }
    mid[i] = acc;
  }
  __syncthreads();
  for (int i = t; i < th * line; i += kPxBlock) {
    const int r = i / line, e = i - r * line, cx = e / 3;
    const int oy = oy0 + r, ox = ox0 + cx;
    if (oy >= Ho || ox >= Wo) continue;
    const int first = row_lo[r] - r0;
    int n = row_n[r];
    n = first + n <= nrows ? n : nrows - first;
    const float *w = wrow + r * plan.taps;
    float acc = 0.0f;
    {
#pragma clang fp contract(off)
      for (int j = 0; j < n; j++) acc += w[j] * mid[(first + j) * line + e];
    }
    out[((int64_t)oy * Wo + ox) * 3 + (e - cx * 3)] = acc;
  }
}

struct MaskArgs {
  const float *in[kPxMaxMasks];
  float *out[kPxMaxMasks];
};

__global__ __launch_bounds__(kPxBlock) void masks_resize_nearest_kernel(int H, int W, int Ho, int Wo, float scale, MaskArgs m) {
  const uint32_t t = blockIdx.x * (uint32_t)kPxBlock + threadIdx.x;
  if (t >= (uint32_t)Ho * (uint32_t)Wo) return;
  const int oy = (int)(t / (uint32_t)Wo), ox = (int)(t - (uint32_t)oy * (uint32_t)Wo);
  const int64_t src = (int64_t)px_nearest(oy, scale, H) * W + px_nearest(ox, scale, W);
  m.out[blockIdx.y][t] = m.in[blockIdx.y][src];
}

static bool px_al(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// 0 < factor <= 1: the reference never enlarges; floor(n * factor) in double, as F.interpolate(scale_factor=factor) takes it
static bool px_factor_ok(double factor) { return factor > 0.0 && factor <= 1.0; }
static int px_out_size(int n, double factor) { return (int)floor((double)n * factor); }

}  // namespace bds

using namespace bds;

extern "C" int bds_view_fields(int B, int H, int W, const float *c2w, const float *intrinsics, int n_intrinsics, float scale,
                               const float *normed_time, const int64_t *ids, float *origins, float *viewdirs, float *direction_norm,
                               float *pixel_coords, float *normed_time_out, int64_t *img_idx, int64_t *frame_idx, int64_t *cam_id,
                               float *intrinsics_out, bds_stream_t stream) {
  BDS_REQUIRE(B >= 0 && B <= 65535 && H >= 0 && W >= 0);
  if (B == 0 || H == 0 || W == 0) return BDS_OK;
  BDS_REQUIRE((int64_t)H * W <= kPxMaxRows && (int64_t)B * H * W <= kPxMaxRows);
  BDS_REQUIRE(c2w != nullptr && intrinsics != nullptr && (n_intrinsics == 1 || n_intrinsics == B));
  BDS_REQUIRE(scale > 0.0f && scale <= 3.0e38f);
  if (normed_time_out != nullptr) BDS_REQUIRE(normed_time != nullptr);
  if (img_idx != nullptr || frame_idx != nullptr || cam_id != nullptr) BDS_REQUIRE(ids != nullptr);
  BDS_REQUIRE(px_al(c2w, 4) && px_al(intrinsics, 4) && px_al(normed_time, 4) && px_al(ids, 8) && px_al(intrinsics_out, 4));
  BDS_REQUIRE(aligned16(origins) && aligned16(viewdirs) && aligned16(direction_norm) && aligned16(pixel_coords) &&
              aligned16(normed_time_out) && aligned16(img_idx) && aligned16(frame_idx) && aligned16(cam_id));
  ViewFieldsArgs a;
  a.H = H;
  a.W = W;
  a.n_intr = n_intrinsics;
  a.scale = scale;
  a.origins = origins;
  a.viewdirs = viewdirs;
  a.norm = direction_norm;
  a.coords = pixel_coords;
  a.time_out = normed_time_out;
  a.intr_out = intrinsics_out;
  a.img = img_idx;
  a.frame = frame_idx;
  a.cam = cam_id;
  const int64_t lanes = (int64_t)H * W / 4 + 6;      // the groups of a view, its head and its tail; the first nine also write the intrinsics
  hipLaunchKernelGGL(view_fields_kernel, dim3((unsigned)cdiv(lanes, kPxBlock), (unsigned)B), dim3(kPxBlock), 0, as_stream(stream), a,
                     c2w, intrinsics, normed_time, ids);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_image_resize_aa(int H, int W, double factor, const float *in, float *out, bds_stream_t stream) {
  BDS_REQUIRE(H >= 0 && W >= 0 && px_factor_ok(factor) && (int64_t)H * W * 3 <= kPxMaxRows);
  const int Ho = px_out_size(H, factor), Wo = px_out_size(W, factor);
  if (Ho == 0 || Wo == 0) return BDS_OK;
  BDS_REQUIRE(in != nullptr && out != nullptr && px_al(in, 4) && px_al(out, 4));
  const float scale = (float)(1.0 / factor);
  BDS_REQUIRE(scale >= 1.0f && scale <= (float)BDS_PIXELS_MAX_SCALE);      // (a 1 x 1 tile at that scale stages 41 KB)
  const ResizePlan plan = resize_plan(scale);
  BDS_REQUIRE(plan.bytes <= 64 * 1024);
  hipLaunchKernelGGL(image_resize_aa_kernel, dim3((unsigned)cdiv(Wo, plan.tw), (unsigned)cdiv(Ho, plan.th)), dim3(kPxBlock), plan.bytes,
                     as_stream(stream), H, W, Ho, Wo, scale, plan, in, out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_masks_resize_nearest(int n, int H, int W, double factor, const float *const *in, float *const *out,
                                        bds_stream_t stream) {
  BDS_REQUIRE(n >= 0 && n <= kPxMaxMasks && H >= 0 && W >= 0 && px_factor_ok(factor) && (int64_t)H * W <= kPxMaxRows);
  const int Ho = px_out_size(H, factor), Wo = px_out_size(W, factor);
  if (n == 0 || Ho == 0 || Wo == 0) return BDS_OK;
  BDS_REQUIRE(in != nullptr && out != nullptr);
  MaskArgs m = {};
  for (int i = 0; i < n; i++) {
    BDS_REQUIRE(in[i] != nullptr && out[i] != nullptr && px_al(in[i], 4) && px_al(out[i], 4));
    m.in[i] = in[i];
    m.out[i] = out[i];
  }
  const float scale = (float)(1.0 / factor);
  hipLaunchKernelGGL(masks_resize_nearest_kernel, dim3((unsigned)cdiv((int64_t)Ho * Wo, kPxBlock), (unsigned)n), dim3(kPxBlock), 0,
                     as_stream(stream), H, W, Ho, Wo, scale, m);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
