// Lidar scene preparation on the device (include/bds.h: bds_lidar_project, bds_lidar_visible, bds_lidar_points_in_boxes*,
// bds_lidar_depth_downsample): what DrivingDataset does with the lidar before step 0 (datasets/driving_dataset.py:280-416, 496-603,
// 644-727) and the sparse depth map's downsampler of every coarse-to-fine step (datasets/base/pixel_source.py:77-92).
//
// Every kernel takes one thread per point (per pixel in the resolve pass and the downsampler) and reads the small per-view / per-box
// tables through LDS, staged in chunks by the whole workgroup; all lanes of a wave read the same LDS address (a broadcast, no bank
// conflict).  Nothing adds floats atomically: the projection's only atomic is an integer max of the row, the boxes' emit form takes
// its offsets from a scan of per-point counts, so every output is bit-identical run to run.
#include "bds_common.h"
#include "lidar_math.h"
#include "scan.h"

namespace bds {

constexpr int kLidarBlock = 256;
constexpr int kLidarViewChunk = BDS_LIDAR_VIEW_CHUNK;
constexpr int kLidarBoxChunk = BDS_LIDAR_BOX_CHUNK;
constexpr int kLidarScanBlock = 1024;

struct LidarProjectArgs {
  int V, W, H;
  int64_t N;
  const float *points, *mats, *images;
  const int64_t *ranges;
  int32_t *winner, *pix;
  float *depth, *colors;
  uint8_t *visible;
};

// stages views [v0, v0 + n) of the launch: 12 floats and the row range, clamped to [0, N], of each
__device__ __forceinline__ void lidar_stage_views(const LidarProjectArgs &a, int v0, int n, float (*sm)[12], int (*sr)[2]) {
  for (int t = threadIdx.x; t < n * 12; t += blockDim.x) sm[t / 12][t % 12] = a.mats[(int64_t)v0 * 12 + t];
  for (int t = threadIdx.x; t < n * 2; t += blockDim.x) {
    int64_t r = a.ranges[(int64_t)v0 * 2 + t];
    r = r < 0 ? 0 : (r > a.N ? a.N : r);
    sr[t / 2][t % 2] = (int)r;
  }
}

// pass 1 (GATHER = false): the highest valid row of every pixel, by an integer atomicMax into the winner map.
// pass 3 (GATHER = true): per point the pixel of the LAST view that sees it, its visibility and the image's colour at that pixel.
template <bool GATHER>
__global__ __launch_bounds__(kLidarBlock) void lidar_points_kernel(LidarProjectArgs a) {
  __shared__ float sm[kLidarViewChunk][12];
  __shared__ int sr[kLidarViewChunk][2];
  const int64_t i = (int64_t)blockIdx.x * kLidarBlock + threadIdx.x;
  const bool live = i < a.N;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = a.points[3 * i];
    y = a.points[3 * i + 1];
    z = a.points[3 * i + 2];
  }
  int last = -1;
  for (int v0 = 0; v0 < a.V; v0 += kLidarViewChunk) {
    const int n = a.V - v0 < kLidarViewChunk ? a.V - v0 : kLidarViewChunk;
    __syncthreads();
    lidar_stage_views(a, v0, n, sm, sr);
    __syncthreads();
    if (!live) continue;
    for (int k = 0; k < n; k++) {
      if (i < sr[k][0] || i >= sr[k][1]) continue;
      int px, py;
      float d;
      if (!lidar_project(sm[k], x, y, z, a.W, a.H, &px, &py, &d)) continue;
      const int p = ((v0 + k) * a.H + py) * a.W + px;
      if (GATHER)
        last = p;
      else
        atomicMax(&a.winner[p], (int)i);
    }
  }
  if (GATHER && live) {
    a.pix[i] = last;
    if (last >= 0) {
      a.visible[i] = 1;
      if (a.images != nullptr && a.colors != nullptr) {
        a.colors[3 * i] = a.images[3 * (int64_t)last];
        a.colors[3 * i + 1] = a.images[3 * (int64_t)last + 1];
        a.colors[3 * i + 2] = a.images[3 * (int64_t)last + 2];
      }
    }
  }
}

// pass 2: the depth of every pixel's winner, recomputed from the point (the same expression as pass 1), 0 where no point landed
__global__ __launch_bounds__(kLidarBlock) void lidar_resolve_kernel(LidarProjectArgs a) {
  const int64_t total = (int64_t)a.V * a.H * a.W;
  const int64_t p = (int64_t)blockIdx.x * kLidarBlock + threadIdx.x;
  if (p >= total) return;
  const int w = a.winner[p];
  float d = 0.0f;
  if (w >= 0 && w < a.N) {
    const int v = (int)(p / ((int64_t)a.H * a.W));
    d = lidar_row(a.mats + (int64_t)v * 12 + 8, a.points[3 * (int64_t)w], a.points[3 * (int64_t)w + 1], a.points[3 * (int64_t)w + 2]);
  }
  a.depth[p] = d;
}

// check_pts_visibility: the OR of the valid test over V views with their own sizes
__global__ __launch_bounds__(kLidarBlock) void lidar_visible_kernel(int64_t N, const float *__restrict__ points, int V,
                                                                    const float *__restrict__ mats, const int32_t *__restrict__ sizes,
                                                                    uint8_t *__restrict__ visible) {
  __shared__ float sm[kLidarViewChunk][12];
  __shared__ int ss[kLidarViewChunk][2];
  const int64_t i = (int64_t)blockIdx.x * kLidarBlock + threadIdx.x;
  const bool live = i < N;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = points[3 * i];
    y = points[3 * i + 1];
    z = points[3 * i + 2];
  }
  bool seen = !live;      // (a lane past the end has nothing left to find)
  for (int v0 = 0; v0 < V; v0 += kLidarViewChunk) {
    const int n = V - v0 < kLidarViewChunk ? V - v0 : kLidarViewChunk;
    __syncthreads();
    for (int t = threadIdx.x; t < n * 12; t += blockDim.x) sm[t / 12][t % 12] = mats[(int64_t)v0 * 12 + t];
    for (int t = threadIdx.x; t < n * 2; t += blockDim.x) ss[t / 2][t % 2] = sizes[(int64_t)v0 * 2 + t];
    __syncthreads();
    if (__all(seen)) continue;      // wave-uniform: every point of the wave is already visible
    for (int k = 0; k < n; k++) {
      int px, py;
      float d;
      seen = seen || lidar_project(sm[k], x, y, z, ss[k][0], ss[k][1], &px, &py, &d);
    }
  }
  if (live) visible[i] = seen ? 1 : 0;
}

struct LidarBoxArgs {
  int64_t N;
  int B, chunk;
  const float *points, *w2o, *half;
  const int64_t *ranges;      // [B,2] or NULL (every row)
  const int32_t *ids;         // [B,2] (instance, frame): emit form
  uint8_t *inside;            // mask form
  int32_t *counts;            // [N]
  int64_t *block_off;         // [cdiv(N, kLidarBlock)]: the workgroups' sums, then their exclusive offsets
  int64_t capacity;
  int32_t *rec_ids;           // [capacity,3]
  float *rec_xyz;             // [capacity,3]
};

enum { kBoxMask = 0, kBoxCount = 1, kBoxEmit = 2 };

template <int MODE>
__global__ __launch_bounds__(kLidarBlock) void lidar_boxes_kernel(LidarBoxArgs a) {
  __shared__ float sm[kLidarBoxChunk][16];      // w2o 12, half 3, -
  __shared__ int sr[kLidarBoxChunk][2];
  __shared__ int scratch[kLidarBlock / kWave];
  const int64_t i = (int64_t)blockIdx.x * kLidarBlock + threadIdx.x;
  const bool live = i < a.N;
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    x = a.points[3 * i];
    y = a.points[3 * i + 1];
    z = a.points[3 * i + 2];
  }
  int64_t at = 0;
  if (MODE == kBoxEmit) {
    int total;
    at = a.block_off[blockIdx.x] + block_excl_scan<kLidarBlock / kWave>(live ? a.counts[i] : 0, total, scratch);
  }
  int found = 0;
  for (int b0 = 0; b0 < a.B; b0 += a.chunk) {
    const int n = a.B - b0 < a.chunk ? a.B - b0 : a.chunk;
    __syncthreads();
    for (int t = threadIdx.x; t < n * 16; t += blockDim.x) {
      const int k = t >> 4, c = t & 15;
      sm[k][c] = c < 12 ? a.w2o[(int64_t)(b0 + k) * 12 + c] : (c < 15 ? a.half[(int64_t)(b0 + k) * 3 + (c - 12)] : 0.0f);
    }
    for (int t = threadIdx.x; t < n * 2; t += blockDim.x) {
      int64_t r = a.ranges != nullptr ? a.ranges[(int64_t)b0 * 2 + t] : ((t & 1) ? a.N : 0);
      r = r < 0 ? 0 : (r > a.N ? a.N : r);
      sr[t >> 1][t & 1] = (int)r;
    }
    __syncthreads();
    if (!live) continue;
    if (MODE == kBoxMask && __all(found != 0)) continue;      // wave-uniform: the OR is already 1 for every point of the wave
    for (int k = 0; k < n; k++) {
      if (i < sr[k][0] || i >= sr[k][1]) continue;
      float o[3];
      if (!lidar_in_box(sm[k], sm[k] + 12, x, y, z, o)) continue;
      if (MODE == kBoxEmit) {
        if (at < a.capacity) {
          a.rec_ids[3 * at] = a.ids[2 * (int64_t)(b0 + k)];
          a.rec_ids[3 * at + 1] = a.ids[2 * (int64_t)(b0 + k) + 1];
          a.rec_ids[3 * at + 2] = (int32_t)i;
          a.rec_xyz[3 * at] = o[0];
          a.rec_xyz[3 * at + 1] = o[1];
          a.rec_xyz[3 * at + 2] = o[2];
        }
        at++;
      }
      found++;
    }
  }
  if (MODE == kBoxMask && live) a.inside[i] = found ? 1 : 0;
  if (MODE == kBoxCount) {
    if (live) a.counts[i] = found;
    int total;
    block_excl_scan<kLidarBlock / kWave>(live ? found : 0, total, scratch);
    if (threadIdx.x == 0) a.block_off[blockIdx.x] = total;
  }
}

// one workgroup: the workgroups' sums -> their exclusive offsets, in place; *total the number of records
__global__ __launch_bounds__(kLidarScanBlock) void lidar_scan_kernel(int64_t *__restrict__ block_off, int64_t nblk, int64_t *__restrict__ total) {
  __shared__ int64_t lw[kLidarScanBlock / kWave];
  int64_t sum;
  workgroup_scan_in_place<kLidarScanBlock>(block_off, nblk, &sum, lw);
  if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kLidarBlock) void lidar_downsample_kernel(int B, int H, int W, int Ho, int Wo, const float *__restrict__ in,
                                                                       float *__restrict__ out) {
  const int64_t cells = (int64_t)Ho * Wo, t = (int64_t)blockIdx.x * kLidarBlock + threadIdx.x;
  if (t >= cells * B) return;
  const int b = (int)(t / cells), i = (int)((t % cells) / Wo), j = (int)(t % Wo);
  out[t] = lidar_downsample_cell(in + (int64_t)b * H * W, H, W, Ho, Wo, i, j);
}

static bool lidar_al(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr int64_t kLidarMaxRows = 2147483647LL - kLidarBlock;      // rows and linear pixels are int32; the grid's last block may overhang

static size_t lidar_boxes_ws(int64_t N, int64_t *nblk_out) {
  const int64_t nblk = cdiv(N, kLidarBlock);
  if (nblk_out) *nblk_out = nblk;
  return align_up((size_t)nblk * 8, 16) + (size_t)N * 4;
}

static int lidar_box_args(LidarBoxArgs *a, int64_t N, const float *points, int B, const float *w2o, const float *half,
                          const int64_t *ranges, int chunk) {
  BDS_REQUIRE(N >= 0 && N <= kLidarMaxRows && B >= 0);
  BDS_REQUIRE(chunk >= 1 && chunk <= kLidarBoxChunk);
  if (N > 0) BDS_REQUIRE(points != nullptr);
  if (B > 0) BDS_REQUIRE(w2o != nullptr && half != nullptr);
  BDS_REQUIRE(lidar_al(points, 4) && lidar_al(w2o, 4) && lidar_al(half, 4) && lidar_al(ranges, 8));
  *a = LidarBoxArgs{};
  a->N = N;
  a->B = B;
  a->chunk = chunk;
  a->points = points;
  a->w2o = w2o;
  a->half = half;
  a->ranges = ranges;
  return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_lidar_project(int V, int W, int H, int64_t N, const float *points, const float *lidar2img, const int64_t *ranges,
                                 const float *images, int32_t *winner, float *depth, int32_t *pix, uint8_t *visible, float *colors,
                                 bds_stream_t stream) {
  BDS_REQUIRE(V >= 0 && N >= 0 && N <= kLidarMaxRows);
  if (V == 0 && N == 0) return BDS_OK;
  BDS_REQUIRE(W >= 1 && H >= 1 && (V == 0 || (int64_t)V * H * W <= kLidarMaxRows));
  if (V > 0) BDS_REQUIRE(lidar2img && ranges && winner && depth);
  if (N > 0) BDS_REQUIRE(points && pix && visible);
  BDS_REQUIRE((images == nullptr) == (colors == nullptr));
  BDS_REQUIRE(lidar_al(points, 4) && lidar_al(lidar2img, 4) && lidar_al(ranges, 8) && lidar_al(images, 4) && lidar_al(winner, 4) &&
              lidar_al(depth, 4) && lidar_al(pix, 4) && lidar_al(colors, 4));
  LidarProjectArgs a;
  a.V = V;
  a.W = W;
  a.H = H;
  a.N = N;
  a.points = points;
  a.mats = lidar2img;
  a.images = images;
  a.ranges = ranges;
  a.winner = winner;
  a.pix = pix;
  a.depth = depth;
  a.colors = colors;
  a.visible = visible;
  hipStream_t st = as_stream(stream);
  const int64_t pixels = (int64_t)V * H * W;
  const unsigned pgrid = (unsigned)cdiv(N, kLidarBlock);
  if (V > 0) {
    if (hipMemsetAsync(winner, 0xff, (size_t)pixels * 4, st) != hipSuccess) return BDS_ELAUNCH;      // every word -1
    if (N > 0) {
      hipLaunchKernelGGL(lidar_points_kernel<false>, dim3(pgrid), dim3(kLidarBlock), 0, st, a);
      BDS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lidar_resolve_kernel, dim3((unsigned)cdiv(pixels, kLidarBlock)), dim3(kLidarBlock), 0, st, a);
    BDS_LAUNCH_CHECK();
  }
  if (N > 0) {
    hipLaunchKernelGGL(lidar_points_kernel<true>, dim3(pgrid), dim3(kLidarBlock), 0, st, a);
    BDS_LAUNCH_CHECK();
  }
  return BDS_OK;
}

extern "C" int bds_lidar_visible(int64_t N, const float *points, int V, const float *lidar2img, const int32_t *sizes, uint8_t *visible,
                                 bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N <= kLidarMaxRows && V >= 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(points && visible);
  if (V > 0) BDS_REQUIRE(lidar2img && sizes);
  BDS_REQUIRE(lidar_al(points, 4) && lidar_al(lidar2img, 4) && lidar_al(sizes, 4));
  hipLaunchKernelGGL(lidar_visible_kernel, dim3((unsigned)cdiv(N, kLidarBlock)), dim3(kLidarBlock), 0, as_stream(stream), N, points, V,
                     lidar2img, sizes, visible);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_lidar_points_in_boxes(int64_t N, const float *points, int B, const float *w2o, const float *half,
                                         const int64_t *ranges, int chunk, uint8_t *inside, bds_stream_t stream) {
  LidarBoxArgs a;
  const int rc = lidar_box_args(&a, N, points, B, w2o, half, ranges, chunk);
  if (rc != BDS_OK) return rc;
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(inside != nullptr);
  a.inside = inside;
  hipLaunchKernelGGL(lidar_boxes_kernel<kBoxMask>, dim3((unsigned)cdiv(N, kLidarBlock)), dim3(kLidarBlock), 0, as_stream(stream), a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" size_t bds_lidar_boxes_workspace_bytes(int64_t N) {
  if (N < 1 || N > kLidarMaxRows) return 0;
  return lidar_boxes_ws(N, nullptr);
}

extern "C" int bds_lidar_points_in_boxes_count(int64_t N, const float *points, int B, const float *w2o, const float *half,
                                               const int64_t *ranges, int chunk, int64_t *total, void *ws, size_t ws_bytes,
                                               bds_stream_t stream) {
  LidarBoxArgs a;
  const int rc = lidar_box_args(&a, N, points, B, w2o, half, ranges, chunk);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(total != nullptr && lidar_al(total, 8));
  hipStream_t st = as_stream(stream);
  if (N == 0) return hipMemsetAsync(total, 0, 8, st) == hipSuccess ? BDS_OK : BDS_ELAUNCH;
  BDS_REQUIRE(ws != nullptr && aligned16(ws));
  int64_t nblk;
  if (ws_bytes < lidar_boxes_ws(N, &nblk)) return BDS_EWORKSPACE;
  a.block_off = reinterpret_cast<int64_t *>(ws);
  a.counts = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(ws) + align_up((size_t)nblk * 8, 16));
  hipLaunchKernelGGL(lidar_boxes_kernel<kBoxCount>, dim3((unsigned)nblk), dim3(kLidarBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(lidar_scan_kernel, dim3(1), dim3(kLidarScanBlock), 0, st, a.block_off, nblk, total);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_lidar_points_in_boxes_emit(int64_t N, const float *points, int B, const float *w2o, const float *half,
                                              const int64_t *ranges, const int32_t *ids, int chunk, const void *ws, size_t ws_bytes,
                                              int64_t capacity, int32_t *rec_ids, float *rec_xyz, bds_stream_t stream) {
  LidarBoxArgs a;
  const int rc = lidar_box_args(&a, N, points, B, w2o, half, ranges, chunk);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(capacity >= 0);
  if (N == 0 || B == 0 || capacity == 0) return BDS_OK;
  BDS_REQUIRE(ids && rec_ids && rec_xyz && ws && aligned16(ws));
  BDS_REQUIRE(lidar_al(ids, 4) && lidar_al(rec_ids, 4) && lidar_al(rec_xyz, 4));
  int64_t nblk;
  if (ws_bytes < lidar_boxes_ws(N, &nblk)) return BDS_EWORKSPACE;
  a.block_off = reinterpret_cast<int64_t *>(const_cast<void *>(ws));
  a.counts = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(const_cast<void *>(ws)) + align_up((size_t)nblk * 8, 16));
  a.ids = ids;
  a.capacity = capacity;
  a.rec_ids = rec_ids;
  a.rec_xyz = rec_xyz;
  hipLaunchKernelGGL(lidar_boxes_kernel<kBoxEmit>, dim3((unsigned)nblk), dim3(kLidarBlock), 0, as_stream(stream), a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_lidar_depth_downsample(int B, int H, int W, int Ho, int Wo, const float *in, float *out, bds_stream_t stream) {
  BDS_REQUIRE(B >= 0 && H >= 1 && W >= 1 && Ho >= 0 && Wo >= 0);
  BDS_REQUIRE((int64_t)B * H * W <= kLidarMaxRows && (int64_t)B * Ho * Wo <= kLidarMaxRows);
  if (B == 0 || Ho == 0 || Wo == 0) return BDS_OK;
  BDS_REQUIRE(in && out && lidar_al(in, 4) && lidar_al(out, 4));
  hipLaunchKernelGGL(lidar_downsample_kernel, dim3((unsigned)cdiv((int64_t)B * Ho * Wo, kLidarBlock)), dim3(kLidarBlock), 0,
                     as_stream(stream), B, H, W, Ho, Wo, in, out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
