// Pseudo-lidar generation on the device (include/bds.h: bds_pseudo_lidar_from_depth, bds_pseudo_lidar_from_points): a rendered depth
// map, or a cloud, binned into an H x W angular map of beams in which the highest pixel (row) index wins a beam, and the occupied
// beams emitted in beam order (generate_lidar/generate_lidar_from_depth.py:42-162, generate_lidar/depth2lidar.py:41-90).
//
// The recipe is the lidar scene preparation's (csrc/lidar.hip) in the other direction, from image to sensor: the bin kernel pins the
// winner of every beam by an integer atomicMax of the pixel index, the emit kernel ranks the occupied beams of the kept rows with
// scan.h and recomputes each winner's coordinates with the header function the bin kernel used (the same bits).  No float atomics:
// every output is bit-identical run to run.
//
// Atomics.  A 1080p image puts ~250 pixels into each of 8192 beams, and neighbouring pixels of an image row mostly share a beam.  A
// lane therefore issues its atomic only when the next higher lane of its wave is dead or has another cell: inside such a run of lanes
// the last one holds the highest index, so the map is the one that an atomic per pixel gives (9x faster than that on six 1080p maps:
// DESIGN.md section 7, profiles/pseudo_lidar_atomics_ab.json).
#include "bds_common.h"
#include "pseudo_lidar_math.h"
#include "scan.h"

namespace bds {

#ifndef BDS_PL_RUNS
#define BDS_PL_RUNS 1      // 0 (A/B builds only, build.py --variant): one atomic per live pixel
#endif

constexpr int kPlBlock = 256;
constexpr int kPlItems = 4;      // consecutive cells per thread and scan pass of the emit kernel
constexpr int64_t kPlMaxRows = 2147483647LL - kPlBlock;      // pixels, rows, cells and emitted floats are int32 (lidar.MAX_ROWS)

struct PlArgs {
  int Hi, Wi;             // the depth maps' size (depth source)
  int N;                  // keys per camera: Hi * Wi pixels, or the cloud's rows
  int H, W, slice, mode, crop, cap;
  const float *src;       // depth [C,Hi,Wi], or the cloud [N,4]
  const float *cams;      // [C,16] (depth source)
  const double *beams;    // [kPlBeams]
  int32_t *winner;        // [C,H,W]
  float *points;          // [C,cap,3] / [cap,4]
  int32_t *counts;        // [C]
  int32_t *source;        // [C,cap] or NULL
};

// One thread per key (pixel or cloud row), camera blockIdx.y: the highest live key of every beam.
template <bool CLOUD>
__global__ __launch_bounds__(kPlBlock) void pseudo_lidar_bin_kernel(PlArgs a) {
  const int c = blockIdx.y;
  const int64_t t = (int64_t)blockIdx.x * kPlBlock + threadIdx.x;
  const int key = (int)t;
  int cell = -1;
  if (t < a.N) {
    if (CLOUD) {
      const float4 q = reinterpret_cast<const float4 *>(a.src)[key];
      const float p[4] = {q.x, q.y, q.z, q.w};
      cell = pl_point_cell(a.beams, a.crop, a.H, a.W, a.mode, p);
    } else {
      float p[3];
      cell = pl_pixel_cell(a.cams + (int64_t)c * kPlCamFloats, a.beams, a.H, a.W, a.mode, key % a.Wi, key / a.Wi,
                           a.src[(int64_t)c * a.N + key], p);
    }
  }
  const int next = __shfl_down(cell, 1);      // (every lane of the wave is here: none has returned)
  const bool last = !BDS_PL_RUNS || (threadIdx.x & (kWave - 1)) == kWave - 1 || next != cell;
  if (cell >= 0 && last) atomicMax(&a.winner[(int64_t)c * a.H * a.W + cell], key);
}

// One workgroup per camera, over its cells in cell order: the occupied cells of the kept rows (row % slice == 0) take their rank from
// a scan per pass of kPlBlock * kPlItems cells, and each writes its winner's coordinates there.
template <bool CLOUD>
__global__ __launch_bounds__(kPlBlock) void pseudo_lidar_emit_kernel(PlArgs a) {
  __shared__ int lds_w[kPlBlock / kWave];
  const int c = blockIdx.x, cells = a.H * a.W;
  const int32_t *win = a.winner + (int64_t)c * cells;
  const float *cam = CLOUD ? nullptr : a.cams + (int64_t)c * kPlCamFloats;
  int base = 0;
  for (int c0 = 0; c0 < cells; c0 += kPlBlock * kPlItems) {
    const int first = c0 + threadIdx.x * kPlItems;
    int w[kPlItems], n = 0;
#pragma unroll
    for (int k = 0; k < kPlItems; k++) {
      const int cell = first + k;
      w[k] = -1;
      if (cell < cells && (cell / a.W) % a.slice == 0) w[k] = win[cell];
      if (w[k] >= a.N) w[k] = -1;
      n += w[k] >= 0 ? 1 : 0;
    }
    int total;
    int at = base + block_excl_scan<kPlBlock / kWave>(n, total, lds_w);
#pragma unroll
    for (int k = 0; k < kPlItems; k++) {
      if (w[k] < 0) continue;
      const int64_t o = (int64_t)c * a.cap + at;
      if (CLOUD) {
        reinterpret_cast<float4 *>(a.points)[o] = reinterpret_cast<const float4 *>(a.src)[w[k]];
      } else {
        float pc[3], p[3];
        pl_unproject(cam, w[k] % a.Wi, w[k] / a.Wi, a.src[(int64_t)c * a.N + w[k]], a.beams[kPlMaxDepth], pc);
        pl_to_lidar(cam, pc, p);
        a.points[3 * o] = p[0];
        a.points[3 * o + 1] = p[1];
        a.points[3 * o + 2] = p[2];
      }
      if (a.source != nullptr) a.source[o] = w[k];
      at++;
    }
    base += total;
  }
  if (threadIdx.x == 0) a.counts[c] = base;
}

static bool pl_al(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks both entries share, and the launches
template <bool CLOUD>
static int pl_run(PlArgs &a, int C, hipStream_t st) {
  BDS_REQUIRE(a.H >= 1 && a.W >= 1 && a.slice >= 1 && (a.mode == kPlVertical || a.mode == kPlClassic));
  BDS_REQUIRE((int64_t)C * a.H * a.W <= kPlMaxRows);
  const int64_t cap = cdiv(a.H, a.slice) * a.W;
  BDS_REQUIRE((int64_t)C * cap * 4 <= kPlMaxRows);
  a.cap = (int)cap;
  BDS_REQUIRE(a.beams && a.winner && a.points && a.counts);
  BDS_REQUIRE(pl_al(a.beams, 8) && pl_al(a.winner, 4) && pl_al(a.points, CLOUD ? 16 : 4) && pl_al(a.counts, 4) && pl_al(a.source, 4));
  if (hipMemsetAsync(a.winner, 0xff, (size_t)C * a.H * a.W * 4, st) != hipSuccess) return BDS_ELAUNCH;      // every word -1
  if (a.N > 0) {
    hipLaunchKernelGGL(pseudo_lidar_bin_kernel<CLOUD>, dim3((unsigned)cdiv(a.N, kPlBlock), (unsigned)C), dim3(kPlBlock), 0, st, a);
    BDS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pseudo_lidar_emit_kernel<CLOUD>, dim3((unsigned)C), dim3(kPlBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_pseudo_lidar_from_depth(int C, int Hi, int Wi, const float *depth, const float *cams, const double *beams, int H,
                                           int W, int slice, int mode, int32_t *winner, float *points, int32_t *counts,
                                           int32_t *source, bds_stream_t stream) {
  BDS_REQUIRE(C >= 0 && C <= 65535);
  if (C == 0) return BDS_OK;
  BDS_REQUIRE(Hi >= 1 && Wi >= 1 && (int64_t)C * Hi * Wi <= kPlMaxRows);
  BDS_REQUIRE(depth && cams && pl_al(depth, 4) && pl_al(cams, 4));
  PlArgs a{};
  a.Hi = Hi;
  a.Wi = Wi;
  a.N = Hi * Wi;
  a.H = H;
  a.W = W;
  a.slice = slice;
  a.mode = mode;
  a.crop = 1;
  a.src = depth;
  a.cams = cams;
  a.beams = beams;
  a.winner = winner;
  a.points = points;
  a.counts = counts;
  a.source = source;
  return pl_run<false>(a, C, as_stream(stream));
}

extern "C" int bds_pseudo_lidar_from_points(int64_t N, const float *cloud, const double *beams, int crop, int H, int W, int slice,
                                            int mode, int32_t *winner, float *points, int32_t *counts, int32_t *source,
                                            bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N <= kPlMaxRows && (crop == 0 || crop == 1));
  if (N > 0) BDS_REQUIRE(cloud != nullptr);
  BDS_REQUIRE(pl_al(cloud, 16));
  PlArgs a{};
  a.N = (int)N;
  a.H = H;
  a.W = W;
  a.slice = slice;
  a.mode = mode;
  a.crop = crop;
  a.src = cloud;
  a.beams = beams;
  a.winner = winner;
  a.points = points;
  a.counts = counts;
  a.source = source;
  return pl_run<true>(a, 1, as_stream(stream));
}
