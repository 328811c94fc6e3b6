// Evaluation geometry metrics of one frame (models/video_utils.py:363-536, utils/chamfer_distance.py:34-75): the Chamfer distance
// between the unprojected lidar depth and the unprojected rendered depth, whole-frame and per class, and the depth errors, where the
// reference calls pytorch3d's knn_points six times, sorts three arrays and reads thirty values back.  The per-element math lives in
// geometry_math.h.
//   flag     per pixel the validity test and the five class bits, one byte; per 256-pixel workgroup the six counts
//   scan     one workgroup turns the six count arrays into exclusive offsets and leaves the six totals on the device
//   scatter  ORDERED compaction in row-major order (offset of the workgroup + ballot rank inside it: no inter-workgroup wait): the
//            two point arrays, |pred - gt|, and per class the list of its points' positions in those arrays
//   nn       the pair loop, grid (query block, direction, group): kGeoQ queries per lane in registers (independent min chains), the
//            targets staged through LDS in tiles of kGeoTile and read at a wave-uniform address (a broadcast: no bank conflicts).
//            The whole-frame group stores the distances, a class group one sum per query block (double, fixed order)
//   select   one workgroup per (array, quantity): a radix select on the bit patterns (non-negative floats order as their bits)
//            finds the rank the trim or the median needs, one more pass sums what lies below it in double
//   finish   one workgroup adds the class sums in a fixed order and writes the row of BDS_GEOMETRY_METRICS_ROW doubles
// Every launch is sized by the capacity H*W and leaves early on the device's counts.  No floating-point atomics (the histograms of
// the select count with integer LDS atomics, whose result does not depend on their order): bit-identical run to run.
#include "bds_common.h"
#include "geometry_math.h"

namespace bds {

constexpr int kGeoBlock = 256, kGeoBlockWaves = kGeoBlock / kWave;
constexpr int kGeoScanBlock = 1024, kGeoScanWaves = kGeoScanBlock / kWave;
constexpr int kGeoNNThreads = 128, kGeoQ = 4;
constexpr int kGeoQueryBlock = kGeoNNThreads * kGeoQ, kGeoTile = 512;
constexpr int kGeoSelBlock = 1024, kGeoSelWaves = kGeoSelBlock / kWave;
constexpr int kGeoArrays = 3;       // cham_pred, cham_gt, |err|
constexpr int kGeoSlots = 5;        // per array: all of it, the three trims, the lower median
constexpr int kGeoSelVals = 4;      // {sum, sum of squares, k, threshold}
constexpr int64_t kGeoMaxPixels = (int64_t)1 << 24;
static_assert(BDS_GEOMETRY_METRICS_ROW == 32 && BDS_GEOMETRY_QUERY_BLOCK == kGeoQueryBlock && BDS_GEOMETRY_TARGET_TILE == kGeoTile, "include/bds.h");
static_assert(kGeoTile % kGeoNNThreads == 0, "tile staging");

struct GeoFrame {
  int64_t cap;          // H * W
  int W;
  int mode;             // 0: the frame's validity and classes; 1: plain unprojection under m[0] (NULL: every pixel)
  const float *pred, *gt;
  const void *ego, *m[4];
  int kind;             // masks: 0 one byte per pixel, 1 float32; non-zero = true
  const float *K, *c2w;
};

struct GeoWs {
  uint32_t *counts;     // [8] the six totals
  double *sel;          // [kGeoArrays][kGeoSlots][kGeoSelVals]
  uint32_t *blk;        // [kGeoGroups][nblk] counts, then exclusive offsets
  uint8_t *flags;       // [cap]
  float *pts[2];        // [cap,3] pred, gt
  float *err;           // [cap]
  float *dist[2];       // [cap] pred -> gt, gt -> pred
  uint32_t *idx;        // [kGeoClasses][cap]
  double *partial;      // [kGeoClasses][2][nqb]
  int64_t nblk, nqb;
  size_t bytes;
};

static GeoWs geo_ws(void *base, int64_t cap) {
  GeoWs w;
  w.nblk = cdiv(cap, kGeoBlock);
  w.nqb = cdiv(cap, kGeoQueryBlock);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = static_cast<char *>(base) + o;
    o += align_up(bytes, 256);
    return p;
  };
  w.counts = reinterpret_cast<uint32_t *>(take(8 * sizeof(uint32_t)));
  w.sel = reinterpret_cast<double *>(take(kGeoArrays * kGeoSlots * kGeoSelVals * sizeof(double)));
  w.blk = reinterpret_cast<uint32_t *>(take((size_t)kGeoGroups * w.nblk * sizeof(uint32_t)));
  w.flags = reinterpret_cast<uint8_t *>(take((size_t)cap));
  for (int d = 0; d < 2; d++) w.pts[d] = reinterpret_cast<float *>(take((size_t)cap * 3 * sizeof(float)));
  w.err = reinterpret_cast<float *>(take((size_t)cap * sizeof(float)));
  for (int d = 0; d < 2; d++) w.dist[d] = reinterpret_cast<float *>(take((size_t)cap * sizeof(float)));
  w.idx = reinterpret_cast<uint32_t *>(take((size_t)kGeoClasses * cap * sizeof(uint32_t)));
  w.partial = reinterpret_cast<double *>(take((size_t)kGeoClasses * 2 * w.nqb * sizeof(double)));
  w.bytes = o;
  return w;
}

__device__ __forceinline__ bool geo_mask(const void *p, int kind, int64_t pix) {
  if (p == nullptr) return false;
  return kind ? static_cast<const float *>(p)[pix] != 0.0f : static_cast<const uint8_t *>(p)[pix] != 0;
}

__device__ __forceinline__ unsigned geo_pixel_flags(const GeoFrame &f, int64_t pix) {
  if (f.mode == 1) return (f.m[0] == nullptr || geo_mask(f.m[0], f.kind, pix)) ? 1u : 0u;
  const bool valid = geo_valid(f.pred[pix], f.gt[pix], geo_mask(f.ego, f.kind, pix));
  return geo_flags(valid, geo_mask(f.m[0], f.kind, pix), geo_mask(f.m[1], f.kind, pix), geo_mask(f.m[2], f.kind, pix),
                   geo_mask(f.m[3], f.kind, pix));
}

__device__ __forceinline__ unsigned lane_rank(uint64_t ballot) {      // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ __launch_bounds__(kGeoBlock) void geo_flag_kernel(GeoFrame f, int groups, uint8_t *__restrict__ flags, uint32_t *__restrict__ blk,
                                                             int64_t nblk) {
  __shared__ uint32_t s_cnt[kGeoGroups][kGeoBlockWaves];
  const int tid = threadIdx.x;
  const int64_t pix = (int64_t)blockIdx.x * kGeoBlock + tid;
  const unsigned fl = pix < f.cap ? geo_pixel_flags(f, pix) : 0u;
  if (pix < f.cap) flags[pix] = (uint8_t)fl;
#pragma unroll
  for (int g = 0; g < kGeoGroups; g++) {
    const uint64_t b = __ballot((fl >> g) & 1u);
    if ((tid & (kWave - 1)) == 0) s_cnt[g][tid / kWave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (tid < groups) blk[(int64_t)tid * nblk + blockIdx.x] = (s_cnt[tid][0] + s_cnt[tid][1]) + (s_cnt[tid][2] + s_cnt[tid][3]);
}

__global__ __launch_bounds__(kGeoScanBlock) void geo_scan_kernel(int groups, uint32_t *__restrict__ blk, int64_t nblk, uint32_t *__restrict__ counts,
                                                                 int64_t *__restrict__ count_out) {
  __shared__ uint32_t s_w[kGeoScanWaves + 1];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t chunk = (nblk + kGeoScanBlock - 1) / kGeoScanBlock;
  const int64_t lo = (int64_t)tid * chunk < nblk ? (int64_t)tid * chunk : nblk, hi = lo + chunk < nblk ? lo + chunk : nblk;
  for (int g = 0; g < groups; g++) {
    uint32_t *b = blk + (int64_t)g * nblk;
    uint32_t local = 0;
    for (int64_t i = lo; i < hi; i++) local += b[i];
    uint32_t v = local;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t o = __shfl_up(v, off);
      if (lane >= off) v += o;
    }
    if (lane == kWave - 1) s_w[wave] = v;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (int w = 0; w < kGeoScanWaves; w++) {
        const uint32_t c = s_w[w];
        s_w[w] = run;
        run += c;
      }
      s_w[kGeoScanWaves] = run;
    }
    __syncthreads();
    uint32_t run = s_w[wave] + (v - local);
    for (int64_t i = lo; i < hi; i++) {
      const uint32_t c = b[i];
      b[i] = run;
      run += c;
    }
    if (tid == 0) {
      counts[g] = s_w[kGeoScanWaves];
      if (g == 0 && count_out != nullptr) *count_out = (int64_t)s_w[kGeoScanWaves];
    }
    __syncthreads();
  }
}

// points: mode 0 -> pts_pred / pts_gt / err / idx of the workspace; mode 1 -> pts_pred only (the caller's [cap,3] buffer)
__global__ __launch_bounds__(kGeoBlock) void geo_scatter_kernel(GeoFrame f, int groups, const uint8_t *__restrict__ flags,
                                                                const uint32_t *__restrict__ blk, int64_t nblk, float *__restrict__ pts_pred,
                                                                float *__restrict__ pts_gt, float *__restrict__ err, uint32_t *__restrict__ idx) {
  __shared__ uint32_t s_cnt[kGeoGroups][kGeoBlockWaves];
  const int tid = threadIdx.x, wave = tid / kWave;
  const int64_t pix = (int64_t)blockIdx.x * kGeoBlock + tid;
  const unsigned fl = pix < f.cap ? flags[pix] : 0u;
  uint32_t rank[kGeoGroups];
#pragma unroll
  for (int g = 0; g < kGeoGroups; g++) {
    const uint64_t b = __ballot((fl >> g) & 1u);
    rank[g] = lane_rank(b);
    if ((tid & (kWave - 1)) == 0) s_cnt[g][wave] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (!(fl & 1u)) return;
#pragma unroll
  for (int g = 0; g < kGeoGroups; g++) {
    if (g < groups) {
      uint32_t base = blk[(int64_t)g * nblk + blockIdx.x];
      for (int w = 0; w < wave; w++) base += s_cnt[g][w];
      rank[g] += base;
    }
  }
  const int64_t j = rank[0];
  if (j >= f.cap) return;      // (cannot happen: the ranks count pixels)
  const int v = (int)(pix / f.W), u = (int)(pix - (int64_t)v * f.W);
  float p[3];
  const float zp = f.pred[pix];
  geo_unproject(u, v, zp, f.K, f.c2w, p);
#pragma unroll
  for (int k = 0; k < 3; k++) pts_pred[3 * j + k] = p[k];
  if (f.mode == 1) return;
  const float zg = f.gt[pix];
  geo_unproject(u, v, zg, f.K, f.c2w, p);
#pragma unroll
  for (int k = 0; k < 3; k++) pts_gt[3 * j + k] = p[k];
  err[j] = fabsf(zp - zg);
#pragma unroll
  for (int c = 0; c < kGeoClasses; c++) {
    if (((fl >> (c + 1)) & 1u) && rank[c + 1] < f.cap) idx[(int64_t)c * f.cap + rank[c + 1]] = (uint32_t)j;
  }
}

// block sum in double in a fixed order; the result is valid in thread 0
template <int WAVES>
__device__ __forceinline__ double geo_block_sum(double v, double *s_red, int tid) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();      // (s_red may still be read from the previous call)
  if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = v;
  __syncthreads();
  double a = 0.0;
  if (tid == 0) {
    for (int w = 0; w < WAVES; w++) a += s_red[w];
  }
  return a;
}

struct GeoNN {
  const float *pts[2];          // [.,3] x, y
  const uint32_t *counts;       // device counts per group, or NULL: host_n
  int64_t host_n[2];            // points of x, y
  int64_t cap;                  // the launch covers this many queries
  const uint32_t *idx;          // [kGeoClasses][cap] positions of the class groups' points, or NULL (one group)
  float *dist[2];               // group 0: x -> y, y -> x
  double *partial;              // [kGeoClasses][2][nqb], or NULL
  int64_t nqb;
};

template <int NORM>
__global__ __launch_bounds__(kGeoNNThreads) void geo_nn_kernel(GeoNN a) {
  __shared__ float4 s_t[kGeoTile];
  __shared__ double s_red[kGeoNNThreads / kWave];
  const int tid = threadIdx.x, dir = blockIdx.y, g = blockIdx.z;
  int64_t nq, nt;
  if (a.counts != nullptr) {
    const int64_t n = a.counts[g] < a.cap ? (int64_t)a.counts[g] : a.cap;
    nq = nt = n;
  } else {
    nq = a.host_n[dir];
    nt = a.host_n[1 - dir];
  }
  const int64_t q0 = (int64_t)blockIdx.x * kGeoQueryBlock;
  if (q0 >= nq) return;      // (uniform over the workgroup, before any barrier)
  const float *__restrict__ Q = a.pts[dir];
  const float *__restrict__ T = a.pts[1 - dir];
  const uint32_t *__restrict__ ids = g > 0 ? a.idx + (int64_t)(g - 1) * a.cap : nullptr;

  float qx[kGeoQ], qy[kGeoQ], qz[kGeoQ], best[kGeoQ];
#pragma unroll
  for (int j = 0; j < kGeoQ; j++) {
    const int64_t q = q0 + j * kGeoNNThreads + tid;
    const int64_t id = q < nq ? (ids ? (int64_t)ids[q] : q) : -1;
    qx[j] = id >= 0 ? Q[3 * id] : 0.0f;
    qy[j] = id >= 0 ? Q[3 * id + 1] : 0.0f;
    qz[j] = id >= 0 ? Q[3 * id + 2] : 0.0f;
    best[j] = INFINITY;
  }
  for (int64_t t0 = 0; t0 < nt; t0 += kGeoTile) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGeoTile / kGeoNNThreads; j++) {
      const int s = j * kGeoNNThreads + tid;
      const int64_t t = t0 + s;
      const int64_t id = t < nt ? (ids ? (int64_t)ids[t] : t) : -1;
      s_t[s] = id >= 0 ? make_float4(T[3 * id], T[3 * id + 1], T[3 * id + 2], 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int m = nt - t0 < kGeoTile ? (int)(nt - t0) : kGeoTile;
#pragma unroll 4
    for (int k = 0; k < m; k++) {
      const float4 p = s_t[k];
#pragma unroll
      for (int j = 0; j < kGeoQ; j++) best[j] = fminf(best[j], geo_pair<NORM>(qx[j], qy[j], qz[j], p.x, p.y, p.z));
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < kGeoQ; j++) {
    const int64_t q = q0 + j * kGeoNNThreads + tid;
    if (q < nq) {
      if (g == 0) a.dist[dir][q] = best[j];
      sum += (double)best[j];
    }
  }
  if (g > 0 && a.partial != nullptr) {
    const double tot = geo_block_sum<kGeoNNThreads / kWave>(sum, s_red, tid);
    if (tid == 0) a.partial[((int64_t)(g - 1) * 2 + dir) * a.nqb + blockIdx.x] = tot;
  }
}

// sel[array][slot] = {sum, sum of squares, k, threshold} over the k smallest of the array's n values.  slot 0: k = n; 1..3: the trims;
// 4: k = (n - 1) / 2 + 1, whose threshold is the lower median (the |err| array only).  k = 0: k is stored as 0, the rest NaN.
__global__ __launch_bounds__(kGeoSelBlock) void geo_select_kernel(const uint32_t *__restrict__ counts, int64_t cap, const float *__restrict__ a0,
                                                                  const float *__restrict__ a1, const float *__restrict__ a2,
                                                                  double *__restrict__ sel) {
  __shared__ unsigned s_hist[256];
  __shared__ unsigned s_prefix;
  __shared__ unsigned long long s_rank;
  __shared__ double s_red[kGeoSelWaves];
  const int tid = threadIdx.x, arr = blockIdx.x / kGeoSlots, slot = blockIdx.x % kGeoSlots;
  const float *__restrict__ vals = arr == 0 ? a0 : (arr == 1 ? a1 : a2);
  const int64_t n = counts[0] < cap ? (int64_t)counts[0] : cap;
  double *out = sel + (int64_t)blockIdx.x * kGeoSelVals;
  if (slot == 4 && arr != 2) return;
  const int64_t k = slot == 0 ? n : (slot == 4 ? (n > 0 ? (n - 1) / 2 + 1 : 0) : (int64_t)geo_trim_count(n, slot - 1));
  if (k <= 0) {
    if (tid < kGeoSelVals) out[tid] = tid == 2 ? 0.0 : (double)NAN;
    return;
  }
  unsigned thr = 0xffffffffu;      // slot 0: every value lies below
  if (slot != 0) {
    unsigned prefix = 0u, mask = 0u;
    if (tid == 0) s_rank = (unsigned long long)(k - 1);
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) s_hist[tid] = 0u;
      __syncthreads();
      for (int64_t i = tid; i < n; i += kGeoSelBlock) {
        const unsigned b = geo_bits(vals[i]);
        if ((b & mask) == prefix) atomicAdd(&s_hist[(b >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned long long r = s_rank;
        const unsigned d = geo_select_digit(s_hist, &r);
        s_rank = r;
        s_prefix = prefix | (d << shift);
      }
      __syncthreads();
      prefix = s_prefix;
      mask |= 255u << shift;
    }
    thr = prefix;
  }
  double s = 0.0, s2 = 0.0, c = 0.0;
  for (int64_t i = tid; i < n; i += kGeoSelBlock) {
    const float v = vals[i];
    if (geo_bits(v) < thr) {
      s += (double)v;
      s2 += (double)v * (double)v;
      c += 1.0;
    }
  }
  s = geo_block_sum<kGeoSelWaves>(s, s_red, tid);
  s2 = geo_block_sum<kGeoSelWaves>(s2, s_red, tid);
  c = geo_block_sum<kGeoSelWaves>(c, s_red, tid);      // (counts below 2^53: exact)
  if (tid == 0) {
    const float t = slot == 0 ? 0.0f : geo_from_bits(thr);
    geo_trimmed(s, s2, (unsigned long long)c, (unsigned long long)k, t, &out[0], &out[1]);
    out[2] = (double)k;
    out[3] = (double)t;
  }
}

constexpr int kGeoFinBlock = 2 * kGeoClasses * kWave;      // one wave per (class, direction)

__global__ __launch_bounds__(kGeoFinBlock) void geo_finish_kernel(const uint32_t *__restrict__ counts, int64_t cap, const double *__restrict__ sel,
                                                                  const double *__restrict__ partial, int64_t nqb, double *__restrict__ row) {
  __shared__ double s_cls[2 * kGeoClasses];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave, c = w / 2;
  const int64_t nc = counts[c + 1] < cap ? (int64_t)counts[c + 1] : cap;
  const int64_t blocks = (nc + kGeoQueryBlock - 1) / kGeoQueryBlock;
  double acc = 0.0;
  for (int64_t b = lane; b < blocks; b += kWave) acc += partial[(int64_t)w * nqb + b];
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) s_cls[w] = acc;
  __syncthreads();
  if (tid != 0) return;
  const double nan = (double)NAN;
  const int64_t n = counts[0] < cap ? (int64_t)counts[0] : cap;
  auto S = [&](int arr, int slot, int v) { return sel[((int64_t)arr * kGeoSlots + slot) * kGeoSelVals + v]; };
  for (int s = 0; s < 1 + kGeoTrims; s++) {
    const double k = S(0, s, 2);
    const double mp = k > 0.0 ? S(0, s, 0) / k : nan, mg = k > 0.0 ? S(1, s, 0) / k : nan, me = k > 0.0 ? S(2, s, 0) / k : nan;
    row[s] = mp + mg;
    row[4 + s] = k > 0.0 ? sqrt(S(2, s, 1) / k) : nan;
    row[20 + s] = mp;
    row[24 + s] = mg;
    row[28 + s] = me;
  }
  const double med = S(2, 4, 3);
  row[8] = n > 0 ? med * med : nan;
  row[14] = (double)n;
  for (int q = 0; q < kGeoClasses; q++) {
    const int64_t m = counts[q + 1] < cap ? (int64_t)counts[q + 1] : cap;
    row[9 + q] = m > 0 ? s_cls[2 * q] / (double)m + s_cls[2 * q + 1] / (double)m : nan;
    row[15 + q] = (double)m;
  }
}

static bool geo_extent_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W <= kGeoMaxPixels; }
static bool al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace bds

using namespace bds;

extern "C" size_t bds_geometry_metrics_workspace_bytes(int H, int W) {
  if (!geo_extent_ok(H, W)) return 0;
  return geo_ws(nullptr, (int64_t)H * W).bytes;
}

extern "C" int bds_geometry_metrics(int H, int W, const float *pred, const float *gt, const void *egocar, const void *mask0, const void *mask1,
                                    const void *mask2, const void *mask3, int mask_kind, const float *K, const float *c2w, double *row_out,
                                    float *dist_pred, float *dist_gt, void *ws, size_t ws_bytes, bds_stream_t stream) {
  BDS_REQUIRE(geo_extent_ok(H, W));
  BDS_REQUIRE(pred && gt && K && c2w && row_out && al4(pred) && al4(gt) && al4(K) && al4(c2w));
  BDS_REQUIRE((reinterpret_cast<uintptr_t>(row_out) & 7u) == 0);
  BDS_REQUIRE(mask_kind == 0 || mask_kind == 1);
  BDS_REQUIRE((dist_pred == nullptr) == (dist_gt == nullptr) && al4(dist_pred) && al4(dist_gt));
  const void *masks[5] = {egocar, mask0, mask1, mask2, mask3};
  for (int s = 0; s < 5; s++) BDS_REQUIRE(mask_kind == 0 || al4(masks[s]));
  BDS_REQUIRE(ws && aligned16(ws));
  if (ws_bytes < bds_geometry_metrics_workspace_bytes(H, W)) return BDS_EWORKSPACE;
  const int64_t cap = (int64_t)H * W;
  GeoWs w = geo_ws(ws, cap);
  GeoFrame f;
  f.cap = cap;
  f.W = W;
  f.mode = 0;
  f.pred = pred;
  f.gt = gt;
  f.ego = egocar;
  for (int s = 0; s < 4; s++) f.m[s] = masks[1 + s];
  f.kind = mask_kind;
  f.K = K;
  f.c2w = c2w;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(geo_flag_kernel, dim3((unsigned)w.nblk), dim3(kGeoBlock), 0, st, f, kGeoGroups, w.flags, w.blk, w.nblk);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_scan_kernel, dim3(1), dim3(kGeoScanBlock), 0, st, kGeoGroups, w.blk, w.nblk, w.counts, (int64_t *)nullptr);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_scatter_kernel, dim3((unsigned)w.nblk), dim3(kGeoBlock), 0, st, f, kGeoGroups, w.flags, w.blk, w.nblk, w.pts[0],
                     w.pts[1], w.err, w.idx);
  BDS_LAUNCH_CHECK();
  GeoNN a;
  a.pts[0] = w.pts[0];
  a.pts[1] = w.pts[1];
  a.counts = w.counts;
  a.host_n[0] = a.host_n[1] = 0;
  a.cap = cap;
  a.idx = w.idx;
  a.dist[0] = dist_pred ? dist_pred : w.dist[0];
  a.dist[1] = dist_gt ? dist_gt : w.dist[1];
  a.partial = w.partial;
  a.nqb = w.nqb;
  hipLaunchKernelGGL(geo_nn_kernel<2>, dim3((unsigned)w.nqb, 2, kGeoGroups), dim3(kGeoNNThreads), 0, st, a);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_select_kernel, dim3(kGeoArrays * kGeoSlots), dim3(kGeoSelBlock), 0, st, w.counts, cap, a.dist[0], a.dist[1], w.err,
                     w.sel);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_finish_kernel, dim3(1), dim3(kGeoFinBlock), 0, st, w.counts, cap, w.sel, w.partial, w.nqb, row_out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_depth_unproject(int H, int W, const float *depth, const void *mask, int mask_kind, const float *K, const float *c2w,
                                   float *points, int64_t *count, void *ws, size_t ws_bytes, bds_stream_t stream) {
  BDS_REQUIRE(geo_extent_ok(H, W));
  BDS_REQUIRE(depth && K && c2w && points && count && al4(depth) && al4(K) && al4(c2w) && al4(points));
  BDS_REQUIRE((reinterpret_cast<uintptr_t>(count) & 7u) == 0);
  BDS_REQUIRE((mask_kind == 0 || mask_kind == 1) && (mask_kind == 0 || al4(mask)));
  BDS_REQUIRE(ws && aligned16(ws));
  if (ws_bytes < bds_geometry_metrics_workspace_bytes(H, W)) return BDS_EWORKSPACE;
  const int64_t cap = (int64_t)H * W;
  GeoWs w = geo_ws(ws, cap);
  GeoFrame f;
  f.cap = cap;
  f.W = W;
  f.mode = 1;
  f.pred = depth;
  f.gt = nullptr;
  f.ego = nullptr;
  f.m[0] = mask;
  f.m[1] = f.m[2] = f.m[3] = nullptr;
  f.kind = mask_kind;
  f.K = K;
  f.c2w = c2w;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(geo_flag_kernel, dim3((unsigned)w.nblk), dim3(kGeoBlock), 0, st, f, 1, w.flags, w.blk, w.nblk);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_scan_kernel, dim3(1), dim3(kGeoScanBlock), 0, st, 1, w.blk, w.nblk, w.counts, count);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(geo_scatter_kernel, dim3((unsigned)w.nblk), dim3(kGeoBlock), 0, st, f, 1, w.flags, w.blk, w.nblk, points, (float *)nullptr,
                     (float *)nullptr, (uint32_t *)nullptr);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_chamfer_nn(int64_t P1, int64_t P2, const float *x, const float *y, int norm, float *dist_x, float *dist_y,
                              bds_stream_t stream) {
  BDS_REQUIRE(P1 >= 0 && P2 >= 0 && P1 <= INT32_MAX && P2 <= INT32_MAX && (norm == 1 || norm == 2));
  BDS_REQUIRE((P1 == 0 || (x && dist_x)) && (P2 == 0 || (y && dist_y)));
  BDS_REQUIRE(al4(x) && al4(y) && al4(dist_x) && al4(dist_y));
  const int64_t cap = P1 > P2 ? P1 : P2;
  if (cap == 0) return BDS_OK;
  GeoNN a;
  a.pts[0] = x;
  a.pts[1] = y;
  a.counts = nullptr;
  a.host_n[0] = P1;
  a.host_n[1] = P2;
  a.cap = cap;
  a.idx = nullptr;
  a.dist[0] = dist_x;
  a.dist[1] = dist_y;
  a.partial = nullptr;
  a.nqb = cdiv(cap, kGeoQueryBlock);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)a.nqb, 2, 1);
  if (norm == 1)
    hipLaunchKernelGGL(geo_nn_kernel<1>, grid, dim3(kGeoNNThreads), 0, st, a);
  else
    hipLaunchKernelGGL(geo_nn_kernel<2>, grid, dim3(kGeoNNThreads), 0, st, a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
