// Exact K-nearest self-search of a point cloud, K = 1..8, and the initial log-scales of a scene's Gaussians from it: what
// k_nearest_sklearn (models/gaussians/basics.py:208-224) gives create_from_pcd (vanilla.py:79-105) and the rigid nodes' initialiser
// (nodes/rigid.py:113-120) from a kd-tree on the host.  The per-element math lives in knn_math.h.
//   clear     zero the per-cell counts (capacity 2 N + 2) and the histograms, and set the stats block
//   bounds    min / max of the cloud: per-workgroup reduction, then integer atomics on an order-preserving encoding (min and max do
//             not depend on the order)
//   hist      (twice) per axis a 1024-bin histogram of the coordinates, over the cloud's box and then over the first trim's result:
//             per-workgroup in LDS, integer atomics outwards
//   trim      (twice) drops from either end of every axis the bins that hold at most N / 128 points together; the second time one
//             lane also picks the cell edge and the dimensions from the trimmed box and N (at most max(1, 2 N) cells, so the
//             workspace and the launches depend on N alone) and writes them into the stats block
//   count     per point its cell; an integer atomic on the cell's count, whose return value is the point's rank inside the cell
//   scan      one workgroup turns the counts into exclusive offsets (scan.h)
//   scatter   each point as one 16-byte record {x, y, z, original index} to offset[cell] + rank
//   query     one lane per record IN CELL ORDER: rings r = 0..BDS_KNN_RING_MAX of cells around the query's, the K best (d2, index)
//             in registers, the termination test after every ring; a resolved query writes its rows, another appends itself to
//             the unresolved list
//   fallback  exact brute force for the listed queries: BDS_KNN_QUERY_BLOCK per workgroup against LDS tiles of BDS_KNN_TARGET_TILE
//             records read at a wave-uniform address (a broadcast, as geo_nn_kernel); launched at capacity N, leaves on the count
// Order: the atomics place a cell's points in an order that changes from run to run, and the unresolved list likewise.  Neither
// reaches the result: a query's K best under the (d2, index) order are a function of the SET of candidates (knn_math.h), every query
// writes only its own rows, and no floating-point value is accumulated across lanes.  Bit-identical run to run, and invariant under
// a permutation of the rows up to that permutation (the indices then differ where distances tie).
//
// Why records of 16 bytes: a candidate is one global_load_dwordx4 (the index travels with the coordinates: no second gather through
// a permutation), a wave's 64 queries are 1 KiB of consecutive records, and the fallback stages a record with one 16-byte LDS write
// and reads it back with one ds_read_b128.
// Bytes per point: 12 read by bounds, 12 by each histogram pass, 12 by count (+4 rank), 12 + 4 read and 16 written by scatter, 16
// read by query plus its candidates -- about 27 cells' records at ring 1, most of them shared with the neighbouring lanes and served by L1 / L2 -- and
// 4 K (distances) + 4 K (indices) + 4 S written: about 100 bytes of compulsory traffic per point at K = 3.  The cell offsets add
// 8 bytes per point (2 N cells at most) through the scan.
// Occupancy: the query kernel holds 2 K registers of list, the query and loop state -- 66 VGPRs at K = 3 (7 waves / SIMD), 92 at
// K = 8 (5 waves); no LDS.  The fallback holds two queries per lane (4 K registers of lists) and 8 KiB of LDS per
// 128-thread workgroup, so LDS never limits it.  No kernel uses scratch: the lists are indexed statically in unrolled loops.
// BDS_KNN_RING_MAX = 2: at the grid's density (one cell per point of the box, at least half a point per cell) a volume-filling
// cloud leaves a query unresolved after ring 2 only when fewer than K points lie within two edges of it (a Poisson tail below 1e-4
// at K = 3), and on surfaces (lidar) the cells that hold points hold many, so ring 0 or 1 resolves.  What is left are points in
// regions far sparser than the average -- lidar outliers -- whose neighbours lie tens of edges away: a ring walk grows with r^3 empty
// cells per lane and stalls the other 63 lanes of its wave meanwhile, the fallback runs them with every lane busy.
#include "bds_common.h"
#include "knn_math.h"
#include "scan.h"

namespace bds {

constexpr int kKnnBlock = 256, kKnnBlockWaves = kKnnBlock / kWave;
constexpr int kKnnScanBlock = 1024;
constexpr int kKnnFbThreads = 128, kKnnFbQ = 2;
constexpr int kKnnQueryBlock = kKnnFbThreads * kKnnFbQ, kKnnTile = 512;
constexpr int kKnnRingMax = 2;
constexpr int kKnnBoundsGrid = 1024;
constexpr int64_t kKnnMaxPoints = (int64_t)1 << 30;
// the stats block (include/bds.h): 32-bit words
constexpr int kStEdge = 0, kStInv = 1, kStSlack = 2, kStDim = 3, kStUnresolved = 6, kStLo = 7, kStHi = 10, kStCells = 13;
constexpr int kStCloudLo = 14, kStCloudHi = 17;
constexpr int kKnnHistWords = 3 * kKnnBins;
static_assert(BDS_KNN_QUERY_BLOCK == kKnnQueryBlock && BDS_KNN_TARGET_TILE == kKnnTile && BDS_KNN_RING_MAX == kKnnRingMax &&
                  BDS_KNN_STATS_WORDS == kKnnStatsWords && BDS_KNN_MAX_K == kKnnMaxK && BDS_KNN_MAX_POINTS == kKnnMaxPoints,
              "include/bds.h");
static_assert(BDS_KNN_STAT_EDGE == kStEdge && BDS_KNN_STAT_DIMS == kStDim && BDS_KNN_STAT_UNRESOLVED == kStUnresolved &&
                  BDS_KNN_STAT_LO == kStLo && BDS_KNN_STAT_HI == kStHi && BDS_KNN_STAT_CELLS == kStCells &&
                  BDS_KNN_STAT_CLOUD_LO == kStCloudLo && BDS_KNN_STAT_CLOUD_HI == kStCloudHi,
              "include/bds.h");
static_assert(kKnnTile % kKnnFbThreads == 0, "tile staging");

struct KnnWs {
  uint32_t *stats;      // [kKnnStatsWords]
  uint32_t *hist;       // [2][3][kKnnBins] the two trimming passes' histograms
  uint32_t *cells;      // [2 N + 2] counts, then exclusive offsets (offset[cells] = N)
  uint32_t *rank;       // [N] rank inside the cell; after the scatter, the unresolved list (positions in cell order)
  float4 *rec;          // [N] {x, y, z, original index} in cell order
  int64_t cell_cap;
  size_t bytes;
};

static KnnWs knn_ws(void *base, int64_t N) {
  KnnWs w;
  w.cell_cap = 2 * N + 2;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char *p = static_cast<char *>(base) + o;
    o += align_up(bytes, 256);
    return p;
  };
  w.stats = reinterpret_cast<uint32_t *>(take(kKnnStatsWords * sizeof(uint32_t)));
  w.hist = reinterpret_cast<uint32_t *>(take(2 * kKnnHistWords * sizeof(uint32_t)));
  w.cells = reinterpret_cast<uint32_t *>(take((size_t)w.cell_cap * sizeof(uint32_t)));
  w.rank = reinterpret_cast<uint32_t *>(take((size_t)N * sizeof(uint32_t)));
  w.rec = reinterpret_cast<float4 *>(take((size_t)N * sizeof(float4)));
  w.bytes = o;
  return w;
}

struct KnnArgs {
  int64_t N;
  const float *x;
  float *dist;
  int32_t *idx;
  float *log_scales;
  int S;
  float clamp_lo, clamp_hi;
  uint32_t *stats, *cells, *rank;
  float4 *rec;
};

__device__ __forceinline__ KnnGrid knn_load_grid(const uint32_t *__restrict__ st) {
  KnnGrid g;
  g.edge = __uint_as_float(st[kStEdge]);
  g.inv = __uint_as_float(st[kStInv]);
  g.slack = __uint_as_float(st[kStSlack]);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    g.dim[a] = (int)st[kStDim + a];
    g.lo[a] = __uint_as_float(st[kStLo + a]);
  }
  return g;
}

__global__ __launch_bounds__(kKnnBlock) void knn_clear_kernel(uint32_t *__restrict__ stats, uint32_t *__restrict__ hist, uint32_t *__restrict__ cells,
                                                             int64_t cell_cap) {
  const int64_t stride = (int64_t)gridDim.x * kKnnBlock, first = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
  for (int64_t i = first; i < cell_cap; i += stride) cells[i] = 0u;
  for (int64_t i = first; i < 2 * kKnnHistWords; i += stride) hist[i] = 0u;
  if (blockIdx.x == 0 && threadIdx.x < kKnnStatsWords) {
    const int t = threadIdx.x;
    stats[t] = (t >= kStCloudLo && t < kStCloudLo + 3) ? 0xffffffffu : 0u;      // the minima start at the top of the ordered encoding
  }
}

__global__ __launch_bounds__(kKnnBlock) void knn_bounds_kernel(int64_t N, const float *__restrict__ x, uint32_t *__restrict__ stats) {
  __shared__ float s_lo[3][kKnnBlockWaves], s_hi[3][kKnnBlockWaves];
  const int tid = threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int64_t stride = (int64_t)gridDim.x * kKnnBlock;
  for (int64_t i = (int64_t)blockIdx.x * kKnnBlock + tid; i < N; i += stride) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = x[3 * i + a];
      lo[a] = fminf(lo[a], v);
      hi[a] = fmaxf(hi[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
    }
    if ((tid & (kWave - 1)) == 0) {
      s_lo[a][tid / kWave] = lo[a];
      s_hi[a][tid / kWave] = hi[a];
    }
  }
  __syncthreads();
  if (tid < 3) {
    float l = s_lo[tid][0], h = s_hi[tid][0];
    for (int w = 1; w < kKnnBlockWaves; w++) {
      l = fminf(l, s_lo[tid][w]);
      h = fmaxf(h, s_hi[tid][w]);
    }
    if (l <= h) {      // (a workgroup past the end of a short cloud holds no point)
      atomicMin(&stats[kStCloudLo + tid], knn_ordered(l));
      atomicMax(&stats[kStCloudHi + tid], knn_ordered(h));
    }
  }
}

// pass 0: over the cloud's box (still in the ordered encoding); pass 1: over the first trim's box
__global__ __launch_bounds__(kKnnBlock) void knn_hist_kernel(int64_t N, const float *__restrict__ x, const uint32_t *__restrict__ stats, int pass,
                                                            uint32_t *__restrict__ hist) {
  __shared__ uint32_t s_h[kKnnHistWords];
  const int tid = threadIdx.x;
  for (int i = tid; i < kKnnHistWords; i += kKnnBlock) s_h[i] = 0u;
  float lo[3], scale[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = pass == 0 ? knn_from_ordered(stats[kStCloudLo + a]) : __uint_as_float(stats[kStLo + a]);
    const float hi = pass == 0 ? knn_from_ordered(stats[kStCloudHi + a]) : __uint_as_float(stats[kStHi + a]);
    scale[a] = knn_bin_scale(lo[a], hi);
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kKnnBlock;
  for (int64_t i = (int64_t)blockIdx.x * kKnnBlock + tid; i < N; i += stride) {
#pragma unroll
    for (int a = 0; a < 3; a++) atomicAdd(&s_h[a * kKnnBins + knn_bin(x[3 * i + a], lo[a], scale[a])], 1u);      // (bin < kKnnBins: clamped)
  }
  __syncthreads();
  for (int i = tid; i < kKnnHistWords; i += kKnnBlock)
    if (s_h[i] != 0u) atomicAdd(&hist[i], s_h[i]);
}

// pass 0: cloud box -> first trim (and the cloud's box decoded in place); pass 1: first trim -> the grid's box, then the grid
__global__ __launch_bounds__(kWave) void knn_trim_kernel(int64_t N, uint32_t *__restrict__ stats, int pass, const uint32_t *__restrict__ hist) {
  __shared__ float s_lo[3], s_hi[3];
  const int tid = threadIdx.x;
  if (tid < 3) {
    float lo, hi;
    if (pass == 0) {
      lo = knn_from_ordered(stats[kStCloudLo + tid]);
      hi = knn_from_ordered(stats[kStCloudHi + tid]);
      stats[kStCloudLo + tid] = __float_as_uint(lo);
      stats[kStCloudHi + tid] = __float_as_uint(hi);
    } else {
      lo = __uint_as_float(stats[kStLo + tid]);
      hi = __uint_as_float(stats[kStHi + tid]);
    }
    knn_trim_axis(hist + tid * kKnnBins, (long long)N, lo, hi, &s_lo[tid], &s_hi[tid]);
    stats[kStLo + tid] = __float_as_uint(s_lo[tid]);
    stats[kStHi + tid] = __float_as_uint(s_hi[tid]);
  }
  __syncthreads();
  if (pass == 0 || tid != 0) return;
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    lo[a] = s_lo[a];
    hi[a] = s_hi[a];
  }
  KnnGrid g;
  knn_choose_grid(lo, hi, (long long)N, &g);
  stats[kStEdge] = __float_as_uint(g.edge);
  stats[kStInv] = __float_as_uint(g.inv);
  stats[kStSlack] = __float_as_uint(g.slack);
  for (int a = 0; a < 3; a++) stats[kStDim + a] = (uint32_t)g.dim[a];
  stats[kStCells] = (uint32_t)((int64_t)g.dim[0] * g.dim[1] * g.dim[2]);
}

__global__ __launch_bounds__(kKnnBlock) void knn_count_kernel(KnnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
  if (i >= a.N) return;
  const KnnGrid g = knn_load_grid(a.stats);
  int c[3];
  knn_cell(g, a.x[3 * i], a.x[3 * i + 1], a.x[3 * i + 2], c);
  const int64_t cell = knn_cell_id(g, c);      // < dim0 dim1 dim2 <= 2 N: inside the counts
  a.rank[i] = atomicAdd(&a.cells[cell], 1u);
}

// counts[0 .. n) -> exclusive offsets, n = cells + 1 (the last count is 0, so offsets[cells] = N)
__global__ __launch_bounds__(kKnnScanBlock) void knn_scan_kernel(uint32_t *__restrict__ b, const uint32_t *__restrict__ stats, int64_t cell_cap) {
  __shared__ uint32_t lw[kKnnScanBlock / kWave];
  const int64_t n = (int64_t)stats[kStCells] + 1;
  uint32_t total;
  workgroup_scan_in_place<kKnnScanBlock>(b, n < cell_cap ? n : cell_cap, &total, lw);
}

__global__ __launch_bounds__(kKnnBlock) void knn_scatter_kernel(KnnArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
  if (i >= a.N) return;
  const KnnGrid g = knn_load_grid(a.stats);
  const float px = a.x[3 * i], py = a.x[3 * i + 1], pz = a.x[3 * i + 2];
  int c[3];
  knn_cell(g, px, py, pz, c);
  const int64_t j = (int64_t)a.cells[knn_cell_id(g, c)] + a.rank[i];
  if (j < a.N) a.rec[j] = make_float4(px, py, pz, __int_as_float((int)i));      // (always: the offsets count the points)
}

template <int K>
__device__ __forceinline__ void knn_write(const KnnArgs &a, int64_t self, const KnnBest<K> &b) {
  float d[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    d[k] = sqrtf(b.d[k]);
    a.dist[self * K + k] = d[k];
  }
  if (a.idx != nullptr) {
#pragma unroll
    for (int k = 0; k < K; k++) a.idx[self * K + k] = b.i[k];
  }
  if (a.log_scales != nullptr) {
    const float s = knn_log_scale<K>(d, a.clamp_lo, a.clamp_hi);
#pragma unroll
    for (int k = 0; k < 3; k++)
      if (k < a.S) a.log_scales[self * a.S + k] = s;
  }
}

template <int K>
__device__ __forceinline__ void knn_scan_range(const float4 *__restrict__ rec, uint32_t s, uint32_t e, const float4 &q, int self, KnnBest<K> &b) {
  for (uint32_t t = s; t < e; t++) {
    const float4 p = rec[t];
    const int pi = __float_as_int(p.w);
    if (pi != self) knn_insert<K>(b, knn_pair(q.x, q.y, q.z, p.x, p.y, p.z), pi);
  }
}

// Every loop below runs over at most 2 kKnnRingMax + 1 cells per axis, clipped to the grid, and over a cell range's records, which
// the offsets bound by N: the kernel ends whatever the input.
template <int K>
__global__ __launch_bounds__(kKnnBlock) void knn_query_kernel(KnnArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kKnnBlock + threadIdx.x;
  if (j >= a.N) return;
  const KnnGrid g = knn_load_grid(a.stats);
  const float4 q = a.rec[j];
  const int self = __float_as_int(q.w);
  int c[3];
  knn_cell(g, q.x, q.y, q.z, c);
  const float ql[3] = {q.x - g.lo[0], q.y - g.lo[1], q.z - g.lo[2]};
  const uint32_t *__restrict__ off = a.cells;
  const uint32_t n32 = (uint32_t)a.N;
  KnnBest<K> b;
  knn_clear<K>(b);
  bool done = false;
  for (int r = 0; r <= kKnnRingMax && !done; r++) {
    const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < g.dim[2] - 1 ? c[2] + r : g.dim[2] - 1;
    const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < g.dim[1] - 1 ? c[1] + r : g.dim[1] - 1;
    const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < g.dim[0] - 1 ? c[0] + r : g.dim[0] - 1;
    for (int z = z0; z <= z1; z++) {
      for (int y = y0; y <= y1; y++) {
        const int64_t row = ((int64_t)z * g.dim[1] + y) * g.dim[0];
        const bool shell = z - c[2] == r || c[2] - z == r || y - c[1] == r || c[1] - y == r;
        if (shell) {      // the whole row of the cube: its cells are consecutive, so are their records
          const uint32_t s = off[row + x0], e = off[row + x1 + 1];
          knn_scan_range<K>(a.rec, s, e < n32 ? e : n32, q, self, b);
        } else {          // (r > 0) only the row's two end cells belong to this ring
          if (c[0] - r >= 0) {
            const uint32_t s = off[row + c[0] - r], e = off[row + c[0] - r + 1];
            knn_scan_range<K>(a.rec, s, e < n32 ? e : n32, q, self, b);
          }
          if (c[0] + r <= g.dim[0] - 1) {
            const uint32_t s = off[row + c[0] + r], e = off[row + c[0] + r + 1];
            knn_scan_range<K>(a.rec, s, e < n32 ? e : n32, q, self, b);
          }
        }
      }
    }
    done = knn_resolved(b.d[K - 1], knn_ring_margin2(g, ql, c, r));
  }
  if (done) {
    knn_write<K>(a, (int64_t)self, b);
  } else {
    const uint32_t slot = atomicAdd(&a.stats[kStUnresolved], 1u);
    if (slot < n32) a.rank[slot] = (uint32_t)j;      // (always: at most N queries arrive)
  }
}

template <int K>
__global__ __launch_bounds__(kKnnFbThreads) void knn_fallback_kernel(KnnArgs a) {
  __shared__ float4 s_t[kKnnTile];
  const int tid = threadIdx.x;
  const int64_t count = a.stats[kStUnresolved] < a.N ? (int64_t)a.stats[kStUnresolved] : a.N;
  const int64_t q0 = (int64_t)blockIdx.x * kKnnQueryBlock;
  if (q0 >= count) return;      // (uniform over the workgroup, before any barrier)
  float4 q[kKnnFbQ];
  int self[kKnnFbQ];
  KnnBest<K> b[kKnnFbQ];
#pragma unroll
  for (int j = 0; j < kKnnFbQ; j++) {
    const int64_t u = q0 + j * kKnnFbThreads + tid;
    int64_t pos = u < count ? (int64_t)a.rank[u] : 0;
    pos = pos < a.N ? pos : 0;
    q[j] = a.rec[pos];
    self[j] = u < count ? __float_as_int(q[j].w) : -1;
    knn_clear<K>(b[j]);
  }
  for (int64_t t0 = 0; t0 < a.N; t0 += kKnnTile) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kKnnTile / kKnnFbThreads; j++) {
      const int s = j * kKnnFbThreads + tid;
      const int64_t t = t0 + s;
      s_t[s] = t < a.N ? a.rec[t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const int m = a.N - t0 < kKnnTile ? (int)(a.N - t0) : kKnnTile;
#pragma unroll 2
    for (int k = 0; k < m; k++) {
      const float4 p = s_t[k];
      const int pi = __float_as_int(p.w);
#pragma unroll
      for (int j = 0; j < kKnnFbQ; j++)
        if (pi != self[j]) knn_insert<K>(b[j], knn_pair(q[j].x, q[j].y, q[j].z, p.x, p.y, p.z), pi);
    }
  }
#pragma unroll
  for (int j = 0; j < kKnnFbQ; j++)
    if (self[j] >= 0) knn_write<K>(a, (int64_t)self[j], b[j]);
}

template <int K>
static int knn_launch_search(const KnnArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(knn_query_kernel<K>, dim3((unsigned)cdiv(a.N, kKnnBlock)), dim3(kKnnBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_fallback_kernel<K>, dim3((unsigned)cdiv(a.N, kKnnQueryBlock)), dim3(kKnnFbThreads), 0, st, a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

static bool knn_al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace bds

using namespace bds;

extern "C" size_t bds_knn_workspace_bytes(int64_t N) {
  if (N < 2 || N > kKnnMaxPoints) return 0;
  return knn_ws(nullptr, N).bytes;
}

extern "C" int bds_knn_self(int64_t N, const float *x, int K, float *dist, int32_t *idx, float *log_scales, int S, float clamp_lo,
                            float clamp_hi, void *ws, size_t ws_bytes, bds_stream_t stream) {
  BDS_REQUIRE(K >= 1 && K <= kKnnMaxK);
  BDS_REQUIRE(N >= (int64_t)K + 1 && N <= kKnnMaxPoints);
  BDS_REQUIRE(x && dist && ws);
  BDS_REQUIRE(knn_al4(x) && knn_al4(dist) && knn_al4(idx) && knn_al4(log_scales) && aligned16(ws));
  if (log_scales != nullptr) {
    BDS_REQUIRE(S >= 1 && S <= 3);
    BDS_REQUIRE(clamp_lo <= clamp_hi);      // (false for a NaN on either side)
  }
  if (ws_bytes < bds_knn_workspace_bytes(N)) return BDS_EWORKSPACE;
  const KnnWs w = knn_ws(ws, N);
  KnnArgs a;
  a.N = N;
  a.x = x;
  a.dist = dist;
  a.idx = idx;
  a.log_scales = log_scales;
  a.S = S;
  a.clamp_lo = clamp_lo;
  a.clamp_hi = clamp_hi;
  a.stats = w.stats;
  a.cells = w.cells;
  a.rank = w.rank;
  a.rec = w.rec;
  hipStream_t st = as_stream(stream);
  const unsigned nblk = (unsigned)cdiv(N, kKnnBlock);
  const unsigned clear_grid = (unsigned)(cdiv(w.cell_cap, kKnnBlock) < 2048 ? cdiv(w.cell_cap, kKnnBlock) : 2048);
  hipLaunchKernelGGL(knn_clear_kernel, dim3(clear_grid), dim3(kKnnBlock), 0, st, w.stats, w.hist, w.cells, w.cell_cap);
  BDS_LAUNCH_CHECK();
  const unsigned pass_grid = nblk < (unsigned)kKnnBoundsGrid ? nblk : (unsigned)kKnnBoundsGrid;
  hipLaunchKernelGGL(knn_bounds_kernel, dim3(pass_grid), dim3(kKnnBlock), 0, st, N, x, w.stats);
  BDS_LAUNCH_CHECK();
  for (int pass = 0; pass < 2; pass++) {
    hipLaunchKernelGGL(knn_hist_kernel, dim3(pass_grid), dim3(kKnnBlock), 0, st, N, x, w.stats, pass, w.hist + pass * kKnnHistWords);
    BDS_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_trim_kernel, dim3(1), dim3(kWave), 0, st, N, w.stats, pass, w.hist + pass * kKnnHistWords);
    BDS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(knn_count_kernel, dim3(nblk), dim3(kKnnBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_scan_kernel, dim3(1), dim3(kKnnScanBlock), 0, st, w.cells, w.stats, w.cell_cap);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(knn_scatter_kernel, dim3(nblk), dim3(kKnnBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  switch (K) {
    case 1: return knn_launch_search<1>(a, st);
    case 2: return knn_launch_search<2>(a, st);
    case 3: return knn_launch_search<3>(a, st);
    case 4: return knn_launch_search<4>(a, st);
    case 5: return knn_launch_search<5>(a, st);
    case 6: return knn_launch_search<6>(a, st);
    case 7: return knn_launch_search<7>(a, st);
    default: return knn_launch_search<8>(a, st);
  }
}
