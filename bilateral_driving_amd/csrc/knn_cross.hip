// Exact K nearest rows of one cloud for every row of another, batched, K = 1..32: pytorch3d's knn_points as the reference calls it
// (models/modules.py:1199 VoxelDeformer._query_weights_smpl, K = 30 of the template's vertices for every voxel centre;
// models/nodes/smpl.py:186 update_knn, a batch of clouds against themselves at K = 3; utils/chamfer_distance.py:45-46, K = 1), and
// the inverse-distance blend of per-row features that modules.py:1200-1206 forms from the result.  The per-element math lives in
// knn_math.h.  One launch, no workspace, no host wait.
//   search    one query per lane, BDS_KNN_CROSS_QUERY_BLOCK queries of ONE cloud per workgroup; the cloud's candidates pass through
//             LDS in tiles of BDS_KNN_CROSS_TARGET_TILE records {x, y, z, row bits}, and every lane reads the same record at the same
//             time (one ds_read_b128 at a wave-uniform address: a broadcast, no bank conflicts).  The K best (value, row) stay in
//             registers as KnnBest<Kc>, Kc the capacity 4, 8, 16 or 32 that holds K: a list longer than asked is exact in its first K
//   order     knn_insert_shift tests the newcomer against the list's last entry first; only an accepted one walks the list, entry by
//             entry without a branch (three compares, two mask operations and four selects each), in place.  Consecutive lanes are
//             neighbouring queries (the voxel grid lays x fastest), so a wave mostly accepts together
//   lengths   only rows below len2[b] are staged or compared (a tile's tail is never read); rows of p1 at or beyond len1[b], and the
//             slots beyond len2[b], are written as zeros: every element of every output is written
//   blend     w_k = 1 / clamp(sqrt(d2_k)), normalised by their sum, times the neighbours' feature rows, k ascending, per lane; the
//             features come through buffer loads, one register of byte offset per slot
// Order: a query's list is a function of the SET of candidates under the total (value, row) order, every lane writes only its own rows
// and nothing is accumulated across lanes: bit-identical run to run, and a permutation of p1 permutes the rows of the result.
// Bounds: a lane reads p1 only for q < P1, stages p2 only for rows < min(len2[b], P2), gathers features only at rows a candidate
// brought (so < len2[b]), and writes only the rows q < P1 of cloud b < B.
// Registers: the list is 2 Kc VGPRs, indexed statically in unrolled loops, so nothing goes to scratch; the blend keeps its weights
// and offsets in the list's own registers.  Kc = 32: 87 VGPRs (88 allocated), 5 waves per SIMD; Kc <= 16: 8 waves.  LDS: 8 KiB per
// workgroup.
#include "bds_common.h"
#include "knn_math.h"

namespace bds {

constexpr int kKxBlock = 256, kKxTile = 512;
constexpr int kKxMaxK = 32, kKxMaxJ = 64;
static_assert(BDS_KNN_CROSS_QUERY_BLOCK == kKxBlock && BDS_KNN_CROSS_TARGET_TILE == kKxTile && BDS_KNN_CROSS_MAX_K == kKxMaxK &&
                  BDS_KNN_CROSS_MAX_J == kKxMaxJ,
              "include/bds.h");
static_assert(kKxTile % kKxBlock == 0, "tile staging");

struct KnnCrossArgs {
  int K, J, blocks_per_cloud;
  int64_t P1, P2;
  const float *p1, *p2, *feat;
  const int64_t *len1, *len2;
  float *dists, *blend;
  int64_t *idx;
  float clamp_lo, clamp_hi;
};

__device__ __forceinline__ int64_t knn_cross_length(const int64_t *__restrict__ len, int b, int64_t cap) {
  if (len == nullptr) return cap;
  const int64_t n = len[b];
  return n < 0 ? 0 : (n < cap ? n : cap);
}

template <int Kc, int NORM>
__global__ __launch_bounds__(kKxBlock) void knn_cross_kernel(KnnCrossArgs a) {
  __shared__ float4 s_t[kKxTile];
  const int tid = threadIdx.x;
  const int b = (int)blockIdx.x / a.blocks_per_cloud;      // (< B: the grid is B * blocks_per_cloud)
  const int64_t q0 = (int64_t)((int)blockIdx.x - b * a.blocks_per_cloud) * kKxBlock, q = q0 + tid;
  const int64_t n1 = knn_cross_length(a.len1, b, a.P1), n2 = knn_cross_length(a.len2, b, a.P2);
  const bool inside = q < a.P1;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (inside) {
    const float *__restrict__ p = a.p1 + ((int64_t)b * a.P1 + q) * 3;
    qx = p[0];
    qy = p[1];
    qz = p[2];
  }
  KnnBest<Kc> best;
  knn_clear<Kc>(best);
  const float *__restrict__ cloud = a.p2 + (int64_t)b * a.P2 * 3;
  const int64_t scan = q0 < n1 ? n2 : 0;      // (uniform over the workgroup: one whose queries are all padding searches nothing)
  for (int64_t t0 = 0; t0 < scan; t0 += kKxTile) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kKxTile / kKxBlock; j++) {
      const int s = j * kKxBlock + tid;
      const int64_t t = t0 + s;
      if (t < scan) s_t[s] = make_float4(cloud[3 * t], cloud[3 * t + 1], cloud[3 * t + 2], __int_as_float((int)t));
    }
    __syncthreads();
    const int m = scan - t0 < kKxTile ? (int)(scan - t0) : kKxTile;
#pragma unroll 2
    for (int k = 0; k < m; k++) {
      const float4 p = s_t[k];
      const float d = NORM == 2 ? knn_pair(qx, qy, qz, p.x, p.y, p.z) : knn_pair_l1(qx, qy, qz, p.x, p.y, p.z);
      knn_insert_shift<Kc>(best, d, __float_as_int(p.w));
    }
  }
  if (!inside) return;      // (behind the last barrier)
  const int64_t row = (int64_t)b * a.P1 + q;
  const int limit = q < n1 ? (int)(n2 < (int64_t)a.K ? n2 : (int64_t)a.K) : 0;
  unsigned taken = 0u;      // bit k: slot k holds a neighbour (k < min(K, len2), and a candidate arrived: a NaN never does)
#pragma unroll
  for (int k = 0; k < Kc; k++)
    if (k < limit && best.i[k] != kKnnEmptyRow) taken |= 1u << k;
  if (a.dists != nullptr) {
#pragma unroll
    for (int k = 0; k < Kc; k++) {
      if (k < a.K) a.dists[row * a.K + k] = (taken >> k & 1u) ? best.d[k] : 0.0f;
      if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // (four stores' operands at a time, not Kc)
    }
  }
  if (a.idx != nullptr) {
#pragma unroll
    for (int k = 0; k < Kc; k++) {
      if (k < a.K) a.idx[row * a.K + k] = (taken >> k & 1u) ? (int64_t)(unsigned)best.i[k] : (int64_t)0;      // (a row is never negative)
      if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (a.blend == nullptr) return;
  // The rows become 32-bit byte offsets into the cloud's features (the entry bounds P2 * J): a load is a buffer load, the cloud's
  // descriptor and the column in scalar registers and ONE vector register of address per slot, checked against the cloud's size by
  // the hardware.  A slot without a neighbour reads where slot 0 reads, at weight 0: the column loop then carries no per-slot
  // predicate, and the zero meets only a value that enters the sum anyway.  Eight loads at a time are in flight, not Kc.
  const float *__restrict__ f = a.feat + (int64_t)b * a.P2 * a.J;
  float *__restrict__ o = a.blend + row * a.J;
  if (taken == 0u) {      // (no candidate: nothing to read, and feat may be empty)
    for (int j = 0; j < a.J; j++) o[j] = 0.0f;
    return;
  }
  float sum = 0.0f;
  // (slot 0 is taken whenever any is: the list fills from the front; a taken slot's row is < len2[b] <= P2)
  const int first = best.i[0] * a.J * (int)sizeof(float);
#pragma unroll
  for (int k = 0; k < Kc; k++) {
    const bool on = taken >> k & 1u;
    best.d[k] = on ? knn_blend_weight(best.d[k], a.clamp_lo, a.clamp_hi) : 0.0f;
    best.i[k] = on ? best.i[k] * a.J * (int)sizeof(float) : first;
    sum += best.d[k];
    if (k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
  }
  const float inv = 1.0f / sum;      // (finite: a taken slot's weight is at least 1 / clamp_hi, at most 1 / clamp_lo)
#pragma unroll
  for (int k = 0; k < Kc; k++) best.d[k] *= inv;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(f), 0, (int)(a.P2 * a.J) * (int)sizeof(float), 0x00020000);
  for (int j = 0; j < a.J; j++) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < Kc; k++) {
      acc += best.d[k] * __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, best.i[k], j * (int)sizeof(float), 0));
      if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
    }
    o[j] = acc;
  }
}

template <int Kc>
static int knn_cross_launch(const KnnCrossArgs &a, int norm, unsigned grid, hipStream_t st) {
  if (norm == 2)
    hipLaunchKernelGGL((knn_cross_kernel<Kc, 2>), dim3(grid), dim3(kKxBlock), 0, st, a);
  else
    hipLaunchKernelGGL((knn_cross_kernel<Kc, 1>), dim3(grid), dim3(kKxBlock), 0, st, a);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

static bool knn_cross_al(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

}  // namespace bds

using namespace bds;

extern "C" int bds_cross_knn(int B, int64_t P1, int64_t P2, const float *p1, const float *p2, const int64_t *len1, const int64_t *len2, int K,
                             int norm, float *dists, int64_t *idx, const float *feat, int J, float clamp_lo, float clamp_hi, float *blend,
                             bds_stream_t stream) {
  BDS_REQUIRE(B >= 0 && P1 >= 0 && P2 >= 0 && P2 < (int64_t)kKnnEmptyRow);
  BDS_REQUIRE(K >= 1 && K <= kKxMaxK);
  BDS_REQUIRE(norm == 1 || norm == 2);
  BDS_REQUIRE(dists != nullptr || idx != nullptr || blend != nullptr);
  BDS_REQUIRE((feat != nullptr) == (blend != nullptr));
  if (blend != nullptr) {
    BDS_REQUIRE(norm == 2);
    BDS_REQUIRE(J >= 1 && J <= kKxMaxJ && P2 * J <= ((int64_t)1 << 29));      // (byte offsets of the features in 32 bits)
    BDS_REQUIRE(clamp_lo > 0.0f && clamp_lo <= clamp_hi);      // (false for a NaN on either side)
  }
  BDS_REQUIRE(p1 != nullptr || (int64_t)B * P1 == 0);
  BDS_REQUIRE(p2 != nullptr || (int64_t)B * P2 == 0);
  BDS_REQUIRE(knn_cross_al(p1, 4) && knn_cross_al(p2, 4) && knn_cross_al(dists, 4) && knn_cross_al(feat, 4) && knn_cross_al(blend, 4));
  BDS_REQUIRE(knn_cross_al(idx, 8) && knn_cross_al(len1, 8) && knn_cross_al(len2, 8));
  if (B == 0 || P1 == 0) return BDS_OK;
  const int64_t per_cloud = cdiv(P1, kKxBlock);
  BDS_REQUIRE(per_cloud * B <= (int64_t)0x7fffffff);
  KnnCrossArgs a;
  a.K = K;
  a.J = J;
  a.blocks_per_cloud = (int)per_cloud;
  a.P1 = P1;
  a.P2 = P2;
  a.p1 = p1;
  a.p2 = p2;
  a.feat = feat;
  a.len1 = len1;
  a.len2 = len2;
  a.dists = dists;
  a.blend = blend;
  a.idx = idx;
  a.clamp_lo = clamp_lo;
  a.clamp_hi = clamp_hi;
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)(per_cloud * B);
  if (K <= 4) return knn_cross_launch<4>(a, norm, grid, st);
  if (K <= 8) return knn_cross_launch<8>(a, norm, grid, st);
  if (K <= 16) return knn_cross_launch<16>(a, norm, grid, st);
  return knn_cross_launch<32>(a, norm, grid, st);
}
