// Pose transform of the node classes (RigidNodes, models/nodes/rigid.py:385-493; DeformableNodes, models/nodes/deformable.py:49-114):
// instance-local means / quaternions to the world by the instance poses of the current frame, and the opacity mask of the frame's
// visible instances.  The per-point math lives in nodes_math.h.
//   forward: one launch, one thread per point.
//   backward: one launch over waves that own contiguous ranges of 64-point tiles.  Each wave writes the point gradients and reduces
//     the instance part (16 floats per point) of the ids among its lanes: the distinct ids are peeled one at a time (usually one or
//     two per tile), each by a fixed-order butterfly, and added to the wave's own row of a [waves, I, 16] slab (only that wave
//     touches the row, always from the same lane per float).  A second launch sums the slab per instance in a fixed order and applies
//     the instance-level chain rule.  No float atomics: the gradients are bit-identical run to run.
#include "bds_common.h"
#include "nodes_math.h"

namespace bds {

constexpr int kNpBlock = 256;                    // 4 waves
constexpr int kNpWavesPerBlock = kNpBlock / kWave;
constexpr int kNpReduceRows = 16;                // the reduce's wave-row lanes per instance (16 x 16 threads)

// waves of the backward: contiguous tile ranges, the slab kept to <= 128 Ki instance rows (8 MB) unless I alone exceeds that
struct NpGrid {
  int64_t tiles, tiles_per_wave, waves;
};
static NpGrid np_grid(int64_t N, int I) {
  NpGrid g;
  g.tiles = cdiv(N, kWave);
  int64_t cap = (int64_t)131072 / (I > 0 ? I : 1);
  cap = cap < 256 ? 256 : (cap > 2048 ? 2048 : cap);
  const int64_t w = g.tiles < cap ? g.tiles : cap;
  g.tiles_per_wave = w > 0 ? cdiv(g.tiles, w) : 0;
  g.waves = g.tiles_per_wave > 0 ? cdiv(g.tiles, g.tiles_per_wave) : 0;
  return g;
}
static size_t np_slab_bytes(int64_t N, int I) { return align_up((size_t)np_grid(N, I).waves * (size_t)I * kNpSlab * sizeof(float), 256); }

__device__ __forceinline__ void np_load4(const float *__restrict__ p, float *o) {
  for (int k = 0; k < 4; k++) o[k] = p[k];
}
__device__ __forceinline__ void np_load3(const float *__restrict__ p, float *o) {
  for (int k = 0; k < 3; k++) o[k] = p[k];
}

// An id outside [0, I) reads nothing: the point's outputs are NaN and bit 0 of *bad_ids is raised (sticky).
__global__ __launch_bounds__(kNpBlock) void node_pose_fwd_kernel(int64_t N, int I, int f, int interp, const float *__restrict__ means,
                                                                 const float *__restrict__ quats, const float *__restrict__ logits,
                                                                 const int64_t *__restrict__ ids, const float *__restrict__ iq,
                                                                 const float *__restrict__ it, const uint8_t *__restrict__ fv,
                                                                 float *__restrict__ wm, float *__restrict__ wq, float *__restrict__ op,
                                                                 uint32_t *__restrict__ bad_ids) {
  const int64_t p = (int64_t)blockIdx.x * kNpBlock + threadIdx.x;
  if (p >= N) return;
  const int64_t id = ids[p];
  if (id < 0 || id >= I) {
    if (bad_ids) atomicOr(bad_ids, 1u);
    const float nan = __int_as_float(0x7fc00000);
    for (int k = 0; k < 3; k++) wm[p * 3 + k] = nan;
    for (int k = 0; k < 4; k++) wq[p * 4 + k] = nan;
    op[p] = nan;
    return;
  }
  const int64_t row = (int64_t)f * I + id;
  float q[4], t[3], qr[4], tr[3], m[3], qp[4];
  np_load4(iq + row * 4, q);
  np_load3(it + row * 3, t);
  for (int k = 0; k < 4; k++) qr[k] = q[k];
  for (int k = 0; k < 3; k++) tr[k] = t[k];
  if (interp) {   // rigid.py:392-432: frames f-1 and f+1 where both see the instance; transform_quats keeps frame f
    const int64_t r0 = row - I, r1 = row + I;
    if (fv[r0] && fv[r1]) {
      float q0[4], q1[4];
      np_load4(iq + r0 * 4, q0);
      np_load4(iq + r1 * 4, q1);
      np_interp_quats(q0, q1, qr);
      for (int k = 0; k < 3; k++) tr[k] = (it[r0 * 3 + k] + it[r1 * 3 + k]) * 0.5f;
    }
  }
  np_load3(means + p * 3, m);
  np_load4(quats + p * 4, qp);
  float om[3], oq[4], oo;
  np_forward(qr, tr, q, m, qp, logits[p], fv[row] ? 1.0f : 0.0f, om, oq, &oo);
  for (int k = 0; k < 3; k++) wm[p * 3 + k] = om[k];
  for (int k = 0; k < 4; k++) wq[p * 4 + k] = oq[k];
  op[p] = oo;
}

__global__ __launch_bounds__(kNpBlock) void node_pose_bwd_kernel(int64_t N, int I, int f, NpGrid g, const float *__restrict__ means,
                                                                 const float *__restrict__ quats, const float *__restrict__ logits,
                                                                 const int64_t *__restrict__ ids, const float *__restrict__ iq,
                                                                 const uint8_t *__restrict__ fv, const float *__restrict__ v_wm,
                                                                 const float *__restrict__ v_wq, const float *__restrict__ v_op,
                                                                 float *__restrict__ v_means, float *__restrict__ v_quats,
                                                                 float *__restrict__ v_logits, float *__restrict__ slab) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * kNpWavesPerBlock + (threadIdx.x >> 6);
  const int64_t t0 = wave * g.tiles_per_wave;
  int64_t t1 = t0 + g.tiles_per_wave;
  if (t1 > g.tiles) t1 = g.tiles;
  const int slot = butterfly_slot(lane);
  const bool writer = (lane & 3) == 0;        // one lane per slot (the four lanes of a quad hold the same total)
  float *__restrict__ srow = slab + wave * (int64_t)I * kNpSlab;
  int cur = -1;                               // wave-uniform: the instance whose running sum `acc` holds
  float acc = 0.0f;
  for (int64_t tile = t0; tile < t1; tile++) {   // (wave-uniform loop: every lane runs the butterflies)
    const int64_t p = tile * kWave + lane;
    const bool valid = p < N;
    int id = -1;
    float part[kNpSlab];
    for (int k = 0; k < kNpSlab; k++) part[k] = 0.0f;
    if (valid) {
      const int64_t id64 = ids[p];
      float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vl = 0.0f;
      if (id64 >= 0 && id64 < I) {
        id = (int)id64;
        const int64_t row = (int64_t)f * I + id;
        float q[4], m[3], qp[4], gm[3], gq[4];
        np_load4(iq + row * 4, q);
        np_load3(means + p * 3, m);
        np_load4(quats + p * 4, qp);
        np_load3(v_wm + p * 3, gm);
        np_load4(v_wq + p * 4, gq);
        np_backward(q, m, qp, logits[p], fv[row] ? 1.0f : 0.0f, gm, gq, v_op[p], vm, vq, &vl, part);
      }
      for (int k = 0; k < 3; k++) v_means[p * 3 + k] = vm[k];
      for (int k = 0; k < 4; k++) v_quats[p * 4 + k] = vq[k];
      v_logits[p] = vl;
    }
    uint64_t pending = __ballot(id >= 0);
    while (pending) {
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const int lid = __builtin_amdgcn_readlane(id, leader);
      const bool mine = id == lid;
      pending &= ~(uint64_t)__ballot(mine);
      float v[kNpSlab];
      for (int k = 0; k < kNpSlab; k++) v[k] = mine ? part[k] : 0.0f;
      const float s = butterfly_sum16(v, lane);
      if (lid != cur) {
        if (cur >= 0 && writer) srow[(int64_t)cur * kNpSlab + slot] += acc;
        cur = lid;
        acc = 0.0f;
      }
      acc += s;
    }
  }
  if (cur >= 0 && writer) srow[(int64_t)cur * kNpSlab + slot] += acc;
}

// One workgroup per instance: the slab's rows summed in a fixed order (16 strided partial sums, then in order), the instance-level chain
// rule, frame f's rows of v_iq / v_it stored.
__global__ __launch_bounds__(kNpBlock) void node_pose_reduce_kernel(int I, int f, int64_t waves, const float *__restrict__ slab,
                                                                    const float *__restrict__ iq, float *__restrict__ v_iq,
                                                                    float *__restrict__ v_it) {
  __shared__ float red[kNpReduceRows][kNpSlab];
  __shared__ float tot[kNpSlab];
  const int i = blockIdx.x, c = threadIdx.x & (kNpSlab - 1), r = threadIdx.x / kNpSlab;
  float s = 0.0f;
  for (int64_t w = r; w < waves; w += kNpReduceRows) s += slab[(w * I + i) * kNpSlab + c];
  red[r][c] = s;
  __syncthreads();
  if (r == 0) {
    float t = 0.0f;
    for (int k = 0; k < kNpReduceRows; k++) t += red[k][c];
    tot[c] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t row = (int64_t)f * I + i;
    float q[4], vq[4], vt[3], part[kNpSlab];
    for (int k = 0; k < 4; k++) q[k] = iq[row * 4 + k];
    for (int k = 0; k < kNpSlab; k++) part[k] = tot[k];
    np_instance_chain(q, part, vq, vt);
    for (int k = 0; k < 4; k++) v_iq[row * 4 + k] = vq[k];
    for (int k = 0; k < 3; k++) v_it[row * 3 + k] = vt[k];
  }
}

}  // namespace bds

using namespace bds;

extern "C" size_t bds_node_pose_bwd_temp_bytes(int64_t N, int I) {
  if (N <= 0 || I < 1) return 0;
  return np_slab_bytes(N, I);
}

extern "C" int bds_node_pose_fwd(int64_t N, int F, int I, int cur_frame, int interpolate, const float *means, const float *quats,
                                 const float *logits, const int64_t *point_ids, const float *instances_quats,
                                 const float *instances_trans, const uint8_t *instances_fv, float *world_means, float *world_quats,
                                 float *opacities, uint32_t *bad_ids, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && F >= 1 && I >= 1 && cur_frame >= 0 && cur_frame < F);
  BDS_REQUIRE(!interpolate || (cur_frame - 1 > 0 && cur_frame + 1 < F));
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(means && quats && logits && point_ids && instances_quats && instances_trans && instances_fv && world_means && world_quats &&
              opacities);
  hipLaunchKernelGGL(node_pose_fwd_kernel, dim3((unsigned)cdiv(N, kNpBlock)), dim3(kNpBlock), 0, as_stream(stream), N, I, cur_frame,
                     interpolate ? 1 : 0, means, quats, logits, point_ids, instances_quats, instances_trans, instances_fv, world_means,
                     world_quats, opacities, bad_ids);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_node_pose_bwd(int64_t N, int F, int I, int cur_frame, const float *means, const float *quats, const float *logits,
                                 const int64_t *point_ids, const float *instances_quats, const uint8_t *instances_fv, const float *v_world_means,
                                 const float *v_world_quats, const float *v_opacities, float *v_means, float *v_quats, float *v_logits,
                                 float *v_instances_quats, float *v_instances_trans, void *temp, size_t temp_bytes, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && F >= 1 && I >= 1 && cur_frame >= 0 && cur_frame < F);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(means && quats && logits && point_ids && instances_quats && instances_fv && v_world_means && v_world_quats && v_opacities &&
              v_means && v_quats && v_logits && v_instances_quats && v_instances_trans);
  const size_t need = np_slab_bytes(N, I);
  BDS_REQUIRE(temp && temp_bytes >= need && aligned16(temp));
  const NpGrid g = np_grid(N, I);
  hipStream_t st = as_stream(stream);
  float *slab = static_cast<float *>(temp);
  if (hipMemsetAsync(slab, 0, need, st) != hipSuccess) return BDS_ELAUNCH;
  if (hipMemsetAsync(v_instances_quats, 0, (size_t)F * I * 4 * sizeof(float), st) != hipSuccess) return BDS_ELAUNCH;
  if (hipMemsetAsync(v_instances_trans, 0, (size_t)F * I * 3 * sizeof(float), st) != hipSuccess) return BDS_ELAUNCH;
  hipLaunchKernelGGL(node_pose_bwd_kernel, dim3((unsigned)cdiv(g.waves, kNpWavesPerBlock)), dim3(kNpBlock), 0, st, N, I, cur_frame, g,
                     means, quats, logits, point_ids, instances_quats, instances_fv, v_world_means, v_world_quats, v_opacities, v_means,
                     v_quats, v_logits, slab);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(node_pose_reduce_kernel, dim3((unsigned)I), dim3(kNpBlock), 0, st, I, cur_frame, g.waves, (const float *)slab,
                     instances_quats, v_instances_quats, v_instances_trans);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
