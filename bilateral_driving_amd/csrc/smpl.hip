// Pose chain and skinning of the SMPL nodes (models/nodes/smpl.py:267-341, models/human_body.py:158-180,
// third_party/smplx/smplx/lbs.py:362-418, models/modules.py:1168-1188).  The math lives in smpl_math.h.
//   forward: one launch, grid (cdiv(V, 256), I), one thread per point.  Every workgroup rebuilds its instance's 24-joint chain in LDS
//     (the joints' local matrices and the products with A0_inv by 24 threads, the 23 dependent products by one), then streams over the
//     joints: one sampled weight at a time, added into the point's blended 3x4 transform.  The workgroups of column 0 store A.
//   backward: a per-point launch of the same grid and a per-instance launch.  The per-point kernel loads the saved A, runs the joints
//     twice (the blend, then with the blend's gradient the weights' gradients: float atomics into the zeroed field gradient and the
//     coordinate term of the means' gradient), keeps the 24 weights and the 12 floats of the blend's gradient of its 256 points in
//     LDS and forms from them the workgroup's part of v_A [24,12] and v_trans in a fixed order, one (joint, element) per thread,
//     into its own row of the workspace.  The per-instance kernel sums the rows in order and runs the chain backward in LDS.
//     Pose and translation gradients are bit-identical run to run; the field gradient's summation order is the atomics'.
#include "bds_common.h"
#include "smpl_math.h"

namespace bds {

constexpr int kSmplBlock = 256;
constexpr int kSmplPad = kSmplBlock + 1;      // LDS row stride of the per-point slabs (rows a multiple of 64 apart share a bank)

struct SmplArgs {
  int I, V, d, h, w, ratio_dim;
  float ratio;
  SmplParents parents;
  const float *means, *quats, *root_quats, *body_quats, *trans, *J, *A0_inv, *base, *corr, *W, *offset, *scale;
  const uint8_t *present;
};

__device__ __forceinline__ const float *smpl_joint_quat(const SmplArgs &a, int i, int j) {
  return j == 0 ? a.root_quats + (int64_t)i * 4 : a.body_quats + ((int64_t)i * (kSmplJoints - 1) + (j - 1)) * 4;
}

// The chain of instance i in LDS: M [24,12] local, G [24,12] world.  Called by every thread of the workgroup.
__device__ __forceinline__ void smpl_chain_lds(const SmplArgs &a, int i, float *M, float *G) {
  const int t = threadIdx.x;
  const float *J = a.J + (int64_t)i * kSmplJoints * 3;
  if (t < kSmplJoints) {
    float m[kSmplAff];
    smpl_joint_local(smpl_joint_quat(a, i, t), J + t * 3, t ? J + smpl_parent(a.parents, t) * 3 : nullptr, m);
    for (int k = 0; k < kSmplAff; k++) M[t * kSmplAff + k] = m[k];
    if (t == 0)
      for (int k = 0; k < kSmplAff; k++) G[k] = m[k];
  }
  __syncthreads();
  if (t == 0)
    for (int j = 1; j < kSmplJoints; j++) smpl_affine_mul(G + smpl_parent(a.parents, j) * kSmplAff, M + j * kSmplAff, G + j * kSmplAff);
  __syncthreads();
}

// weight of joint j at point p of instance i (the field, or the fixed table when there is none)
__device__ __forceinline__ float smpl_weight(const SmplArgs &a, int i, int p, int j, const SmplCell &c, float *dW) {
  if (a.base == nullptr) return a.W[((int64_t)i * a.V + p) * kSmplJoints + j];
  const int64_t slab = ((int64_t)i * kSmplJoints + j) * ((int64_t)a.d * a.h * a.w);
  return smpl_sample(a.base + slab, a.corr ? a.corr + slab : nullptr, c, a.h, a.w, dW);
}

__device__ __forceinline__ SmplCell smpl_point_cell(const SmplArgs &a, int i, const float *x) {
  if (a.base == nullptr) return SmplCell{};
  return smpl_cell(x, a.offset + (int64_t)i * 3, a.scale[i], a.ratio, a.ratio_dim, a.d, a.h, a.w);
}

__global__ __launch_bounds__(kSmplBlock) void smpl_skin_fwd_kernel(SmplArgs a, float *__restrict__ wm, float *__restrict__ wq,
                                                                   float *__restrict__ A_out) {
  __shared__ float sM[kSmplJoints * kSmplAff], sG[kSmplJoints * kSmplAff], sA[kSmplJoints * kSmplAff];
  const int i = blockIdx.y, t = threadIdx.x;
  const int p = blockIdx.x * kSmplBlock + t;
  const int64_t row = (int64_t)i * a.V + p;
  if (!a.present[i]) {      // (workgroup-uniform) the container's zero row plus the translation, the unit quaternion
    if (blockIdx.x == 0)
      for (int k = t; k < kSmplJoints * kSmplAff; k += kSmplBlock) A_out[(int64_t)i * kSmplJoints * kSmplAff + k] = 0.0f;
    if (p < a.V) {
      for (int k = 0; k < 3; k++) wm[row * 3 + k] = a.trans[i * 3 + k];
      if (wq)
        for (int k = 0; k < 4; k++) wq[row * 4 + k] = k == 0 ? 1.0f : 0.0f;
    }
    return;
  }
  smpl_chain_lds(a, i, sM, sG);
  if (t < kSmplJoints) {
    float m[kSmplAff];
    smpl_joint_skin(sG + t * kSmplAff, a.J + ((int64_t)i * kSmplJoints + t) * 3, a.A0_inv + ((int64_t)i * kSmplJoints + t) * 16, m);
    for (int k = 0; k < kSmplAff; k++) sA[t * kSmplAff + k] = m[k];
  }
  __syncthreads();
  if (blockIdx.x == 0)
    for (int k = t; k < kSmplJoints * kSmplAff; k += kSmplBlock) A_out[(int64_t)i * kSmplJoints * kSmplAff + k] = sA[k];
  if (p >= a.V) return;
  float x[3], T[kSmplAff];
  for (int k = 0; k < 3; k++) x[k] = a.means[row * 3 + k];
  for (int k = 0; k < kSmplAff; k++) T[k] = 0.0f;
  const SmplCell c = smpl_point_cell(a, i, x);
#pragma unroll 2
  for (int j = 0; j < kSmplJoints; j++) {
    const float wj = smpl_weight(a, i, p, j, c, nullptr);
    for (int k = 0; k < kSmplAff; k++) T[k] += wj * sA[j * kSmplAff + k];
  }
  float om[3], oq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q[4] = {1.0f, 0.0f, 0.0f, 0.0f};
  if (wq)
    for (int k = 0; k < 4; k++) q[k] = a.quats[row * 4 + k];
  smpl_point_fwd(T, x, a.trans + i * 3, q, wq == nullptr, om, oq);
  for (int k = 0; k < 3; k++) wm[row * 3 + k] = om[k];
  if (wq)
    for (int k = 0; k < 4; k++) wq[row * 4 + k] = oq[k];
}

__global__ __launch_bounds__(kSmplBlock) void smpl_skin_bwd_kernel(SmplArgs a, const float *__restrict__ A, const float *__restrict__ v_wm,
                                                                   const float *__restrict__ v_wq, float *__restrict__ v_means,
                                                                   float *__restrict__ v_quats, float *__restrict__ v_corr,
                                                                   float *__restrict__ part) {
  __shared__ float sA[kSmplJoints * kSmplAff], sW[kSmplJoints * kSmplPad], sV[kSmplAff * kSmplPad];
  const int i = blockIdx.y, t = threadIdx.x;
  const int p = blockIdx.x * kSmplBlock + t;
  const int64_t row = (int64_t)i * a.V + p;
  const bool present = a.present[i] != 0, valid = p < a.V;
  for (int k = t; k < kSmplJoints * kSmplAff; k += kSmplBlock) sA[k] = A[(int64_t)i * kSmplJoints * kSmplAff + k];
  __syncthreads();
  float vT[kSmplAff];
  for (int k = 0; k < kSmplAff; k++) vT[k] = 0.0f;
  if (valid) {
    float gm[3], vx[3] = {0.0f, 0.0f, 0.0f}, vq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) gm[k] = v_wm[row * 3 + k];
    if (!present) {      // only the translation sees an absent instance's rows
      for (int r = 0; r < 3; r++) vT[r * 4 + 3] = gm[r];
      for (int j = 0; j < kSmplJoints; j++) sW[j * kSmplPad + t] = 0.0f;
    } else {
      float x[3], q[4] = {1.0f, 0.0f, 0.0f, 0.0f}, gq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, T[kSmplAff];
      for (int k = 0; k < 3; k++) x[k] = a.means[row * 3 + k];
      for (int k = 0; k < kSmplAff; k++) T[k] = 0.0f;
      const SmplCell c = smpl_point_cell(a, i, x);
#pragma unroll 2
      for (int j = 0; j < kSmplJoints; j++) {
        const float wj = smpl_weight(a, i, p, j, c, nullptr);
        sW[j * kSmplPad + t] = wj;
        for (int k = 0; k < kSmplAff; k++) T[k] += wj * sA[j * kSmplAff + k];
      }
      if (v_wq)
        for (int k = 0; k < 4; k++) {
          q[k] = a.quats[row * 4 + k];
          gq[k] = v_wq[row * 4 + k];
        }
      smpl_point_bwd(T, x, q, gm, gq, v_wq == nullptr, vT, vx, vq);
      if (a.base != nullptr) {      // the weights' gradients: v_w_j = <vT, A_j>
        const int64_t vol = (int64_t)a.d * a.h * a.w;
#pragma unroll 1
        for (int j = 0; j < kSmplJoints; j++) {
          const float vw = smpl_dot12(vT, sA + j * kSmplAff);
          float dW[3];
          smpl_weight(a, i, p, j, c, dW);
          for (int k = 0; k < 3; k++) vx[k] += vw * dW[k];
          if (v_corr) {
            float *g = v_corr + ((int64_t)i * kSmplJoints + j) * vol;
            for (int k = 0; k < 8; k++) atomicAdd(g + smpl_corner_index(c, k, a.h, a.w), vw * smpl_corner_weight(c, k));
          }
        }
      }
    }
    for (int k = 0; k < 3; k++) v_means[row * 3 + k] = vx[k];
    if (v_quats)
      for (int k = 0; k < 4; k++) v_quats[row * 4 + k] = vq[k];
  } else {
    for (int j = 0; j < kSmplJoints; j++) sW[j * kSmplPad + t] = 0.0f;
  }
  for (int k = 0; k < kSmplAff; k++) sV[k * kSmplPad + t] = vT[k];
  __syncthreads();
  // the workgroup's part of v_A [24,12] and of v_trans [3], each by one thread over the 256 points in order
  float *__restrict__ out = part + ((int64_t)i * gridDim.x + blockIdx.x) * kSmplPart;
  for (int o = t; o < kSmplPart; o += kSmplBlock) {
    float s = 0.0f;
    if (o < kSmplJoints * kSmplAff) {
      const float *wr = sW + (o / kSmplAff) * kSmplPad, *vr = sV + (o % kSmplAff) * kSmplPad;
      for (int n = 0; n < kSmplBlock; n++) s += wr[n] * vr[n];
    } else if (o < kSmplJoints * kSmplAff + 3) {
      const float *vr = sV + ((o - kSmplJoints * kSmplAff) * 4 + 3) * kSmplPad;
      for (int n = 0; n < kSmplBlock; n++) s += vr[n];
    }
    out[o] = s;
  }
}

// One workgroup per instance: the workgroups' rows summed in order, then the chain backward in LDS.
__global__ __launch_bounds__(kSmplBlock) void smpl_pose_bwd_kernel(SmplArgs a, int blocks, const float *__restrict__ part,
                                                                   float *__restrict__ v_root, float *__restrict__ v_body,
                                                                   float *__restrict__ v_trans) {
  __shared__ float sM[kSmplJoints * kSmplAff], sG[kSmplJoints * kSmplAff], sVA[kSmplPart], sVG[kSmplJoints * kSmplAff],
      sVR[kSmplJoints * 9];
  const int i = blockIdx.x, t = threadIdx.x;
  for (int o = t; o < kSmplPart; o += kSmplBlock) {
    float s = 0.0f;
    for (int b = 0; b < blocks; b++) s += part[((int64_t)i * blocks + b) * kSmplPart + o];
    sVA[o] = s;
  }
  __syncthreads();
  if (t < 3) v_trans[i * 3 + t] = sVA[kSmplJoints * kSmplAff + t];
  if (!a.present[i]) {      // (workgroup-uniform)
    if (t < kSmplJoints)
      for (int k = 0; k < 4; k++) (t == 0 ? v_root + (int64_t)i * 4 : v_body + ((int64_t)i * (kSmplJoints - 1) + (t - 1)) * 4)[k] = 0.0f;
    return;
  }
  smpl_chain_lds(a, i, sM, sG);
  if (t < kSmplJoints) {
    float va[kSmplAff], vg[kSmplAff];
    for (int k = 0; k < kSmplAff; k++) va[k] = sVA[t * kSmplAff + k];
    smpl_joint_skin_vjp(va, a.J + ((int64_t)i * kSmplJoints + t) * 3, a.A0_inv + ((int64_t)i * kSmplJoints + t) * 16, vg);
    for (int k = 0; k < kSmplAff; k++) sVG[t * kSmplAff + k] = vg[k];
  }
  __syncthreads();
  if (t == 0) {      // children before parents: parents[j] < j
    for (int j = kSmplJoints - 1; j >= 1; j--) {
      const int pj = smpl_parent(a.parents, j);
      smpl_affine_mul_vjp(sG + pj * kSmplAff, sM + j * kSmplAff, sVG + j * kSmplAff, sVG + pj * kSmplAff, sVR + j * 9);
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) sVR[r * 3 + c] = sVG[r * 4 + c];
  }
  __syncthreads();
  if (t < kSmplJoints) {
    float vr[9], vq[4];
    for (int k = 0; k < 9; k++) vr[k] = sVR[t * 9 + k];
    smpl_joint_local_vjp(smpl_joint_quat(a, i, t), vr, vq);
    float *o = t == 0 ? v_root + (int64_t)i * 4 : v_body + ((int64_t)i * (kSmplJoints - 1) + (t - 1)) * 4;
    for (int k = 0; k < 4; k++) o[k] = vq[k];
  }
}

static size_t smpl_temp_bytes(int I, int V) { return align_up((size_t)I * (size_t)cdiv(V, kSmplBlock) * kSmplPart * sizeof(float), 256); }

// host: every parents[j] of j = 1..23 in [0, j), packed 5 bits each
static bool smpl_pack_parents(const int32_t *parents, SmplParents *out) {
  out->lo = out->hi = 0;
  for (int j = 1; j < kSmplJoints; j++) {
    if (parents[j] < 0 || parents[j] >= j) return false;
    (j < 12 ? out->lo : out->hi) |= (uint64_t)parents[j] << (5 * (j < 12 ? j : j - 12));
  }
  return true;
}

}  // namespace bds

using namespace bds;

extern "C" size_t bds_smpl_skin_bwd_temp_bytes(int I, int V) {
  if (I < 1 || V < 1) return 0;
  return smpl_temp_bytes(I, V);
}

static int smpl_args(int I, int V, const float *means, const float *quats, const float *root_quats, const float *body_quats,
                     const float *trans, const uint8_t *present, const float *J_canonical, const float *A0_inv, const int32_t *parents,
                     const float *voxel_base, const float *voxel_corr, const float *W, int d, int h, int w, const float *offset,
                     const float *scale, float ratio, int ratio_dim, bool ball, SmplArgs *a) {
  BDS_REQUIRE(I >= 1 && V >= 1 && (int64_t)I * V <= (int64_t)1 << 30);
  BDS_REQUIRE(means && (ball || quats) && root_quats && body_quats && present && J_canonical && A0_inv && parents);
  if (voxel_base) {
    BDS_REQUIRE(offset && scale && d >= 1 && h >= 1 && w >= 1 && (int64_t)d * h * w <= (int64_t)1 << 30);
    BDS_REQUIRE(ratio_dim >= 0 && ratio_dim <= 2);
  } else {
    BDS_REQUIRE(W && !voxel_corr);
  }
  SmplParents packed;
  BDS_REQUIRE(smpl_pack_parents(parents, &packed));
  *a = SmplArgs{I, V, d, h, w, ratio_dim, ratio, packed, means, quats, root_quats, body_quats, trans, J_canonical, A0_inv, voxel_base,
                voxel_corr, W, offset, scale, present};
  return BDS_OK;
}

extern "C" int bds_smpl_skin_fwd(int I, int V, const float *means, const float *quats, const float *root_quats, const float *body_quats,
                                 const float *trans, const uint8_t *present, const float *J_canonical, const float *A0_inv,
                                 const int32_t *parents, const float *voxel_base, const float *voxel_corr, const float *W, int d, int h, int w,
                                 const float *offset, const float *scale, float ratio, int ratio_dim, float *world_means,
                                 float *world_quats, float *A, bds_stream_t stream) {
  SmplArgs a;
  const int rc = smpl_args(I, V, means, quats, root_quats, body_quats, trans, present, J_canonical, A0_inv, parents, voxel_base,
                           voxel_corr, W, d, h, w, offset, scale, ratio, ratio_dim, world_quats == nullptr, &a);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(trans && world_means && A);
  hipLaunchKernelGGL(smpl_skin_fwd_kernel, dim3((unsigned)cdiv(V, kSmplBlock), (unsigned)I), dim3(kSmplBlock), 0, as_stream(stream), a,
                     world_means, world_quats, A);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_smpl_skin_bwd(int I, int V, const float *means, const float *quats, const float *root_quats, const float *body_quats,
                                 const uint8_t *present, const float *J_canonical, const float *A0_inv, const int32_t *parents,
                                 const float *voxel_base, const float *voxel_corr, const float *W, int d, int h, int w, const float *offset,
                                 const float *scale, float ratio, int ratio_dim, const float *A, const float *v_world_means,
                                 const float *v_world_quats, float *v_means, float *v_quats, float *v_root_quats, float *v_body_quats,
                                 float *v_trans, float *v_voxel_corr, void *temp, size_t temp_bytes, bds_stream_t stream) {
  SmplArgs a;
  const int rc = smpl_args(I, V, means, quats, root_quats, body_quats, nullptr, present, J_canonical, A0_inv, parents, voxel_base,
                           voxel_corr, W, d, h, w, offset, scale, ratio, ratio_dim, v_world_quats == nullptr, &a);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(A && v_world_means && v_means && (v_world_quats == nullptr) == (v_quats == nullptr) && v_root_quats && v_body_quats && v_trans);
  BDS_REQUIRE(voxel_base || !v_voxel_corr);
  BDS_REQUIRE(temp && temp_bytes >= smpl_temp_bytes(I, V) && aligned16(temp));
  hipStream_t st = as_stream(stream);
  if (v_voxel_corr &&
      hipMemsetAsync(v_voxel_corr, 0, (size_t)I * kSmplJoints * (size_t)d * h * w * sizeof(float), st) != hipSuccess)
    return BDS_ELAUNCH;
  const int blocks = (int)cdiv(V, kSmplBlock);
  hipLaunchKernelGGL(smpl_skin_bwd_kernel, dim3((unsigned)blocks, (unsigned)I), dim3(kSmplBlock), 0, st, a, A, v_world_means, v_world_quats,
                     v_means, v_quats, v_voxel_corr, static_cast<float *>(temp));
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(smpl_pose_bwd_kernel, dim3((unsigned)I), dim3(kSmplBlock), 0, st, a, blocks, (const float *)temp, v_root_quats,
                     v_body_quats, v_trans);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
