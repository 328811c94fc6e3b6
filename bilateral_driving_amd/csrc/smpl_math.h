// Math of the SMPL nodes' pose chain and skinning (models/nodes/smpl.py:267-341 transform_means_and_quats / transform_means,
// models/human_body.py:158-180 SMPLTemplate.forward, third_party/smplx/smplx/lbs.py:362-418 batch_rigid_transform,
// models/modules.py:1168-1188 VoxelDeformer.forward / normalize), used by csrc/smpl.hip and by the host shim
// tests/hostmath_smpl_shim.hip.  Affine matrices are 3x4 row-major {R | t} with the implied bottom row {0, 0, 0, 1}.
//   pose, per joint j:  u = q_j / |q_j|,  M_j = {R(u) | J_j - J_parent(j)}  (J_0 for the root; R: pytorch3d's quaternion_to_matrix,
//                       2 / |u|^2),  G_0 = M_0,  G_j = G_parent(j) M_j,  A_j = {G_j.R | G_j.t - G_j.R J_j} A0_inv_j   (rows 0..2)
//   weights, per point: n = (x - offset) / scale, component ratio_dim times ratio; trilinear sample of voxel_base + voxel_corr
//                       (align_corners, border padding: the unnormalised coordinate clamped into [0, size - 1], a clamped axis has no
//                       coordinate gradient), grid x -> w, y -> h, z -> d
//   point:              T = sum_j w_j A_j,  world_mean = T.R x + T.t + trans,
//                       world_quat = quat_mult(n(matrix_to_quaternion(T.R)), n(q))    (n = q / |q|)
// T.R is a blend of rotations and not orthogonal, so matrix_to_quaternion's four candidates differ: pytorch3d's rule is followed
// (largest q_abs, divided by 2 max(q_abs, 0.1), sign to w >= 0), and the gradient is that branch's.
#pragma once
#include <math.h>
#include <stdint.h>
#include "nodes_math.h"

namespace bds {

constexpr int kSmplJoints = 24;
constexpr int kSmplAff = 12;                              // floats of one 3x4 matrix
constexpr int kSmplPart = kSmplJoints * kSmplAff + 4;     // per-workgroup partial: v_A [24,12], v_trans [3], one pad

// the parent table, 5 bits per joint in two words (12 joints each): no indexed thread-local array anywhere
struct SmplParents { uint64_t lo, hi; };
BDS_HD int smpl_parent(const SmplParents &p, int j) { return (int)(((j < 12 ? p.lo : p.hi) >> (5 * (j < 12 ? j : j - 12))) & 31u); }

// ---- pose chain -------------------------------------------------------------------------------------------------------------------
// pytorch3d's quaternion_to_matrix: correct for any non-zero length (two_s = 2 / |u|^2)
BDS_HD void smpl_quat_to_matrix(const float *u, float *R) {
  const float r = u[0], i = u[1], j = u[2], k = u[3];
  const float s = 2.0f / (r * r + i * i + j * j + k * k);
  R[0] = 1.0f - s * (j * j + k * k);
  R[1] = s * (i * j - k * r);
  R[2] = s * (i * k + j * r);
  R[3] = s * (i * j + k * r);
  R[4] = 1.0f - s * (i * i + k * k);
  R[5] = s * (j * k - i * r);
  R[6] = s * (i * k - j * r);
  R[7] = s * (j * k + i * r);
  R[8] = 1.0f - s * (i * i + j * j);
}

BDS_HD void smpl_quat_to_matrix_vjp(const float *u, const float *v, float *vu) {
  const float r = u[0], i = u[1], j = u[2], k = u[3];
  const float s = 2.0f / (r * r + i * i + j * j + k * k);
  // v_s = <v, P>, R = 1 + s P
  const float vs = -v[0] * (j * j + k * k) + v[1] * (i * j - k * r) + v[2] * (i * k + j * r) + v[3] * (i * j + k * r) -
                   v[4] * (i * i + k * k) + v[5] * (j * k - i * r) + v[6] * (i * k - j * r) + v[7] * (j * k + i * r) - v[8] * (i * i + j * j);
  const float c = -s * s * vs;      // d s / d u = -s^2 u
  vu[0] = s * (k * (v[3] - v[1]) + j * (v[2] - v[6]) + i * (v[7] - v[5])) + c * r;
  vu[1] = s * (j * (v[1] + v[3]) + k * (v[2] + v[6]) - 2.0f * i * (v[4] + v[8]) + r * (v[7] - v[5])) + c * i;
  vu[2] = s * (-2.0f * j * (v[0] + v[8]) + i * (v[1] + v[3]) + r * (v[2] - v[6]) + k * (v[5] + v[7])) + c * j;
  vu[3] = s * (-2.0f * k * (v[0] + v[4]) + r * (v[3] - v[1]) + i * (v[2] + v[6]) + j * (v[5] + v[7])) + c * k;
}

// M_j of the raw quaternion q and the rest joints (Jp: the parent's, NULL for the root)
BDS_HD void smpl_joint_local(const float *q, const float *Jj, const float *Jp, float *M) {
  float u[4], R[9];
  np_normalize(q, u);
  smpl_quat_to_matrix(u, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[r * 4 + c] = R[r * 3 + c];
    M[r * 4 + 3] = Jp ? Jj[r] - Jp[r] : Jj[r];
  }
}

BDS_HD void smpl_joint_local_vjp(const float *q, const float *vR, float *vq) {
  float u[4], vu[4];
  const float inv = np_normalize(q, u);
  smpl_quat_to_matrix_vjp(u, vR, vu);
  np_normalize_vjp(u, inv, vu, vq);
}

// G = Gp M
BDS_HD void smpl_affine_mul(const float *Gp, const float *M, float *G) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++)
      G[r * 4 + c] = Gp[r * 4] * M[c] + Gp[r * 4 + 1] * M[4 + c] + Gp[r * 4 + 2] * M[8 + c] + (c == 3 ? Gp[r * 4 + 3] : 0.0f);
}

// of G = Gp M: vGp += vG M^T (with the translation row), vR = Gp.R^T vG.R (M's translation is a constant)
BDS_HD void smpl_affine_mul_vjp(const float *Gp, const float *M, const float *vG, float *vGp, float *vR) {
  for (int r = 0; r < 3; r++) {
    for (int k = 0; k < 3; k++)
      vGp[r * 4 + k] += vG[r * 4] * M[k * 4] + vG[r * 4 + 1] * M[k * 4 + 1] + vG[r * 4 + 2] * M[k * 4 + 2] + vG[r * 4 + 3] * M[k * 4 + 3];
    vGp[r * 4 + 3] += vG[r * 4 + 3];
  }
  for (int k = 0; k < 3; k++)
    for (int c = 0; c < 3; c++) vR[k * 3 + c] = Gp[k] * vG[c] + Gp[4 + k] * vG[4 + c] + Gp[8 + k] * vG[8 + c];
}

// A_j (rows 0..2) of G_j, the rest joint and A0_inv_j [4,4]
BDS_HD void smpl_joint_skin(const float *G, const float *Jj, const float *B, float *A) {
  for (int r = 0; r < 3; r++) {
    const float t = G[r * 4 + 3] - (G[r * 4] * Jj[0] + G[r * 4 + 1] * Jj[1] + G[r * 4 + 2] * Jj[2]);
    for (int c = 0; c < 4; c++) A[r * 4 + c] = G[r * 4] * B[c] + G[r * 4 + 1] * B[4 + c] + G[r * 4 + 2] * B[8 + c] + t * B[12 + c];
  }
}

BDS_HD void smpl_joint_skin_vjp(const float *vA, const float *Jj, const float *B, float *vG) {
  for (int r = 0; r < 3; r++) {
    float a[4];
    for (int k = 0; k < 4; k++) a[k] = vA[r * 4] * B[k * 4] + vA[r * 4 + 1] * B[k * 4 + 1] + vA[r * 4 + 2] * B[k * 4 + 2] + vA[r * 4 + 3] * B[k * 4 + 3];
    for (int k = 0; k < 3; k++) vG[r * 4 + k] = a[k] - a[3] * Jj[k];
    vG[r * 4 + 3] = a[3];
  }
}

// ---- the weight field -------------------------------------------------------------------------------------------------------------
// One point's cell: the two indices and the fraction per axis, and g = d(unnormalised coordinate) / d(x) (0 on a clamped axis).
struct SmplCell {
  int x0, x1, y0, y1, z0, z1;
  float fx, fy, fz, gx, gy, gz;
};

// one axis: n in [-1, 1] -> [0, size - 1] (align_corners), clamped (border); NaN goes to 0, so the indices are always in range
BDS_HD void smpl_axis(float n, int size, float dn, int *i0, int *i1, float *f, float *g) {
  float u = ((n + 1.0f) / 2.0f) * (float)(size - 1);
  const float top = (float)(size - 1);
  float m = 1.0f;
  if (!(u > 0.0f)) {
    u = 0.0f;
    m = 0.0f;
  } else if (u >= top) {
    u = top;
    m = 0.0f;
  }
  int a = (int)floorf(u);
  a = a < 0 ? 0 : (a > size - 1 ? size - 1 : a);
  *i0 = a;
  *i1 = a + 1 > size - 1 ? size - 1 : a + 1;      // (the upper face: fraction 0, the same cell twice)
  *f = u - (float)a;
  *g = m * (top / 2.0f) * dn;
}

BDS_HD SmplCell smpl_cell(const float *x, const float *offset, float scale, float ratio, int ratio_dim, int d, int h, int w) {
  SmplCell c;
  const float rx = ratio_dim == 0 ? ratio : 1.0f, ry = ratio_dim == 1 ? ratio : 1.0f, rz = ratio_dim == 2 ? ratio : 1.0f;
  smpl_axis((x[0] - offset[0]) / scale * rx, w, rx / scale, &c.x0, &c.x1, &c.fx, &c.gx);
  smpl_axis((x[1] - offset[1]) / scale * ry, h, ry / scale, &c.y0, &c.y1, &c.fy, &c.gy);
  smpl_axis((x[2] - offset[2]) / scale * rz, d, rz / scale, &c.z0, &c.z1, &c.fz, &c.gz);
  return c;
}

// corner k (bit 0: x, bit 1: y, bit 2: z) of the cell: its element in a [d,h,w] slab and its trilinear weight
BDS_HD int smpl_corner_index(const SmplCell &c, int k, int h, int w) {
  return (((k & 4) ? c.z1 : c.z0) * h + ((k & 2) ? c.y1 : c.y0)) * w + ((k & 1) ? c.x1 : c.x0);
}
BDS_HD float smpl_corner_weight(const SmplCell &c, int k) {
  return ((k & 1) ? c.fx : 1.0f - c.fx) * ((k & 2) ? c.fy : 1.0f - c.fy) * ((k & 4) ? c.fz : 1.0f - c.fz);
}

// The sampled weight of one channel (base + corr per fetched corner; corr may be NULL); dW (may be NULL): its gradient to x.
BDS_HD float smpl_sample(const float *base, const float *corr, const SmplCell &c, int h, int w, float *dW) {
  float v[8];
  for (int k = 0; k < 8; k++) {
    const int e = smpl_corner_index(c, k, h, w);
    v[k] = corr ? base[e] + corr[e] : base[e];
  }
  float s = 0.0f;
  for (int k = 0; k < 8; k++) s += v[k] * smpl_corner_weight(c, k);
  if (dW) {
    const float ax = 1.0f - c.fx, ay = 1.0f - c.fy, az = 1.0f - c.fz;
    dW[0] = c.gx * (((v[1] - v[0]) * ay + (v[3] - v[2]) * c.fy) * az + ((v[5] - v[4]) * ay + (v[7] - v[6]) * c.fy) * c.fz);
    dW[1] = c.gy * (((v[2] - v[0]) * ax + (v[3] - v[1]) * c.fx) * az + ((v[6] - v[4]) * ax + (v[7] - v[5]) * c.fx) * c.fz);
    dW[2] = c.gz * (((v[4] - v[0]) * ax + (v[5] - v[1]) * c.fx) * ay + ((v[6] - v[2]) * ax + (v[7] - v[3]) * c.fx) * c.fy);
  }
  return s;
}

// ---- the point --------------------------------------------------------------------------------------------------------------------
// pytorch3d's matrix_to_quaternion of T's 3x3 part (T: 3x4).  Returns the branch; c: the chosen candidate before the division,
// *s its q_abs, *den = 2 max(s, 0.1), *sign the flip to w >= 0.
BDS_HD int smpl_matrix_to_quat(const float *T, float *q, float *c, float *s, float *den, float *sign) {
  const float m00 = T[0], m01 = T[1], m02 = T[2], m10 = T[4], m11 = T[5], m12 = T[6], m20 = T[8], m21 = T[9], m22 = T[10];
  const float t0 = 1.0f + m00 + m11 + m22, t1 = 1.0f + m00 - m11 - m22, t2 = 1.0f - m00 + m11 - m22, t3 = 1.0f - m00 - m11 + m22;
  const float a0 = t0 > 0.0f ? sqrtf(t0) : 0.0f, a1 = t1 > 0.0f ? sqrtf(t1) : 0.0f, a2 = t2 > 0.0f ? sqrtf(t2) : 0.0f,
              a3 = t3 > 0.0f ? sqrtf(t3) : 0.0f;
  int b = 0;
  float a = a0;
  if (a1 > a) { a = a1; b = 1; }
  if (a2 > a) { a = a2; b = 2; }
  if (a3 > a) { a = a3; b = 3; }
  switch (b) {
    case 0: c[0] = a * a; c[1] = m21 - m12; c[2] = m02 - m20; c[3] = m10 - m01; break;
    case 1: c[0] = m21 - m12; c[1] = a * a; c[2] = m10 + m01; c[3] = m02 + m20; break;
    case 2: c[0] = m02 - m20; c[1] = m10 + m01; c[2] = a * a; c[3] = m12 + m21; break;
    default: c[0] = m10 - m01; c[1] = m20 + m02; c[2] = m21 + m12; c[3] = a * a; break;
  }
  *s = a;
  *den = 2.0f * fmaxf(a, 0.1f);
  *sign = c[0] / *den < 0.0f ? -1.0f : 1.0f;
  for (int k = 0; k < 4; k++) q[k] = *sign * (c[k] / *den);
  return b;
}

// the chosen branch's gradient: vq -> vR [9] (row-major 3x3); the clamps' subgradients are zero where they are active
BDS_HD void smpl_matrix_to_quat_vjp(int b, const float *c, float s, float den, float sign, const float *vq, float *vR) {
  float vc[4];
  float dot = 0.0f;
  for (int k = 0; k < 4; k++) {
    vc[k] = sign * vq[k] / den;
    dot += sign * vq[k] * c[k];
  }
  const float vden = -dot / (den * den);
  const float vdiag = b == 0 ? vc[0] : (b == 1 ? vc[1] : (b == 2 ? vc[2] : vc[3]));
  const float vs = vdiag * 2.0f * s + (s >= 0.1f ? 2.0f * vden : 0.0f);
  const float vt = s > 0.0f ? vs / (2.0f * s) : 0.0f;
  float v00, v01, v02, v10, v11, v12, v20, v21, v22;
  switch (b) {
    case 0: v00 = vt; v11 = vt; v22 = vt; v21 = vc[1]; v12 = -vc[1]; v02 = vc[2]; v20 = -vc[2]; v10 = vc[3]; v01 = -vc[3]; break;
    case 1: v00 = vt; v11 = -vt; v22 = -vt; v21 = vc[0]; v12 = -vc[0]; v10 = vc[2]; v01 = vc[2]; v02 = vc[3]; v20 = vc[3]; break;
    case 2: v00 = -vt; v11 = vt; v22 = -vt; v02 = vc[0]; v20 = -vc[0]; v10 = vc[1]; v01 = vc[1]; v12 = vc[3]; v21 = vc[3]; break;
    default: v00 = -vt; v11 = -vt; v22 = vt; v10 = vc[0]; v01 = -vc[0]; v20 = vc[1]; v02 = vc[1]; v21 = vc[2]; v12 = vc[2]; break;
  }
  vR[0] = v00; vR[1] = v01; vR[2] = v02; vR[3] = v10; vR[4] = v11; vR[5] = v12; vR[6] = v20; vR[7] = v21; vR[8] = v22;
}

// Forward of one point of a present instance.  ball: the means only (q is not read, wq not written).
BDS_HD void smpl_point_fwd(const float *T, const float *x, const float *trans, const float *q, bool ball, float *wm, float *wq) {
  for (int r = 0; r < 3; r++) wm[r] = T[r * 4] * x[0] + T[r * 4 + 1] * x[1] + T[r * 4 + 2] * x[2] + T[r * 4 + 3] + trans[r];
  if (ball) return;
  float rq[4], c[4], s, den, sign, a[4], b[4];
  smpl_matrix_to_quat(T, rq, c, &s, &den, &sign);
  np_normalize(rq, a);
  np_normalize(q, b);
  np_quat_mult(a, b, wq);
}

// Backward of one point of a present instance: vT [12] (the gradient of the blended transform), vx [3] = T.R^T v_wm (the direct term of
// the mean's gradient) and vq [4].  ball: q / v_wq are not read and vq is not written.
BDS_HD void smpl_point_bwd(const float *T, const float *x, const float *q, const float *v_wm, const float *v_wq, bool ball, float *vT,
                           float *vx, float *vq) {
  for (int c = 0; c < 3; c++) vx[c] = T[c] * v_wm[0] + T[4 + c] * v_wm[1] + T[8 + c] * v_wm[2];
  float vR[9];
  for (int k = 0; k < 9; k++) vR[k] = 0.0f;
  if (!ball) {
    float rq[4], c[4], s, den, sign, a[4], b[4], va[4], vb[4], vrq[4];
    const int br = smpl_matrix_to_quat(T, rq, c, &s, &den, &sign);
    const float ia = np_normalize(rq, a);
    const float ib = np_normalize(q, b);
    np_quat_mult_vjp(a, b, v_wq, va, vb);
    np_normalize_vjp(b, ib, vb, vq);
    np_normalize_vjp(a, ia, va, vrq);
    smpl_matrix_to_quat_vjp(br, c, s, den, sign, vrq, vR);
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) vT[r * 4 + c] = v_wm[r] * x[c] + vR[r * 3 + c];
    vT[r * 4 + 3] = v_wm[r];
  }
}

BDS_HD float smpl_dot12(const float *a, const float *b) {
  float s = 0.0f;
  for (int k = 0; k < kSmplAff; k++) s += a[k] * b[k];
  return s;
}

}  // namespace bds
