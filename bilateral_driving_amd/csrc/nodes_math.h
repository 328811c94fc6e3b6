// Per-point math of the node classes' pose transform (models/nodes/rigid.py:385-493 transform_means / transform_quats /
// get_gaussians, shared by DeformableNodes, models/nodes/deformable.py:49-114), used by csrc/nodes.hip and by the host shim
// tests/hostmath_nodes_shim.hip.
//   world_means = R(q_i) m + t_i                                  (R: gsplat's normalising quat_to_rotmat of quat_act(q_i))
//   world_quats = n(quat_mult(n(q_i), n(q_p)))                    (n = quat_act = q / |q|; the outer n is get_gaussians' :471)
//   opacities   = sigmoid(logit) * instances_fv[f, i]
// The instance part of the backward is 16 floats per point, summed per instance before np_instance_chain:
//   [0..8] v_R = v_wm m^T (row-major) | [9..11] v_t = v_wm | [12..15] the gradient of n(q_i) through quat_mult.
#pragma once
#include <math.h>
#include "gs_math.h"

namespace bds {

constexpr int kNpSlab = 16;   // floats per instance and partial

// quat_mult (models/gaussians/basics.py:64-74), {w, x, y, z}
BDS_HD void np_quat_mult(const float *a, const float *b, float *o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// gradient of quat_mult's bilinear form: va = L(a)^T vo (into b's slot when called as (a, vo)), vb likewise
BDS_HD void np_quat_mult_vjp(const float *a, const float *b, const float *vo, float *va, float *vb) {
  va[0] = vo[0] * b[0] + vo[1] * b[1] + vo[2] * b[2] + vo[3] * b[3];
  va[1] = -vo[0] * b[1] + vo[1] * b[0] - vo[2] * b[3] + vo[3] * b[2];
  va[2] = -vo[0] * b[2] + vo[1] * b[3] + vo[2] * b[0] - vo[3] * b[1];
  va[3] = -vo[0] * b[3] - vo[1] * b[2] + vo[2] * b[1] + vo[3] * b[0];
  vb[0] = vo[0] * a[0] + vo[1] * a[1] + vo[2] * a[2] + vo[3] * a[3];
  vb[1] = -vo[0] * a[1] + vo[1] * a[0] + vo[2] * a[3] - vo[3] * a[2];
  vb[2] = -vo[0] * a[2] - vo[1] * a[3] + vo[2] * a[0] + vo[3] * a[1];
  vb[3] = -vo[0] * a[3] + vo[1] * a[2] - vo[2] * a[1] + vo[3] * a[0];
}

// q / |q| (a zero row gives NaN, as torch's x / x.norm()); returns 1 / |q|
BDS_HD float np_normalize(const float *q, float *o) {
  const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) o[k] = q[k] * inv;
  return inv;
}

// gradient of q / |q| at the unit result u = q / |q| (inv = 1 / |q|): (v - u (u . v)) / |q|
BDS_HD void np_normalize_vjp(const float *u, float inv, const float *v, float *vq) {
  const float d = u[0] * v[0] + u[1] * v[1] + u[2] * v[2] + u[3] * v[3];
  for (int k = 0; k < 4; k++) vq[k] = (v[k] - u[k] * d) * inv;
}

BDS_HD float np_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// interpolate_quats(q1, q2, 0.5) (models/gaussians/basics.py:17-45): slerp of the normalised rows, q2 negated when dot < 0, the
// lerp branch when dot > 0.9995.  The result is not normalised (the caller's quat_act / quat_to_rotmat does that).
BDS_HD void np_interp_quats(const float *q1r, const float *q2r, float *o) {
  float q1[4], q2[4];
  np_normalize(q1r, q1);
  np_normalize(q2r, q2);
  float dot = q1[0] * q2[0] + q1[1] * q2[1] + q1[2] * q2[2] + q1[3] * q2[3];
  dot = fminf(fmaxf(dot, -1.0f), 1.0f);
  if (dot < 0.0f) {
    for (int k = 0; k < 4; k++) q2[k] = -q2[k];
    dot = -dot;
  }
  if (dot > 0.9995f) {
    for (int k = 0; k < 4; k++) o[k] = q1[k] + 0.5f * (q2[k] - q1[k]);
    return;
  }
  const float th0 = acosf(dot), th = th0 * 0.5f;
  const float st = sinf(th), st0 = sinf(th0);
  const float s1 = cosf(th) - dot * st / st0, s2 = st / st0;
  for (int k = 0; k < 4; k++) o[k] = s1 * q1[k] + s2 * q2[k];
}

// Forward of one point.  qr / tr: the instance's rotation (raw; normalised inside quat_to_rotmat) and translation used for the means;
// qq: the instance's raw quaternion of frame f used for the world quaternion (differs from qr only in interpolated mode).
BDS_HD void np_forward(const float *qr, const float *tr, const float *qq, const float *m, const float *qp, float logit, float fv, float *wm,
                       float *wq, float *op) {
  const M3 R = quat_to_rotmat(qr[0], qr[1], qr[2], qr[3]);
  for (int r = 0; r < 3; r++) wm[r] = R.m[r * 3] * m[0] + R.m[r * 3 + 1] * m[1] + R.m[r * 3 + 2] * m[2] + tr[r];
  float a[4], b[4], c[4];
  np_normalize(qq, a);
  np_normalize(qp, b);
  np_quat_mult(a, b, c);
  np_normalize(c, wq);
  *op = np_sigmoid(logit) * fv;
}

// Backward of one point (non-interpolated: qr = qq = q, the instance's raw quaternion of frame f).  Writes the point's gradients
// v_m [3], v_qp [4], *v_logit and the instance contribution part[16] (layout at the top).
BDS_HD void np_backward(const float *q, const float *m, const float *qp, float logit, float fv, const float *v_wm, const float *v_wq,
                        float v_op, float *v_m, float *v_qp, float *v_logit, float *part) {
  const M3 R = quat_to_rotmat(q[0], q[1], q[2], q[3]);
  for (int c = 0; c < 3; c++) v_m[c] = R.m[c] * v_wm[0] + R.m[3 + c] * v_wm[1] + R.m[6 + c] * v_wm[2];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) part[r * 3 + c] = v_wm[r] * m[c];
  for (int r = 0; r < 3; r++) part[9 + r] = v_wm[r];
  float a[4], b[4], c[4], u[4], vc[4], va[4], vb[4];
  np_normalize(q, a);
  const float ib = np_normalize(qp, b);
  np_quat_mult(a, b, c);
  const float ic = np_normalize(c, u);
  np_normalize_vjp(u, ic, v_wq, vc);
  np_quat_mult_vjp(a, b, vc, va, vb);
  np_normalize_vjp(b, ib, vb, v_qp);
  for (int k = 0; k < 4; k++) part[12 + k] = va[k];
  const float s = np_sigmoid(logit);
  *v_logit = v_op * fv * s * (1.0f - s);
}

// Instance-level chain rule of the summed part[16]: v_q (raw quaternion of frame f) and v_t.
BDS_HD void np_instance_chain(const float *q, const float *part, float *v_q, float *v_t) {
  M3 vR;
  for (int k = 0; k < 9; k++) vR.m[k] = part[k];
  float g[4], a[4], gn[4];
  quat_to_rotmat_vjp(q[0], q[1], q[2], q[3], vR, g);
  const float inv = np_normalize(q, a);
  np_normalize_vjp(a, inv, part + 12, gn);
  for (int k = 0; k < 4; k++) v_q[k] = g[k] + gn[k];
  for (int r = 0; r < 3; r++) v_t[r] = part[9 + r];
}

}  // namespace bds
