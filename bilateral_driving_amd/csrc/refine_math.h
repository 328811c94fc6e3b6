// Per-row math that every class's density control shares: what split_gaussians does to ANY class's parent and children
// (models/gaussians/vanilla.py:336-363, models/gaussians/pvg.py:298-354).  Used by csrc/refine.hip's geometry and decision kernels and,
// through csrc/pvg_math.h, by the host shim tests/hostmath_pvg_refine_shim.hip.  Every function keeps the reference's operations
// apart (no FMA contraction): the decisions compare float32 values, and the goldens pin the geometry's bits.
#pragma once
#include <math.h>
#include "gs_math.h"

namespace bds {

// log(exp(s) / size_fac) with size_fac = 1.6: the log-scale of a split parent and of its children (vanilla.py:358-359, pvg.py:322-323, :335)
BDS_HD float refine_shrink_log(float ls) {
#pragma clang fp contract(off)
  return logf(expf(ls) / 1.6f);
}

// rotation of a split sample (vanilla.py:343-348, pvg.py:310-311): R(quat_act(q)) with the F.normalize inside quat_to_rotmat, rows of R
BDS_HD void refine_split_rotation(const float *quat, float *R) {
#pragma clang fp contract(off)
  float q[4] = {quat[0], quat[1], quat[2], quat[3]};
  const float n1 = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n1;                                  // quat_act
  const float n2 = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n2;                                  // F.normalize
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - w * z); R[2] = 2.f * (x * z + w * y);
  R[3] = 2.f * (x * y + w * z); R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - w * x);
  R[6] = 2.f * (x * z - w * y); R[7] = 2.f * (y * z + w * x); R[8] = 1.f - 2.f * (x * x + y * y);
}

// mean of one split child: R (scale * noise) + mean, `scale` the parent's exp(log-scale) BEFORE the shrink (vanilla.py:343-348, pvg.py:305-313)
BDS_HD void refine_split_mean(const float *R, const float *scale, const float *noise, const float *mean, float *o_mean) {
#pragma clang fp contract(off)
  const float v[3] = {scale[0] * noise[0], scale[1] * noise[1], scale[2] * noise[2]};
  for (int i = 0; i < 3; i++) o_mean[i] = (R[i * 3] * v[0] + R[i * 3 + 1] * v[1] + R[i * 3 + 2] * v[2]) + mean[i];
}

}  // namespace bds
