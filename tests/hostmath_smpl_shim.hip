// TEST-ONLY host shim of the SMPL nodes' pose chain and skinning (csrc/smpl_math.h, the functions the kernels of csrc/smpl.hip run) on
// the CPU, so that tests/test_smpl_skin_cpu.py can compare them with float64 autograd without a GPU.  Not part of libbds.so, never
// loaded by the product.  The loops follow the kernels: per instance the chain, per point the joints streamed twice in the backward;
// the sums the kernels form per workgroup and with atomics are plain float additions in point order here.
#include <vector>

#include "../bilateral_driving_amd/csrc/smpl_math.h"

using namespace bds;

namespace {

struct Tmpl {
  int I, V, d, h, w, ratio_dim;
  float ratio;
  SmplParents par;
  const float *root, *body, *J, *A0, *base, *corr, *W, *offset, *scale;
};

bool pack(const int32_t *parents, SmplParents *out) {
  out->lo = out->hi = 0;
  for (int j = 1; j < kSmplJoints; j++) {
    if (parents[j] < 0 || parents[j] >= j) return false;
    (j < 12 ? out->lo : out->hi) |= (uint64_t)parents[j] << (5 * (j < 12 ? j : j - 12));
  }
  return true;
}

const float *joint_quat(const Tmpl &t, int i, int j) { return j == 0 ? t.root + i * 4 : t.body + (i * (kSmplJoints - 1) + (j - 1)) * 4; }

void chain(const Tmpl &t, int i, float *M, float *G) {
  const float *J = t.J + i * kSmplJoints * 3;
  for (int j = 0; j < kSmplJoints; j++)
    smpl_joint_local(joint_quat(t, i, j), J + j * 3, j ? J + smpl_parent(t.par, j) * 3 : nullptr, M + j * kSmplAff);
  for (int k = 0; k < kSmplAff; k++) G[k] = M[k];
  for (int j = 1; j < kSmplJoints; j++) smpl_affine_mul(G + smpl_parent(t.par, j) * kSmplAff, M + j * kSmplAff, G + j * kSmplAff);
}

float weight(const Tmpl &t, int i, int p, int j, const SmplCell &c, float *dW) {
  if (!t.base) return t.W[((int64_t)i * t.V + p) * kSmplJoints + j];
  const int64_t slab = ((int64_t)i * kSmplJoints + j) * ((int64_t)t.d * t.h * t.w);
  return smpl_sample(t.base + slab, t.corr ? t.corr + slab : nullptr, c, t.h, t.w, dW);
}

SmplCell cell(const Tmpl &t, int i, const float *x) {
  if (!t.base) return SmplCell{};
  return smpl_cell(x, t.offset + i * 3, t.scale[i], t.ratio, t.ratio_dim, t.d, t.h, t.w);
}

}  // namespace

// wq NULL: the ball form.  Returns -1 for an invalid parent table.
extern "C" int hm_smpl_fwd(int I, int V, const float *means, const float *quats, const float *root, const float *body, const float *trans,
                           const uint8_t *present, const float *J, const float *A0, const int32_t *parents, const float *base,
                           const float *corr, const float *W, int d, int h, int w, const float *offset, const float *scale, float ratio,
                           int ratio_dim, float *wm, float *wq, float *A) {
  Tmpl t{I, V, d, h, w, ratio_dim, ratio, {}, root, body, J, A0, base, corr, W, offset, scale};
  if (!pack(parents, &t.par)) return -1;
  for (int i = 0; i < I; i++) {
    float *Ai = A + i * kSmplJoints * kSmplAff;
    if (!present[i]) {
      for (int k = 0; k < kSmplJoints * kSmplAff; k++) Ai[k] = 0.0f;
      for (int p = 0; p < V; p++) {
        const int64_t row = (int64_t)i * V + p;
        for (int k = 0; k < 3; k++) wm[row * 3 + k] = trans[i * 3 + k];
        if (wq)
          for (int k = 0; k < 4; k++) wq[row * 4 + k] = k == 0 ? 1.0f : 0.0f;
      }
      continue;
    }
    float M[kSmplJoints * kSmplAff], G[kSmplJoints * kSmplAff];
    chain(t, i, M, G);
    for (int j = 0; j < kSmplJoints; j++)
      smpl_joint_skin(G + j * kSmplAff, J + (i * kSmplJoints + j) * 3, A0 + (i * kSmplJoints + j) * 16, Ai + j * kSmplAff);
    for (int p = 0; p < V; p++) {
      const int64_t row = (int64_t)i * V + p;
      const float *x = means + row * 3;
      float T[kSmplAff] = {};
      const SmplCell c = cell(t, i, x);
      for (int j = 0; j < kSmplJoints; j++) {
        const float wj = weight(t, i, p, j, c, nullptr);
        for (int k = 0; k < kSmplAff; k++) T[k] += wj * Ai[j * kSmplAff + k];
      }
      float unit[4] = {1.0f, 0.0f, 0.0f, 0.0f}, oq[4];
      smpl_point_fwd(T, x, trans + i * 3, wq ? quats + row * 4 : unit, wq == nullptr, wm + row * 3, wq ? wq + row * 4 : oq);
    }
  }
  return 0;
}

extern "C" int hm_smpl_bwd(int I, int V, const float *means, const float *quats, const float *root, const float *body,
                           const uint8_t *present, const float *J, const float *A0, const int32_t *parents, const float *base,
                           const float *corr, const float *W, int d, int h, int w, const float *offset, const float *scale, float ratio,
                           int ratio_dim, const float *A, const float *v_wm, const float *v_wq, float *v_means, float *v_quats,
                           float *v_root, float *v_body, float *v_trans, float *v_corr) {
  Tmpl t{I, V, d, h, w, ratio_dim, ratio, {}, root, body, J, A0, base, corr, W, offset, scale};
  if (!pack(parents, &t.par)) return -1;
  const int64_t vol = (int64_t)d * h * w;
  if (v_corr)
    for (int64_t k = 0; k < (int64_t)I * kSmplJoints * vol; k++) v_corr[k] = 0.0f;
  for (int i = 0; i < I; i++) {
    const float *Ai = A + i * kSmplJoints * kSmplAff;
    float vA[kSmplJoints * kSmplAff] = {}, vt[3] = {};
    for (int p = 0; p < V; p++) {
      const int64_t row = (int64_t)i * V + p;
      const float *gm = v_wm + row * 3;
      float vx[3] = {}, vq[4] = {}, vT[kSmplAff] = {};
      for (int r = 0; r < 3; r++) vt[r] += gm[r];
      if (present[i]) {
        const float *x = means + row * 3;
        float T[kSmplAff] = {}, wj[kSmplJoints];
        const SmplCell c = cell(t, i, x);
        for (int j = 0; j < kSmplJoints; j++) {
          wj[j] = weight(t, i, p, j, c, nullptr);
          for (int k = 0; k < kSmplAff; k++) T[k] += wj[j] * Ai[j * kSmplAff + k];
        }
        float unit[4] = {1.0f, 0.0f, 0.0f, 0.0f}, zero[4] = {};
        smpl_point_bwd(T, x, v_wq ? quats + row * 4 : unit, gm, v_wq ? v_wq + row * 4 : zero, v_wq == nullptr, vT, vx, vq);
        for (int j = 0; j < kSmplJoints; j++) {
          for (int k = 0; k < kSmplAff; k++) vA[j * kSmplAff + k] += wj[j] * vT[k];
          if (!base) continue;
          const float vw = smpl_dot12(vT, Ai + j * kSmplAff);
          float dW[3];
          weight(t, i, p, j, c, dW);
          for (int k = 0; k < 3; k++) vx[k] += vw * dW[k];
          if (v_corr)
            for (int k = 0; k < 8; k++) v_corr[(i * kSmplJoints + j) * vol + smpl_corner_index(c, k, h, w)] += vw * smpl_corner_weight(c, k);
        }
      }
      for (int k = 0; k < 3; k++) v_means[row * 3 + k] = vx[k];
      if (v_quats)
        for (int k = 0; k < 4; k++) v_quats[row * 4 + k] = vq[k];
    }
    for (int k = 0; k < 3; k++) v_trans[i * 3 + k] = vt[k];
    float *vr = v_root + i * 4, *vb = v_body + i * (kSmplJoints - 1) * 4;
    if (!present[i]) {
      for (int k = 0; k < 4; k++) vr[k] = 0.0f;
      for (int k = 0; k < (kSmplJoints - 1) * 4; k++) vb[k] = 0.0f;
      continue;
    }
    float M[kSmplJoints * kSmplAff], G[kSmplJoints * kSmplAff], vG[kSmplJoints * kSmplAff], vR[kSmplJoints * 9];
    chain(t, i, M, G);
    for (int j = 0; j < kSmplJoints; j++)
      smpl_joint_skin_vjp(vA + j * kSmplAff, J + (i * kSmplJoints + j) * 3, A0 + (i * kSmplJoints + j) * 16, vG + j * kSmplAff);
    for (int j = kSmplJoints - 1; j >= 1; j--) {
      const int pj = smpl_parent(t.par, j);
      smpl_affine_mul_vjp(G + pj * kSmplAff, M + j * kSmplAff, vG + j * kSmplAff, vG + pj * kSmplAff, vR + j * 9);
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) vR[r * 3 + c] = vG[r * 4 + c];
    for (int j = 0; j < kSmplJoints; j++) smpl_joint_local_vjp(joint_quat(t, i, j), vR + j * 9, j == 0 ? vr : vb + (j - 1) * 4);
  }
  return 0;
}
