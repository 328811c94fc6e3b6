// TEST-ONLY host shim of the SMPL nodes' kNN and skinning-field regularisers (csrc/smpl_reg_math.h, the functions the kernels of
// csrc/smpl_reg.hip run) on the CPU, so that tests/test_smpl_reg_cpu.py can compare them with float64 without a GPU.  Not part of
// libbds.so, never loaded by the product.  The loops follow the kernels: one (row, channel) at a time over the live groups' channels
// side by side; the sums the kernels form per workgroup and then over the workgroups' rows (64 lanes striding the rows, a butterfly)
// are formed in the same shape here (256 elements a row, in element order; the rows dealt to 64 partial sums, halved pairwise).
#include "../bilateral_driving_amd/csrc/smpl_reg_math.h"

using namespace bds;

namespace {

struct Sum {
  float row = 0.0f, lanes[64] = {};
  int n = 0, rows = 0;
  void flush() {
    lanes[rows++ % 64] += row;
    row = 0.0f;
    n = 0;
  }
  void add(float v) {
    row += v;
    if (++n == 256) flush();
  }
  float total() {
    if (n) flush();
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; l++) lanes[l] += lanes[l + o];
    return lanes[0];
  }
};

struct Groups {
  const float *attr[kKnnRegGroups];
  int width[kKnnRegGroups], start[kKnnRegGroups], ctot;
};

Groups groups(const float *dc, const float *rest, int c_rest, const float *opac, const float *scales, int s_dim, const float *quats) {
  Groups g{{dc, rest, opac, scales, quats}, {dc ? 3 : 0, rest ? c_rest : 0, opac ? 1 : 0, scales ? s_dim : 0, quats ? 4 : 0}, {}, 0};
  for (int k = 0; k < kKnnRegGroups; k++) {
    g.start[k] = g.ctot;
    g.ctot += g.width[k];
  }
  return g;
}

int group_of(const Groups &g, int c) {
  int at = 0;
  for (int k = 0; k < kKnnRegGroups; k++)
    if (g.width[k] > 0 && c >= g.start[k]) at = k;
  return at;
}

}  // namespace

// mean / rstd: [I V, ctot]; terms, norm: [5]
extern "C" void hm_knn_reg_fwd(int I, int V, int K, const int32_t *nn, const uint8_t *present, const float *dc, const float *rest, int c_rest,
                               const float *opac, const float *scales, int s_dim, const float *quats, float *terms, float *norm,
                               float *mean, float *rstd) {
  const Groups g = groups(dc, rest, c_rest, opac, scales, s_dim, quats);
  Sum sums[kKnnRegGroups];
  int n = 0;
  for (int i = 0; i < I; i++) n += present[i] ? 1 : 0;
  for (int64_t t = 0; t < (int64_t)I * V * g.ctot; t++) {
    const int64_t row = t / g.ctot;
    const int c = (int)(t - row * g.ctot), i = (int)(row / V);
    if (!present[i]) continue;
    const int k = group_of(g, c);
    sums[k].add(knn_reg_std(g.attr[k] + (int64_t)i * V * g.width[k] + (c - g.start[k]), g.width[k], nn + row * K, K, V, knn_reg_act_of(k),
                            mean + t, rstd + t));
  }
  for (int k = 0; k < kKnnRegGroups; k++) {
    const float count = (float)((int64_t)n * V * g.width[k]);
    const bool live = n > 0 && g.width[k] > 0;
    terms[k] = live ? sums[k].total() / count : 0.0f;
    norm[k] = live ? 1.0f / count : 0.0f;
  }
}

extern "C" void hm_knn_reg_bwd(int I, int V, int K, const int32_t *offsets, const int32_t *edges, const uint8_t *present, const float *dc,
                               const float *rest, int c_rest, const float *opac, const float *scales, int s_dim, const float *quats,
                               const float *mean, const float *rstd, const float *norm, const float *v_terms, float *v_dc, float *v_rest,
                               float *v_opac, float *v_scales, float *v_quats) {
  const Groups g = groups(dc, rest, c_rest, opac, scales, s_dim, quats);
  float *out[kKnnRegGroups] = {v_dc, v_rest, v_opac, v_scales, v_quats};
  for (int64_t t = 0; t < (int64_t)I * V * g.ctot; t++) {
    const int64_t row = t / g.ctot;
    const int c = (int)(t - row * g.ctot), i = (int)(row / V), p = (int)(row - (int64_t)i * V);
    const int k = group_of(g, c), act = knn_reg_act_of(k);
    const int64_t at = row * g.width[k] + (c - g.start[k]);
    float grad = 0.0f;
    if (present[i]) {
      const float av = knn_reg_act(g.attr[k][at], act);
      const int e0 = offsets[(int64_t)i * (V + 1) + p], e1 = offsets[(int64_t)i * (V + 1) + p + 1];
      const int64_t first = (int64_t)i * V * g.ctot + c;
      const float gsum = knn_reg_row_grad(av, edges + (int64_t)i * V * K + e0, e1 - e0, K, V, mean + first, rstd + first, g.ctot);
      grad = v_terms[k] * norm[k] * gsum * knn_reg_act_grad(av, act);
    }
    out[k][at] = grad;
  }
}

extern "C" void hm_voxel_reg_fwd(int I, int J, int D, int H, int W, const float *x, float *terms, float *rnorm) {
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  Sum sums[4];
  for (int64_t t = 0; t < DHW * I; t++) {
    const int64_t i = t / DHW, s = t - i * DHW;
    const int d = (int)(s / HW), h = (int)((s - d * HW) / W), w = (int)(s - d * HW - (int64_t)h * W);
    const float *p = x + i * J * DHW + s;
    float sq = 0.0f, nrm, tv[3] = {};
    for (int j = 0; j < J; j++, p += DHW) {
      sq += p[0] * p[0];
      if (d + 1 < D) tv[0] += fabsf(p[HW] - p[0]);
      if (h + 1 < H) tv[1] += fabsf(p[W] - p[0]);
      if (w + 1 < W) tv[2] += fabsf(p[1] - p[0]);
    }
    rnorm[t] = vox_reg_rnorm(sq, &nrm);
    for (int k = 0; k < 3; k++) sums[k].add(tv[k]);
    sums[3].add(nrm);
  }
  const float tot[4] = {sums[0].total(), sums[1].total(), sums[2].total(), sums[3].total()};
  const float B = (float)I * (float)J;
  terms[0] = (tot[0] / (B * (float)((int64_t)(D - 1) * H * W)) + tot[1] / (B * (float)((int64_t)D * (H - 1) * W)) +
              tot[2] / (B * (float)((int64_t)D * H * (W - 1)))) / 3.0f;
  terms[1] = tot[3] / ((float)I * (float)DHW);
}

extern "C" void hm_voxel_reg_bwd(int I, int J, int D, int H, int W, const float *x, const float *rnorm, const float *v_terms, float *v_x) {
  const int64_t HW = (int64_t)H * W, DHW = HW * D;
  const float B = (float)I * (float)J, vtv = v_terms[0] / 3.0f;
  const float wd = vtv / (B * (float)((int64_t)(D - 1) * H * W)), wh = vtv / (B * (float)((int64_t)D * (H - 1) * W)),
              ww = vtv / (B * (float)((int64_t)D * H * (W - 1))), wmag = v_terms[1] / ((float)I * (float)DHW);
  for (int64_t t = 0; t < DHW * I; t++) {
    const int64_t i = t / DHW, s = t - i * DHW;
    const int d = (int)(s / HW), h = (int)((s - d * HW) / W), w = (int)(s - d * HW - (int64_t)h * W);
    const bool dl = d > 0, dh = d + 1 < D, hl = h > 0, hh = h + 1 < H, wl = w > 0, wr = w + 1 < W;
    const float *p = x + i * J * DHW + s;
    float *o = v_x + i * J * DHW + s;
    for (int j = 0; j < J; j++, p += DHW, o += DHW)
      o[0] = vox_reg_grad(p[0], dl ? p[-HW] : 0.0f, dh ? p[HW] : 0.0f, hl ? p[-W] : 0.0f, hh ? p[W] : 0.0f, wl ? p[-1] : 0.0f, wr ? p[1] : 0.0f,
                          dl, dh, hl, hh, wl, wr, wd, wh, ww, wmag, rnorm[t]);
  }
}
