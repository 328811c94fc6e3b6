// The SMPL nodes' two every-step regularisers (SMPLNodes.compute_reg_loss, models/nodes/smpl.py:448-503; include/bds.h
// bds_smpl_knn_reg_* and bds_voxel_reg_*); the per-element formulas are csrc/smpl_reg_math.h.
//
// kNN term.  One thread per (row, channel) over the channels of every live attribute group side by side, so the lanes of a point read
// consecutive floats of the same neighbour rows.  Forward: one launch (at most kRegMaxBlocks workgroups, striding the work) writes mean
// and 1 / ((K-1) std) per (point, channel) and one row of five sums per workgroup; a one-workgroup finish adds the rows in a fixed order, counts the present instances and leaves the
// five means and their 1 / count for the backward.  Backward: one launch in gather form -- a row walks the (point, slot) pairs that
// list it (the reverse adjacency, ascending) and adds (a - mean) rstd in that order; absent instances' and unlisted rows get zeros.
// No atomics: both directions are bit-identical run to run.
//
// Field term.  One thread per voxel of [I,D,H,W], consecutive along W, walking the J channels: the element and its +1 neighbours along
// W, H and D (the same lines other lanes and workgroups load: cache) give the three difference sums and the sum of squares in one
// pass.  The forward leaves 1 / |x|_J per voxel (1 / J of the field's bytes), so the backward reads the field once and writes the
// gradient once.  Per-workgroup rows and a fixed-order finish as above.
#include "bds_common.h"
#include "smpl_reg_math.h"

namespace bds {

constexpr int kRegBlock = 256;
constexpr int kRegWaves = kRegBlock / kWave;
constexpr int kRegMaxBlocks = 2048;   // 8 workgroups of 4 waves per CU on 256 CUs

struct KnnRegArgs {
  int I, V, K, ctot;
  const int32_t *nn;            // [I,V,K]
  const uint8_t *present;       // [I]
  const float *attr[kKnnRegGroups];
  int width[kKnnRegGroups];     // 0: frozen
  int start[kKnnRegGroups];     // first channel of the group among the ctot live ones
};
struct KnnRegGrads {
  float *v[kKnnRegGroups];
};

// the group of live channel c: its attribute pointer, width, first channel (unrolled selects: nothing is indexed by a lane's value)
struct KnnRegSel {
  const float *attr;
  int group, width, start;
};
__device__ __forceinline__ KnnRegSel knn_reg_select(const KnnRegArgs &a, int c) {
  KnnRegSel s{nullptr, 0, 1, 0};
#pragma unroll
  for (int g = 0; g < kKnnRegGroups; g++)
    if (a.width[g] > 0 && c >= a.start[g]) s = KnnRegSel{a.attr[g], g, a.width[g], a.start[g]};
  return s;
}

// NV sums of the workgroup into out[0..NV): waves by the xor butterfly, then the waves in order
template <int NV>
__device__ __forceinline__ void block_row(const float (&v)[NV], float *__restrict__ out) {
  __shared__ float red[kRegWaves][NV];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int n = 0; n < NV; n++) {
    const float s = wave_sum_all(v[n]);
    if (lane == 0) red[wave][n] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRegWaves; w++) s += red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// column `col` of the rows [0, rows) of a [rows, NV] table: lanes stride the rows with four independent partial sums (so the loads of
// four rows are in flight at once), added in a fixed order, then the butterfly (the total in every lane)
__device__ __forceinline__ float column_sum(const float *__restrict__ table, int64_t rows, int nv, int col, int lane) {
  float s[4] = {};
  for (int64_t b = lane; b < rows; b += 4 * kWave) {
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (b + u * kWave < rows) s[u] += table[(b + u * kWave) * nv + col];
  }
  return wave_sum_all((s[0] + s[1]) + (s[2] + s[3]));
}

// workgroups of a forward launch over `items` threads' worth of work: at most kRegMaxBlocks, each thread striding the grid, so the
// finish reads a bounded number of rows
static inline int64_t reg_blocks(int64_t items) {
  const int64_t b = cdiv(items, kRegBlock);
  return b < kRegMaxBlocks ? b : kRegMaxBlocks;
}

__global__ void __launch_bounds__(kRegBlock) smpl_knn_reg_fwd_kernel(KnnRegArgs a, float *__restrict__ mean, float *__restrict__ rstd,
                                                                     float *__restrict__ partials) {
  const int64_t total = (int64_t)a.I * a.V * a.ctot;
  float sums[kKnnRegGroups] = {};
  for (int64_t t = (int64_t)blockIdx.x * kRegBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kRegBlock) {
    const int64_t row = t / a.ctot;
    const int c = (int)(t - row * a.ctot);
    const int i = (int)(row / a.V);
    if (a.present[i]) {
      const KnnRegSel s = knn_reg_select(a, c);
      float m, r;
      const float sd = knn_reg_std(s.attr + (int64_t)i * a.V * s.width + (c - s.start), s.width, a.nn + row * a.K, a.K, a.V,
                                   knn_reg_act_of(s.group), &m, &r);
      mean[t] = m;
      rstd[t] = r;
#pragma unroll
      for (int g = 0; g < kKnnRegGroups; g++) sums[g] += s.group == g ? sd : 0.0f;
    }
  }
  block_row<kKnnRegGroups>(sums, partials + (int64_t)blockIdx.x * kKnnRegGroups);
}

// one workgroup of kKnnRegGroups waves: wave g owns group g
__global__ void __launch_bounds__(kKnnRegGroups *kWave) smpl_knn_reg_finish_kernel(KnnRegArgs a, const float *__restrict__ partials,
                                                                                   int64_t blocks, float *__restrict__ terms,
                                                                                   float *__restrict__ norm) {
  const int lane = threadIdx.x & (kWave - 1), g = threadIdx.x / kWave;
  const float s = column_sum(partials, blocks, kKnnRegGroups, g, lane);
  int n = 0;
  for (int i = lane; i < a.I; i += kWave) n += a.present[i] ? 1 : 0;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if (lane == 0) {
    int width = 0;
#pragma unroll
    for (int k = 0; k < kKnnRegGroups; k++) width = g == k ? a.width[k] : width;
    const float count = (float)((int64_t)n * a.V * width);
    const bool live = n > 0 && width > 0;
    terms[g] = live ? s / count : 0.0f;
    norm[g] = live ? 1.0f / count : 0.0f;
  }
}

__global__ void __launch_bounds__(kRegBlock) smpl_knn_reg_bwd_kernel(KnnRegArgs a, const int32_t *__restrict__ offsets,
                                                                     const int32_t *__restrict__ edges, const float *__restrict__ mean,
                                                                     const float *__restrict__ rstd, const float *__restrict__ norm,
                                                                     const float *__restrict__ v_terms, KnnRegGrads out) {
  const int64_t total = (int64_t)a.I * a.V * a.ctot;
  const int64_t t = (int64_t)blockIdx.x * kRegBlock + threadIdx.x;
  if (t >= total) return;
  const int64_t row = t / a.ctot;
  const int c = (int)(t - row * a.ctot);
  const int i = (int)(row / a.V), p = (int)(row - (int64_t)i * a.V);
  const KnnRegSel s = knn_reg_select(a, c);
  float *dst = nullptr;
#pragma unroll
  for (int g = 0; g < kKnnRegGroups; g++) dst = s.group == g ? out.v[g] : dst;
  const int64_t at = row * s.width + (c - s.start);
  float grad = 0.0f;
  if (a.present[i]) {
    const int act = knn_reg_act_of(s.group);
    const float av = knn_reg_act(s.attr[at], act);
    const int VK = a.V * a.K;
    int e0 = offsets[(int64_t)i * (a.V + 1) + p], e1 = offsets[(int64_t)i * (a.V + 1) + p + 1];
    e0 = min(max(e0, 0), VK);                       // (built by reverse_lists; kept inside the instance's list whatever they hold)
    e1 = min(max(e1, e0), VK);
    const int64_t first = (int64_t)i * a.V * a.ctot + c;
    const float gsum = knn_reg_row_grad(av, edges + (int64_t)i * VK + e0, e1 - e0, a.K, a.V, mean + first, rstd + first, a.ctot);
    float w = 0.0f;
#pragma unroll
    for (int g = 0; g < kKnnRegGroups; g++) w = s.group == g ? v_terms[g] * norm[g] : w;
    grad = w * gsum * knn_reg_act_grad(av, act);
  }
  dst[at] = grad;
}

struct VoxRegDims {
  int I, J, D, H, W;
};

__global__ void __launch_bounds__(kRegBlock) voxel_reg_fwd_kernel(VoxRegDims n, const float *__restrict__ x, float *__restrict__ rnorm,
                                                                  float *__restrict__ partials) {
  const int64_t HW = (int64_t)n.H * n.W, DHW = HW * n.D;
  float sums[4] = {};   // |d/dD|, |d/dH|, |d/dW|, norm
  for (int64_t t = (int64_t)blockIdx.x * kRegBlock + threadIdx.x; t < DHW * n.I; t += (int64_t)gridDim.x * kRegBlock) {
    const int64_t i = t / DHW, s = t - i * DHW;
    const int d = (int)(s / HW), h = (int)((s - d * HW) / n.W), w = (int)(s - d * HW - (int64_t)h * n.W);
    const float *p = x + i * n.J * DHW + s;
    float sq = 0.0f;
    for (int j = 0; j < n.J; j++, p += DHW) {
      const float v = p[0];
      sq += v * v;
      if (d + 1 < n.D) sums[0] += fabsf(p[HW] - v);
      if (h + 1 < n.H) sums[1] += fabsf(p[n.W] - v);
      if (w + 1 < n.W) sums[2] += fabsf(p[1] - v);
    }
    float nrm;
    rnorm[t] = vox_reg_rnorm(sq, &nrm);
    sums[3] += nrm;
  }
  block_row<4>(sums, partials + (int64_t)blockIdx.x * 4);
}

__global__ void __launch_bounds__(4 * kWave) voxel_reg_finish_kernel(VoxRegDims n, const float *__restrict__ partials, int64_t blocks,
                                                                     float *__restrict__ terms) {
  __shared__ float tot[4];
  const int lane = threadIdx.x & (kWave - 1), k = threadIdx.x / kWave;
  const float s = column_sum(partials, blocks, 4, k, lane);
  if (lane == 0) tot[k] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float B = (float)n.I * (float)n.J;
    const float nd = B * (float)((int64_t)(n.D - 1) * n.H * n.W), nh = B * (float)((int64_t)n.D * (n.H - 1) * n.W),
                nw = B * (float)((int64_t)n.D * n.H * (n.W - 1));
    terms[0] = (tot[0] / nd + tot[1] / nh + tot[2] / nw) / 3.0f;
    terms[1] = tot[3] / ((float)n.I * (float)((int64_t)n.D * n.H * n.W));
  }
}

__global__ void __launch_bounds__(kRegBlock) voxel_reg_bwd_kernel(VoxRegDims n, const float *__restrict__ x, const float *__restrict__ rnorm,
                                                                  const float *__restrict__ v_terms, float *__restrict__ v_x) {
  const int64_t HW = (int64_t)n.H * n.W, DHW = HW * n.D;
  const int64_t t = (int64_t)blockIdx.x * kRegBlock + threadIdx.x;
  if (t >= DHW * n.I) return;
  const int64_t i = t / DHW, s = t - i * DHW;
  const int d = (int)(s / HW), h = (int)((s - d * HW) / n.W), w = (int)(s - d * HW - (int64_t)h * n.W);
  const float B = (float)n.I * (float)n.J, vtv = v_terms[0] / 3.0f;
  const float wd = vtv / (B * (float)((int64_t)(n.D - 1) * n.H * n.W)), wh = vtv / (B * (float)((int64_t)n.D * (n.H - 1) * n.W)),
              ww = vtv / (B * (float)((int64_t)n.D * n.H * (n.W - 1)));
  const float wmag = v_terms[1] / ((float)n.I * (float)DHW), rn = rnorm[t];
  const bool dl = d > 0, dh = d + 1 < n.D, hl = h > 0, hh = h + 1 < n.H, wl = w > 0, wh_ = w + 1 < n.W;
  const int64_t at = i * n.J * DHW + s;
  const float *p = x + at;
  float *o = v_x + at;
  for (int j = 0; j < n.J; j++, p += DHW, o += DHW) {
    const float v = p[0];
    o[0] = vox_reg_grad(v, dl ? p[-HW] : 0.0f, dh ? p[HW] : 0.0f, hl ? p[-n.W] : 0.0f, hh ? p[n.W] : 0.0f, wl ? p[-1] : 0.0f,
                        wh_ ? p[1] : 0.0f, dl, dh, hl, hh, wl, wh_, wd, wh, ww, wmag, rn);
  }
}

static int knn_reg_args(int I, int V, int K, const int32_t *nn, const uint8_t *present, const float *dc, const float *rest, int c_rest,
                        const float *opacities, const float *scales, int s_dim, const float *quats, bool need_nn, KnnRegArgs *a) {
  BDS_REQUIRE(I >= 1 && V >= 1 && K >= 2 && K <= kKnnRegMaxK && present);
  BDS_REQUIRE(!rest || c_rest == 9 || c_rest == 24 || c_rest == 45);
  BDS_REQUIRE(!scales || s_dim == 1 || s_dim == 3);
  *a = KnnRegArgs{I, V, K, 0, nn, present, {dc, rest, opacities, scales, quats}, {dc ? 3 : 0, rest ? c_rest : 0, opacities ? 1 : 0,
                  scales ? s_dim : 0, quats ? 4 : 0}, {}};
  for (int g = 0; g < kKnnRegGroups; g++) {
    a->start[g] = a->ctot;
    a->ctot += a->width[g];
  }
  BDS_REQUIRE(a->ctot == 0 || nn || !need_nn);
  BDS_REQUIRE((int64_t)V * K < ((int64_t)1 << 31) && (int64_t)I * V * (a->ctot > 0 ? a->ctot : 1) < ((int64_t)1 << 31));
  return BDS_OK;
}

static bool vox_reg_dims(int I, int J, int D, int H, int W, VoxRegDims *n) {
  *n = VoxRegDims{I, J, D, H, W};
  return I >= 1 && I <= 1 << 16 && J >= 1 && J <= kVoxRegMaxJ && D >= 2 && H >= 2 && W >= 2 && D <= 4096 && H <= 4096 && W <= 4096 &&
         (int64_t)I * J * D * H * W <= ((int64_t)1 << 33);
}

}  // namespace bds

using namespace bds;

extern "C" size_t bds_smpl_knn_reg_temp_bytes(int I, int V, int channels) {
  if (I < 1 || V < 1 || channels < 1) return 0;
  return (size_t)cdiv((int64_t)I * V * channels, kRegBlock) * kKnnRegGroups * sizeof(float);
}

extern "C" int bds_smpl_knn_reg_fwd(int I, int V, int K, const int32_t *nn_ind, const uint8_t *present, const float *features_dc,
                                    const float *features_rest, int c_rest, const float *opacities, const float *scales, int s_dim,
                                    const float *quats, float *terms, float *norm, float *mean, float *rstd, void *temp, size_t temp_bytes,
                                    bds_stream_t stream) {
  KnnRegArgs a;
  const int rc = knn_reg_args(I, V, K, nn_ind, present, features_dc, features_rest, c_rest, opacities, scales, s_dim, quats, true, &a);
  if (rc != BDS_OK) return rc;
  BDS_REQUIRE(terms && norm);
  int64_t blocks = 0;
  if (a.ctot > 0) {
    BDS_REQUIRE(mean && rstd && temp && temp_bytes >= bds_smpl_knn_reg_temp_bytes(I, V, a.ctot));
    blocks = reg_blocks((int64_t)I * V * a.ctot);
    hipLaunchKernelGGL(smpl_knn_reg_fwd_kernel, dim3((unsigned)blocks), dim3(kRegBlock), 0, as_stream(stream), a, mean, rstd,
                       static_cast<float *>(temp));
    BDS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(smpl_knn_reg_finish_kernel, dim3(1), dim3(kKnnRegGroups * kWave), 0, as_stream(stream), a, (const float *)temp, blocks,
                     terms, norm);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_smpl_knn_reg_bwd(int I, int V, int K, const int32_t *rev_offsets, const int32_t *rev_edges, const uint8_t *present,
                                    const float *features_dc, const float *features_rest, int c_rest, const float *opacities,
                                    const float *scales, int s_dim, const float *quats, const float *mean, const float *rstd,
                                    const float *norm, const float *v_terms, float *v_features_dc, float *v_features_rest, float *v_opacities,
                                    float *v_scales, float *v_quats, bds_stream_t stream) {
  KnnRegArgs a;
  const int rc = knn_reg_args(I, V, K, nullptr, present, features_dc, features_rest, c_rest, opacities, scales, s_dim, quats, false, &a);
  if (rc != BDS_OK) return rc;
  const KnnRegGrads out{{v_features_dc, v_features_rest, v_opacities, v_scales, v_quats}};
  for (int g = 0; g < kKnnRegGroups; g++) BDS_REQUIRE((a.attr[g] == nullptr) == (out.v[g] == nullptr));
  if (a.ctot == 0) return BDS_OK;
  BDS_REQUIRE(rev_offsets && rev_edges && mean && rstd && norm && v_terms);
  hipLaunchKernelGGL(smpl_knn_reg_bwd_kernel, dim3((unsigned)cdiv((int64_t)I * V * a.ctot, kRegBlock)), dim3(kRegBlock), 0, as_stream(stream),
                     a, rev_offsets, rev_edges, mean, rstd, norm, v_terms, out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" size_t bds_voxel_reg_temp_bytes(int I, int D, int H, int W) {
  if (I < 1 || D < 1 || H < 1 || W < 1) return 0;
  return (size_t)cdiv((int64_t)I * D * H * W, kRegBlock) * 4 * sizeof(float);
}

extern "C" int bds_voxel_reg_fwd(int I, int J, int D, int H, int W, const float *field, float *terms, float *rnorm, void *temp,
                                 size_t temp_bytes, bds_stream_t stream) {
  VoxRegDims n;
  BDS_REQUIRE(vox_reg_dims(I, J, D, H, W, &n));
  BDS_REQUIRE(field && terms && rnorm && temp && temp_bytes >= bds_voxel_reg_temp_bytes(I, D, H, W));
  const int64_t blocks = reg_blocks((int64_t)I * D * H * W);
  hipLaunchKernelGGL(voxel_reg_fwd_kernel, dim3((unsigned)blocks), dim3(kRegBlock), 0, as_stream(stream), n, field, rnorm,
                     static_cast<float *>(temp));
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(voxel_reg_finish_kernel, dim3(1), dim3(4 * kWave), 0, as_stream(stream), n, (const float *)temp, blocks, terms);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_voxel_reg_bwd(int I, int J, int D, int H, int W, const float *field, const float *rnorm, const float *v_terms,
                                 float *v_field, bds_stream_t stream) {
  VoxRegDims n;
  BDS_REQUIRE(vox_reg_dims(I, J, D, H, W, &n));
  BDS_REQUIRE(field && rnorm && v_terms && v_field);
  hipLaunchKernelGGL(voxel_reg_bwd_kernel, dim3((unsigned)cdiv((int64_t)I * D * H * W, kRegBlock)), dim3(kRegBlock), 0, as_stream(stream), n,
                     field, rnorm, v_terms, v_field);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
