// Per-element math of the SMPL nodes' two every-step regularisers (SMPLNodes.compute_reg_loss, models/nodes/smpl.py:448-503), used by
// csrc/smpl_reg.hip and by the host shim tests/hostmath_smpl_reg_shim.hip.
//   knn_reg (:462-503): per attribute group, mean over (present instance, point, channel) of the unbiased std over the K gathered
//     neighbour values of that channel; opacities enter as sigmoid(raw), scales as exp(raw), dc / rest / quats raw.
//   voxel_deformer_reg (:448-459) with VoxelDeformer.get_tv / get_mag (models/modules.py:1139-1166): the mean absolute forward
//     difference of a field [I,J,D,H,W] along D, H and W, and the mean over [I,D,H,W] of the 2-norm over J.
// The std is formed in two passes: the mean as v_0 + sum(v_k - v_0) / K, then the squared deviations.  K bit-identical values have the
// mean v_0 and the deviations 0 exactly, so a constant neighbourhood has std 0 and (as torch's std_backward) gradient 0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef BDS_HD
#define BDS_HD __host__ __device__ __forceinline__
#endif

namespace bds {

constexpr int kKnnRegGroups = 5;                                  // dc, rest, opacity, scales, quats
enum KnnRegAct { kKnnRegRaw = 0, kKnnRegSigmoid = 1, kKnnRegExp = 2 };
constexpr int kKnnRegMaxK = 32;                                   // the neighbour search's cap
constexpr int kVoxRegMaxJ = 64;

BDS_HD int knn_reg_act_of(int group) { return group == 2 ? kKnnRegSigmoid : group == 3 ? kKnnRegExp : kKnnRegRaw; }

BDS_HD float knn_reg_act(float raw, int act) {
  if (act == kKnnRegSigmoid) return 1.0f / (1.0f + expf(-raw));
  if (act == kKnnRegExp) return expf(raw);
  return raw;
}

// d act / d raw from the ACTIVATED value
BDS_HD float knn_reg_act_grad(float a, int act) {
  if (act == kKnnRegSigmoid) return a * (1.0f - a);
  if (act == kKnnRegExp) return a;
  return 1.0f;
}

// A neighbour index as the kernels use it: validated by the caller (reverse_lists); an index outside [0, V) reads row 0, never memory
// outside the instance.
BDS_HD int knn_reg_index(int32_t idx, int V) { return (uint32_t)idx < (uint32_t)V ? idx : 0; }

// One (point, channel): col = the instance's first row at this channel, `width` floats between rows, nn_row = the point's K indices.
// Returns the unbiased std; *mean and *rstd = 1 / ((K - 1) std) (0 where std == 0) are what the backward needs:
//   d std / d v_k = (v_k - mean) rstd.
BDS_HD float knn_reg_std(const float *col, int width, const int32_t *nn_row, int K, int V, int act, float *mean, float *rstd) {
  const float v0 = knn_reg_act(col[(int64_t)knn_reg_index(nn_row[0], V) * width], act);
  float s = 0.0f;
  for (int k = 1; k < K; k++) s += knn_reg_act(col[(int64_t)knn_reg_index(nn_row[k], V) * width], act) - v0;
  const float m = v0 + s / (float)K;
  float ss = 0.0f;
  for (int k = 0; k < K; k++) {
    const float dv = knn_reg_act(col[(int64_t)knn_reg_index(nn_row[k], V) * width], act) - m;
    ss += dv * dv;
  }
  const float sd = sqrtf(ss / (float)(K - 1));
  *mean = m;
  *rstd = sd > 0.0f ? 1.0f / ((float)(K - 1) * sd) : 0.0f;
  return sd;
}

// One (row, channel) of the backward: the sum over the (point, slot) pairs that list the row, in the reverse list's (ascending) order.
// edges: `count` flat (point * K + slot) entries; mean / rstd: the instance's first row at this channel, `ctot` floats between rows.
BDS_HD float knn_reg_row_grad(float a, const int32_t *edges, int count, int K, int V, const float *mean, const float *rstd, int ctot) {
  float g = 0.0f;
  for (int e = 0; e < count; e++) {
    const int p = knn_reg_index(edges[e] / K, V);
    g += (a - mean[(int64_t)p * ctot]) * rstd[(int64_t)p * ctot];
  }
  return g;
}

BDS_HD float vox_reg_sign(float x) { return x > 0.0f ? 1.0f : x < 0.0f ? -1.0f : 0.0f; }

// 1 / |x| over J from the sum of squares; 0 for the zero vector (torch's norm backward masks it)
BDS_HD float vox_reg_rnorm(float sumsq, float *norm) {
  *norm = sqrtf(sumsq);
  return *norm > 0.0f ? 1.0f / *norm : 0.0f;
}

// gradient of one element: lo / hi = its neighbours at -1 / +1 along D, H, W (has_*: inside the field), wd / wh / ww = the upstream
// gradient of the TV term over (3 x that axis' difference count), wmag = the magnitude term's over the voxel count.
BDS_HD float vox_reg_grad(float x, float d_lo, float d_hi, float h_lo, float h_hi, float w_lo, float w_hi, bool has_d_lo, bool has_d_hi,
                          bool has_h_lo, bool has_h_hi, bool has_w_lo, bool has_w_hi, float wd, float wh, float ww, float wmag, float rnorm) {
  float g = wmag * (x * rnorm);
  g += wd * ((has_d_lo ? vox_reg_sign(x - d_lo) : 0.0f) - (has_d_hi ? vox_reg_sign(d_hi - x) : 0.0f));
  g += wh * ((has_h_lo ? vox_reg_sign(x - h_lo) : 0.0f) - (has_h_hi ? vox_reg_sign(h_hi - x) : 0.0f));
  g += ww * ((has_w_lo ? vox_reg_sign(x - w_lo) : 0.0f) - (has_w_hi ? vox_reg_sign(w_hi - x) : 0.0f));
  return g;
}

}  // namespace bds
