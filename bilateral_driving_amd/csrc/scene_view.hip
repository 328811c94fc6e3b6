// The scene view: one camera over SEVERAL Gaussian classes whose rows lie one behind the other in one global row range
// (models/trainers/base.py:355-366 concatenates every class's get_gaussians per key).  A class is a RAW segment -- its colours are SH
// coefficients held as the reference's two parameters, `_features_dc` [n,3] and `_features_rest` [n,K-1,3], evaluated at the class's
// own active degree (models/gaussians/vanilla.py:382-389) -- or a DENSE segment, which hands over post-activation colours [n,3].
// The projection, the tile stage and the compositors work on global row ids; the two kernels here are the list-driven ends that have
// to know the class of a row:
//   scene_pack_kernel   : splat records of the visible rows (layout and clearing arguments of bds_splat_pack_sh), the colour
//                         evaluated from the row's own segment -- never a concatenated coefficient array, never a culled row.
//   scene_sh_bwd_kernel : the SH backward into the raw segments' own gradient arrays + the activation chain of the raw rows behind
//                         the ACTIVATED projection backward (v_log_scale = v_scale * scale, v_logit = v_o * o (1 - o)).
// Both are streaming kernels, one list rank per lane.  The list is in depth order, so a wave's 64 ranks mix segments: the lookup
// is the branch-free compare chain of scene_math.h over starts held in scalar registers (the table is a kernel argument), and the
// segment loop below visits a segment only when a ballot finds one of its rows in the wave -- kind, K and degree are then
// wave-uniform scalars; a wave of one segment runs one body, a mixed wave runs one predicated body per segment present.
#include "bds_common.h"
#include "gs_math.h"
#include "scene_math.h"

namespace bds {

constexpr int kSceneBlock = 256;

// the record constants of csrc/rasterize.hip (records of 12 floats, gradient records of BDS_GRAD_RECORD_FLOATS, the binned
// schedule's header of 1 + 8 XCDs x 32 bins words): the scene pack writes what bds_splat_pack_sh writes
constexpr float kSceneLog2e = 1.4426950408889634f;
constexpr int kSceneGradStride = BDS_GRAD_RECORD_FLOATS;
constexpr int kSceneSchedHeader = 1 + 8 * 32;

struct SceneTable {
  SceneStarts st;
  int32_t rows[kSceneMaxSegments];
  int32_t kind[kSceneMaxSegments];   // BDS_SCENE_DENSE / BDS_SCENE_RAW
  int32_t K[kSceneMaxSegments];      // raw: SH bases stored per row (1 + rows of `_features_rest`)
  int32_t deg[kSceneMaxSegments];    // raw: active degree
  float *p0[kSceneMaxSegments];      // raw: band 0 [n,3] (forward: `_features_dc`, backward: its gradient) | dense forward: colours [n,3]
  float *p1[kSceneMaxSegments];      // raw: bands 1.. [n,K-1,3]
  int32_t n_seg;
};

// colour of one raw row: sum_k B[k] coeff[k], the bases in the order and the sums in the sequence of csrc/sh.hip
template <int DEG>
__device__ __forceinline__ void scene_sh_colour(const float *__restrict__ dc, const float *__restrict__ rest, float x, float y, float z,
                                                float &o0, float &o1, float &o2) {
  constexpr int nb = (DEG + 1) * (DEG + 1);
  float B[16];
  sh_bases(DEG, x, y, z, B);
  o0 = B[0] * dc[0];
  o1 = B[0] * dc[1];
  o2 = B[0] * dc[2];
#pragma unroll
  for (int k = 1; k < nb; k++) {
    o0 += B[k] * rest[(k - 1) * 3];
    o1 += B[k] * rest[(k - 1) * 3 + 1];
    o2 += B[k] * rest[(k - 1) * 3 + 2];
  }
}

// gradient rows of one raw row: v_coeff[k] = B[k] v_out for the active bands, zeros for the stored bands above them (the row is
// STORED whole, as bds_sh_view_bwd_list stores it)
template <int DEG>
__device__ __forceinline__ void scene_sh_colour_vjp(float *__restrict__ v_dc, float *__restrict__ v_rest, int K, float x, float y, float z,
                                                    float v0, float v1, float v2) {
  constexpr int nb = (DEG + 1) * (DEG + 1);
  float B[16];
  sh_bases(DEG, x, y, z, B);
  v_dc[0] = B[0] * v0;
  v_dc[1] = B[0] * v1;
  v_dc[2] = B[0] * v2;
#pragma unroll
  for (int k = 1; k < 16; k++) {
    if (k < K) {
      const float b = k < nb ? B[k < nb ? k : 0] : 0.f;
      v_rest[(k - 1) * 3] = b * v0;
      v_rest[(k - 1) * 3 + 1] = b * v1;
      v_rest[(k - 1) * 3 + 2] = b * v2;
    }
  }
}

__global__ __launch_bounds__(kSceneBlock) void scene_pack_kernel(
    int64_t n_cap, const uint64_t *__restrict__ n_dev, const int32_t *__restrict__ ids, const SceneTable t,
    const float *__restrict__ means, const float *__restrict__ cam_pos, const float *__restrict__ means2d,
    const float *__restrict__ conics, const float *__restrict__ depths, const float *__restrict__ opacities,
    const int32_t *__restrict__ radii, float4 *__restrict__ rec, float *__restrict__ sh_rgb_out, float4 *__restrict__ zero_rec,
    float4 *__restrict__ zero_tail, int zero_tail_f4, int32_t *__restrict__ schedule) {
  if (zero_tail && blockIdx.x == 0)   // (as splat_pack_kernel: the pose slots and the schedule header are cleared on the way)
    for (int i = threadIdx.x; i < zero_tail_f4; i += kSceneBlock) zero_tail[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (schedule && blockIdx.x == 0)
    for (int i = threadIdx.x; i < kSceneSchedHeader; i += kSceneBlock) schedule[i] = 0;
  const int64_t n = list_length(n_cap, n_dev);
  const int64_t r = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  const bool live = r < n;   // a rank at or beyond the list's length reads and writes nothing
  const int32_t g = live ? ids[r] : -1;
  const int seg = scene_segment(t.st, g);
  float u0 = 0.f, u1 = 0.f, u2 = 0.f;   // the un-clamped SH colour (raw rows)
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;   // the record's colour
  bool done = false;
  for (int s = 0; s < t.n_seg; s++) {   // (wave-uniform: the table entry of s is scalar)
    const int32_t local = g - t.st.start[s];
    const bool mine = live && seg == s && (uint32_t)local < (uint32_t)t.rows[s];   // the id inside its own segment's [0, n) only
    if (!__any(mine)) continue;
    if (mine) {
      done = true;
      if (t.kind[s] == BDS_SCENE_DENSE) {
        const float *c = t.p0[s] + (int64_t)local * 3;
        c0 = c[0]; c1 = c[1]; c2 = c[2];
      } else {
        const float x = means[(int64_t)g * 3] - cam_pos[0], y = means[(int64_t)g * 3 + 1] - cam_pos[1], z = means[(int64_t)g * 3 + 2] - cam_pos[2];
        const float inorm = 1.0f / sqrtf(x * x + y * y + z * z);
        const float *dc = t.p0[s] + (int64_t)local * 3;
        const float *rest = t.p1[s] + (int64_t)local * (t.K[s] - 1) * 3;
        switch (t.deg[s]) {
          case 0: scene_sh_colour<0>(dc, rest, x * inorm, y * inorm, z * inorm, u0, u1, u2); break;
          case 1: scene_sh_colour<1>(dc, rest, x * inorm, y * inorm, z * inorm, u0, u1, u2); break;
          case 2: scene_sh_colour<2>(dc, rest, x * inorm, y * inorm, z * inorm, u0, u1, u2); break;
          default: scene_sh_colour<3>(dc, rest, x * inorm, y * inorm, z * inorm, u0, u1, u2); break;
        }
        c0 = fminf(fmaxf(u0 + 0.5f, 0.f), 1.f);
        c1 = fminf(fmaxf(u1 + 0.5f, 0.f), 1.f);
        c2 = fminf(fmaxf(u2 + 0.5f, 0.f), 1.f);
      }
    }
  }
  if (!done) return;
  if (zero_rec) {
#pragma unroll
    for (int i = 0; i < kSceneGradStride / 4; i++) zero_rec[r * (kSceneGradStride / 4) + i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  sh_rgb_out[r * 3] = u0; sh_rgb_out[r * 3 + 1] = u1; sh_rgb_out[r * 3 + 2] = u2;   // (a dense row: zeros, never read back)
  const float2 xy = *reinterpret_cast<const float2 *>(means2d + (int64_t)g * 2);
  const float *cn = conics + (int64_t)g * 3;
  rec[r * 3] = make_float4(xy.x, xy.y, (-0.5f * kSceneLog2e) * cn[0], -kSceneLog2e * cn[1]);
  rec[r * 3 + 1] = make_float4((-0.5f * kSceneLog2e) * cn[2], opacities[g], c0, c1);
  rec[r * 3 + 2] = make_float4(c2, depths[g], 0.f, __int_as_float(radii[g]));
}

__global__ __launch_bounds__(kSceneBlock) void scene_sh_bwd_kernel(
    int64_t n_cap, const uint64_t *__restrict__ n_dev, const int32_t *__restrict__ ids, const SceneTable t,
    const float *__restrict__ means, const float *__restrict__ cam_pos, const float *__restrict__ sh_rgb,
    const float4 *__restrict__ v_rec, const float *__restrict__ scales, const float *__restrict__ opacities,
    float *__restrict__ v_scales, float *__restrict__ v_opacities) {
  const int64_t n = list_length(n_cap, n_dev);
  const int64_t r = (int64_t)blockIdx.x * kSceneBlock + threadIdx.x;
  const bool live = r < n;
  const int32_t g = live ? ids[r] : -1;
  const int seg = scene_segment(t.st, g);
  for (int s = 0; s < t.n_seg; s++) {
    if (t.kind[s] != BDS_SCENE_RAW) continue;   // (wave-uniform) dense rows keep the activated gradients and their colour gradient
    const int32_t local = g - t.st.start[s];
    const bool mine = live && seg == s && (uint32_t)local < (uint32_t)t.rows[s];
    if (!__any(mine)) continue;
    if (mine) {
      const float4 v = v_rec[r * (kSceneGradStride / 4)];
      float vo[3] = {v.x, v.y, v.z};
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float c = sh_rgb[r * 3 + k] + 0.5f;
        if (!(c >= 0.f && c <= 1.f)) vo[k] = 0.f;   // torch.clamp passes the gradient on the closed interval
      }
      const float x = means[(int64_t)g * 3] - cam_pos[0], y = means[(int64_t)g * 3 + 1] - cam_pos[1], z = means[(int64_t)g * 3 + 2] - cam_pos[2];
      const float inorm = 1.0f / sqrtf(x * x + y * y + z * z);
      const int K = t.K[s];
      float *v_dc = t.p0[s] + (int64_t)local * 3;
      float *v_rest = t.p1[s] + (int64_t)local * (K - 1) * 3;
      switch (t.deg[s]) {
        case 0: scene_sh_colour_vjp<0>(v_dc, v_rest, K, x * inorm, y * inorm, z * inorm, vo[0], vo[1], vo[2]); break;
        case 1: scene_sh_colour_vjp<1>(v_dc, v_rest, K, x * inorm, y * inorm, z * inorm, vo[0], vo[1], vo[2]); break;
        case 2: scene_sh_colour_vjp<2>(v_dc, v_rest, K, x * inorm, y * inorm, z * inorm, vo[0], vo[1], vo[2]); break;
        default: scene_sh_colour_vjp<3>(v_dc, v_rest, K, x * inorm, y * inorm, z * inorm, vo[0], vo[1], vo[2]); break;
      }
      // the activation chain behind the ACTIVATED projection backward (vanilla.py:393-394: exp, sigmoid)
#pragma unroll
      for (int i = 0; i < 3; i++) v_scales[(int64_t)g * 3 + i] = v_scales[(int64_t)g * 3 + i] * scales[(int64_t)g * 3 + i];
      const float o = opacities[g];
      v_opacities[g] = v_opacities[g] * o * (1.f - o);
    }
  }
}

// the table of a call; BDS_OK or why not
static int scene_table(int n_seg, const int64_t *seg_rows, const int *seg_kinds, const int *seg_K, const int *seg_degrees,
                       float *const *p0, float *const *p1, bool forward, SceneTable &t) {
  BDS_REQUIRE(seg_rows && seg_kinds && seg_K && seg_degrees && p0 && p1);
  BDS_REQUIRE(scene_starts_fill(n_seg, seg_rows, t.st, nullptr));
  t.n_seg = n_seg;
  for (int i = 0; i < kSceneMaxSegments; i++) {
    t.rows[i] = 0; t.kind[i] = BDS_SCENE_DENSE; t.K[i] = 1; t.deg[i] = 0; t.p0[i] = nullptr; t.p1[i] = nullptr;
    if (i >= n_seg) continue;
    t.rows[i] = (int32_t)seg_rows[i];
    t.kind[i] = seg_kinds[i];
    BDS_REQUIRE(t.kind[i] == BDS_SCENE_DENSE || t.kind[i] == BDS_SCENE_RAW);
    if (t.kind[i] == BDS_SCENE_RAW) {
      t.K[i] = seg_K[i];
      t.deg[i] = seg_degrees[i];
      BDS_REQUIRE(t.deg[i] >= 0 && t.deg[i] <= 3 && t.K[i] >= (t.deg[i] + 1) * (t.deg[i] + 1) && t.K[i] <= 16);
      BDS_REQUIRE(t.rows[i] == 0 || (p0[i] && (t.K[i] == 1 || p1[i])));
      t.p0[i] = p0[i];
      t.p1[i] = p1[i];
    } else if (forward) {
      BDS_REQUIRE(t.rows[i] == 0 || p0[i]);
      t.p0[i] = p0[i];
    }
  }
  return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_scene_pack(int64_t n, const uint64_t *n_dev, const int32_t *ids, int n_seg, const int64_t *seg_rows,
                              const int *seg_kinds, const int *seg_K, const int *seg_degrees, const float *const *seg_colors,
                              const float *const *seg_rest, const float *means, const float *cam_pos, const float *means2d,
                              const float *conics, const float *depths, const float *opacities, const int32_t *radii, float *records,
                              float *sh_rgb, float *zero_records, float *zero_tail, int64_t zero_tail_floats, int32_t *schedule,
                              bds_stream_t stream) {
  BDS_REQUIRE(n >= 0);
  BDS_REQUIRE(zero_tail_floats >= 0 && zero_tail_floats % 4 == 0 && zero_tail_floats < ((int64_t)1 << 24));
  BDS_REQUIRE((!zero_records || aligned16(zero_records)) && (!zero_tail || aligned16(zero_tail)));
  SceneTable t;
  const int rc = scene_table(n_seg, seg_rows, seg_kinds, seg_K, seg_degrees, const_cast<float *const *>(seg_colors),
                             const_cast<float *const *>(seg_rest), true, t);
  if (rc != BDS_OK) return rc;
  if (n == 0) {
    if (zero_tail && zero_tail_floats &&
        hipMemsetAsync(zero_tail, 0, sizeof(float) * zero_tail_floats, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    if (schedule && hipMemsetAsync(schedule, 0, sizeof(int32_t) * kSceneSchedHeader, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    return BDS_OK;
  }
  BDS_REQUIRE(ids && means && cam_pos && means2d && conics && depths && opacities && radii && records && sh_rgb);
  BDS_REQUIRE(aligned16(records) && (reinterpret_cast<uintptr_t>(means2d) & 7u) == 0);
  BDS_REQUIRE(depths != means2d + 2);   // the projection's outputs as separate arrays (the scene view's per-segment launches write columns)
  hipLaunchKernelGGL(scene_pack_kernel, dim3((unsigned)cdiv(n, kSceneBlock)), dim3(kSceneBlock), 0, as_stream(stream), n, n_dev, ids, t,
                     means, cam_pos, means2d, conics, depths, opacities, radii, reinterpret_cast<float4 *>(records), sh_rgb,
                     reinterpret_cast<float4 *>(zero_records), reinterpret_cast<float4 *>(zero_tail), (int)(zero_tail_floats / 4), schedule);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_scene_sh_bwd(int64_t n_list, const uint64_t *n_dev, const int32_t *ids, int n_seg, const int64_t *seg_rows,
                                const int *seg_kinds, const int *seg_K, const int *seg_degrees, float *const *seg_v_dc,
                                float *const *seg_v_rest, const float *means, const float *cam_pos, const float *sh_rgb,
                                const float *v_records, const float *scales, const float *opacities, float *v_scales,
                                float *v_opacities, bds_stream_t stream) {
  BDS_REQUIRE(n_list >= 0);
  SceneTable t;
  const int rc = scene_table(n_seg, seg_rows, seg_kinds, seg_K, seg_degrees, seg_v_dc, seg_v_rest, false, t);
  if (rc != BDS_OK) return rc;
  if (n_list == 0) return BDS_OK;
  BDS_REQUIRE(ids && means && cam_pos && sh_rgb && v_records && aligned16(v_records) && scales && opacities && v_scales && v_opacities);
  hipLaunchKernelGGL(scene_sh_bwd_kernel, dim3((unsigned)cdiv(n_list, kSceneBlock)), dim3(kSceneBlock), 0, as_stream(stream), n_list, n_dev,
                     ids, t, means, cam_pos, sh_rgb, reinterpret_cast<const float4 *>(v_records), scales, opacities, v_scales, v_opacities);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
