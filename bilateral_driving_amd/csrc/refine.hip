// Adaptive density control: split / duplicate / cull of one class of Gaussians together with its Adam state, and the periodic
// opacity reset.  The CORE serves every class: the planned layout below (the flag bits; refine_plan_run = block scan + ranks behind a
// class's flags kernel; RefineDest = where a row's original and children go), refine_rows_kernel for every array that only moves (the
// optimiser surgery dup_in_optim / remove_from_optim, models/gaussians/basics.py:162-206, is this kernel on the Adam moments),
// opacity_reset_kernel, and the per-row math of a split in csrc/refine_math.h.  A class adds its decision and its geometry kernel:
//   vanilla and the node classes: refine_flags_kernel (split, dup AND cull in one plan) and refine_geometry_kernel --
//     VanillaGaussians.refinement_after (models/gaussians/vanilla.py:205-304), split_gaussians (:336-363), dup_gaussians (:365-376),
//     cull_gaussians (:306-334); refine_out_of_bound_kernel is the node classes' box test, compacted by a second, cull-only plan
//   periodic-vibration: the pvg_* kernels, see their section below (a plan without a cull, then a cull-only plan over the NEW rows)
//
// The reference builds the new set in three rounds of boolean-mask indexing + torch.cat per tensor (6 parameters + 12 state
// tensors, each round a nonzero() with a host sync) and then compacts everything again for the cull.  Here the whole topology
// change is PLANNED once per Gaussian (5 flag bits + 4 exclusive ranks) and every array is then written exactly once, straight
// into its final, culled layout:
//
//   reference order after cat  : [ originals 0..N ) [ split children, sample-major: N + s*S + j ) [ dup children )
//   after the cull (order kept): [ kept originals ) [ kept split children of sample 0 | sample 1 | .. ) [ kept dup children )
//
// The children of one parent share its opacity and (shrunk) scale and have max_2Dsize = 0, so their cull decision is a function
// of the parent alone -> the destination of every row follows from per-parent ranks:
//   original g            -> rank_keepO[g]
//   split child s of g    -> KO + s*KS + rank_keepS[g]        (its noise sample is row s*S + rank_split[g] of `samples`)
//   dup child of g        -> KO + samps*KS + rank_keepD[g]
// HBM-bound byte movement: every parameter / state row is read once and written once (+ once per kept child).
// PINNED by tests/golden/refine_*.npz (the reference's own refinement_after, oracle/gen_golden_refine.py) and pvg_refine_*.npz.
#include "bds_common.h"
#include "pvg_math.h"
#include "refine_math.h"
#include "scan.h"

namespace bds {

constexpr int kRefBlock = 256;
constexpr int kRefWaves = kRefBlock / kWave;
enum RefineFlag : uint8_t { kSplit = 1, kDup = 2, kKeepO = 4, kKeepS = 8, kKeepD = 16 };
constexpr int kChan = 5;  // scanned channels: split, dup, keepO, keepS, keepD   (totals[] in this order)

struct RefineCfg {
  int do_densify;
  float grad_thresh, size_thresh;
  int split_by_screen;
  float split_screen_size;
  int do_cull;
  float cull_alpha;
  int cull_by_scale;
  float cull_scale;
  int cull_by_screen;
  float cull_screen;
};

// Where the rows that input Gaussian g leaves behind go in the planned layout (the table in the file header), and which row of
// `samples` its s-th split child reads.  Built once the row is known to keep anything: a dropped row reads neither ranks nor totals.
struct RefineDest {
  uint4 r;              // exclusive ranks of g: split, keepO, keepS, keepD
  int64_t S, KO, KS;    // totals: split parents, kept originals, kept split parents
  int samps;
  __device__ __forceinline__ RefineDest(int64_t g, int samps_, const uint32_t *__restrict__ ranks, const int64_t *__restrict__ totals)
      : r(reinterpret_cast<const uint4 *>(ranks)[g]), S(totals[0]), KO(totals[2]), KS(totals[3]), samps(samps_) {}
  __device__ __forceinline__ int64_t original() const { return (int64_t)r.y; }
  __device__ __forceinline__ int64_t split_child(int s) const { return KO + (int64_t)s * KS + r.z; }
  __device__ __forceinline__ int64_t dup_child() const { return KO + (int64_t)samps * KS + r.w; }
  __device__ __forceinline__ int64_t sample_row(int s) const { return (int64_t)s * S + r.x; }
};

__device__ __forceinline__ uint8_t refine_classify(int64_t g, const RefineCfg &c, const float *__restrict__ xys_grad_norm,
                                                   const float *__restrict__ vis_counts, const float *__restrict__ max_2Dsize,
                                                   const float *__restrict__ log_scales, const float *__restrict__ logits,
                                                   const uint8_t *__restrict__ extra_cull) {
#pragma clang fp contract(off)
  const float lmax = fmaxf(fmaxf(log_scales[g * 3], log_scales[g * 3 + 1]), log_scales[g * 3 + 2]);
  const float smax = expf(lmax);  // exp is monotone: max_i exp(s_i) = exp(max_i s_i)
  const float m2d = max_2Dsize ? max_2Dsize[g] : 0.f;
  bool split = false, dup = false;
  float s_post = smax;  // largest world-space scale after split_gaussians has shrunk the split parents in place
  if (c.do_densify) {  // vanilla.py:219-250
    const bool high = (xys_grad_norm[g] / vis_counts[g]) > c.grad_thresh;
    split = smax > c.size_thresh;
    if (c.split_by_screen) split = split || (m2d > c.split_screen_size);
    split = split && high;
    if (split) s_post = expf(refine_shrink_log(lmax));
    // the dup mask is evaluated AFTER the split (:246-250): a small Gaussian that is large on screen, or one that drops below
    // the size threshold by the 1/1.6 shrink, is split AND duplicated
    dup = (s_post <= c.size_thresh) && high;
  }
  bool cull_o = false, cull_child = false;
  if (c.do_cull) {  // vanilla.py:312-325, evaluated on the post-split scales
    const float op = 1.f / (1.f + expf(-logits[g]));
    cull_o = cull_child = op < c.cull_alpha;
    if (c.cull_by_scale) {
      const bool toobig = s_post > c.cull_scale;
      cull_o = cull_o || toobig;
      cull_child = cull_child || toobig;
      if (c.cull_by_screen) cull_o = cull_o || (m2d > c.cull_screen);  // children enter with max_2Dsize = 0
    }
  }
  // a caller-computed mask over the INPUT rows (the node classes' box test, see bds_refine_out_of_bound): the children are judged
  // by their own rows in a second plan, not by their parent
  if (c.do_cull && extra_cull && extra_cull[g]) cull_o = true;
  uint8_t f = 0;
  if (split) f |= kSplit;
  if (dup) f |= kDup;
  if (!cull_o) f |= kKeepO;
  if (split && !cull_child) f |= kKeepS;
  if (dup && !cull_child) f |= kKeepD;
  return f;
}

// flags + per-workgroup counts of the five channels
__global__ __launch_bounds__(kRefBlock) void refine_flags_kernel(int64_t N, RefineCfg c, const float *__restrict__ xys_grad_norm,
                                                                const float *__restrict__ vis_counts,
                                                                const float *__restrict__ max_2Dsize,
                                                                const float *__restrict__ log_scales,
                                                                const float *__restrict__ logits,
                                                                const uint8_t *__restrict__ extra_cull, uint8_t *__restrict__ flags,
                                                                uint32_t *__restrict__ blk) {
  __shared__ uint32_t lw[kRefWaves * kChan];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  uint8_t f = 0;
  if (g < N) {
    f = refine_classify(g, c, xys_grad_norm, vis_counts, max_2Dsize, log_scales, logits, extra_cull);
    flags[g] = f;
  }
  const uint32_t total = block_count<kChan, kRefWaves>(f, lw);
  if (threadIdx.x < kChan) blk[(int64_t)blockIdx.x * kChan + threadIdx.x] = total;
}

// exclusive scan of the per-workgroup counts (in place) + totals; ONE workgroup
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void refine_blockscan_kernel(int64_t nb, uint32_t *__restrict__ blk,
                                                                       int64_t *__restrict__ totals) {
  __shared__ uint32_t lw[kScanThreads / kWave];
  uint32_t total[kChan];
  workgroup_scan_in_place<kScanThreads, kChan>(blk, nb, total, lw);
  if (threadIdx.x == 0)
#pragma unroll
    for (int ch = 0; ch < kChan; ch++) totals[ch] = (int64_t)total[ch];
}

// exclusive ranks per Gaussian: [split, keepO, keepS, keepD]
__global__ __launch_bounds__(kRefBlock) void refine_ranks_kernel(int64_t N, const uint8_t *__restrict__ flags,
                                                                const uint32_t *__restrict__ blk, uint32_t *__restrict__ ranks) {
  __shared__ uint32_t lw[kRefWaves * 4];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  const uint32_t f = g < N ? flags[g] : 0;
  uint32_t out[4];
  block_rank<4>((f & 1u) | (f >> 2 << 1), out, lw);      // channels 0, 2, 3, 4 (kDup's rank is not used)
  if (g >= N) return;
  const int chan[4] = {0, 2, 3, 4};
#pragma unroll
  for (int k = 0; k < 4; k++) out[k] += blk[(int64_t)blockIdx.x * kChan + chan[k]];
  uint4 r;
  r.x = out[0]; r.y = out[1]; r.z = out[2]; r.w = out[3];
  reinterpret_cast<uint4 *>(ranks)[g] = r;
}

// means + log-scales of the new set (the only two parameters a split changes)
__global__ __launch_bounds__(kRefBlock) void refine_geometry_kernel(int64_t N, int samps, const uint8_t *__restrict__ flags,
                                                                   const uint32_t *__restrict__ ranks,
                                                                   const int64_t *__restrict__ totals,
                                                                   const float *__restrict__ samples,
                                                                   const float *__restrict__ means, const float *__restrict__ quats,
                                                                   const float *__restrict__ log_scales,
                                                                   float *__restrict__ new_means, float *__restrict__ new_log_scales) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (g >= N) return;
  const uint8_t f = flags[g];
  if (!(f & (kKeepO | kKeepS | kKeepD))) return;
  const RefineDest d(g, samps, ranks, totals);
  const float m[3] = {means[g * 3], means[g * 3 + 1], means[g * 3 + 2]};
  const float ls[3] = {log_scales[g * 3], log_scales[g * 3 + 1], log_scales[g * 3 + 2]};
  float lp[3] = {ls[0], ls[1], ls[2]};
  if (f & kSplit)
    for (int i = 0; i < 3; i++) lp[i] = refine_shrink_log(ls[i]);  // parent and children alike (vanilla.py:358-359)
  auto put = [&](int64_t dst, const float *mm) {
    for (int i = 0; i < 3; i++) { new_means[dst * 3 + i] = mm[i]; new_log_scales[dst * 3 + i] = lp[i]; }
  };
  if (f & kKeepO) put(d.original(), m);
  if (f & kKeepS) {
    // vanilla.py:343-348: rotate (scale * noise) by the normalised quaternion, add the mean
    const float q[4] = {quats[g * 4], quats[g * 4 + 1], quats[g * 4 + 2], quats[g * 4 + 3]};
    float R[9];
    refine_split_rotation(q, R);
    const float sc[3] = {expf(ls[0]), expf(ls[1]), expf(ls[2])};  // the scale BEFORE the shrink
    for (int s = 0; s < samps; s++) {
      float nm[3];
      refine_split_mean(R, sc, samples + d.sample_row(s) * 3, m, nm);
      put(d.split_child(s), nm);
    }
  }
  if (f & kKeepD) put(d.dup_child(), m);
}

// any other per-Gaussian array, one thread per element: rows of kept originals move to their new place; the children receive a
// copy of the parent's row (parameters) or zeros (Adam moments: basics.py:191-201 appends zeros_like)
__global__ __launch_bounds__(kRefBlock) void refine_rows_kernel(int64_t N, int width, int samps, const uint8_t *__restrict__ flags,
                                                               const uint32_t *__restrict__ ranks,
                                                               const int64_t *__restrict__ totals, const float *__restrict__ src,
                                                               float *__restrict__ dst, int zero_children) {
  const int64_t i = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (i >= N * width) return;
  const int64_t g = i / width;
  const int c = (int)(i - g * width);
  const uint8_t f = flags[g];
  if (!(f & (kKeepO | kKeepS | kKeepD))) return;
  const RefineDest d(g, samps, ranks, totals);
  const float v = src[i];
  const float cv = zero_children ? 0.f : v;
  if (f & kKeepO) dst[d.original() * width + c] = v;
  if (f & kKeepS)
    for (int s = 0; s < samps; s++) dst[d.split_child(s) * width + c] = cv;
  if (f & kKeepD) dst[d.dup_child() * width + c] = cv;
}

// nodes/rigid.py:374-383 (get_out_of_bound_mask): |mean| > instances_size[point_id] / 2 in any axis, means in the object frame
__global__ __launch_bounds__(kRefBlock) void refine_out_of_bound_kernel(int64_t N, const float *__restrict__ means,
                                                                       const int64_t *__restrict__ point_ids, int64_t n_instances,
                                                                       const float *__restrict__ instances_size,
                                                                       uint8_t *__restrict__ mask) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (g >= N) return;
  const int64_t id = point_ids[g];
  bool out = true;  // an id outside the table cannot be inside any box
  if (id >= 0 && id < n_instances) {
    out = false;
    for (int i = 0; i < 3; i++) out = out || (fabsf(means[g * 3 + i]) > instances_size[id * 3 + i] / 2.f);
  }
  mask[g] = out ? 1 : 0;
}

// vanilla.py:286-299: opacity = logit(min(sigmoid(opacity), reset_value)); the opacity group's Adam moments start again from zero
__global__ __launch_bounds__(kRefBlock) void opacity_reset_kernel(int64_t N, float *__restrict__ logits, float reset_value,
                                                                 float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (i >= N) return;
  const float op = 1.f / (1.f + expf(-logits[i]));
  const float x = fminf(op, reset_value);
  logits[i] = logf(x / (1.f - x));  // torch.logit
  if (exp_avg) exp_avg[i] = 0.f;
  if (exp_avg_sq) exp_avg_sq[i] = 0.f;
}

// ---- periodic-vibration Gaussians (PeriodicVibrationGaussians, models/gaussians/pvg.py) -----------------------------------------------
// after_train (:100-133), refinement_after (:148-265) with split_gaussians (:298-354), dup_gaussians (:356-372), cull_gaussians
// (:267-284), and the velocity_reg term of compute_reg_loss (:430-435).  The class's decisions differ from the vanilla ones in kind:
// the size thresholds are scaled per point by gamma (:90-98), a second gradient statistic drives time splits and duplications, a
// split samples in time as well, and the cull judges every NEW row by its own mean.  So the densification is planned WITHOUT a
// cull (every keep bit set: the existing ranks / totals / bds_refine_rows then append the children in the reference's order), and
// the cull is a second, cull-only bds_refine_plan over the new rows with pvg_cull_mask_kernel's mask as extra_cull.  The per-row
// math is csrc/pvg_math.h.  PINNED by tests/golden/pvg_refine_*.npz (the reference's own methods, scripts/gen_golden_pvg_refine.py).
__global__ __launch_bounds__(kRefBlock) void pvg_refine_flags_kernel(int64_t N, PvgRefineCfg c, const float *__restrict__ origin,
                                                                    const float *__restrict__ xys_grad_norm,
                                                                    const float *__restrict__ t_grad_accum,
                                                                    const float *__restrict__ vis_counts,
                                                                    const float *__restrict__ max_2Dsize,
                                                                    const float *__restrict__ log_scales, const float *__restrict__ betas,
                                                                    const float *__restrict__ means, uint8_t *__restrict__ flags,
                                                                    uint8_t *__restrict__ kinds, uint32_t *__restrict__ blk) {
  __shared__ uint32_t lw[kRefWaves * kChan];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  uint8_t f = 0;
  if (g < N) {
    for (int i = 0; i < 3; i++) c.origin[i] = origin[i];
    const float ls[3] = {log_scales[g * 3], log_scales[g * 3 + 1], log_scales[g * 3 + 2]};
    const float m[3] = {means[g * 3], means[g * 3 + 1], means[g * 3 + 2]};
    uint8_t kind;
    const unsigned sd = pvg_refine_decide(c, xys_grad_norm[g], t_grad_accum[g], vis_counts[g], max_2Dsize[g], ls, betas[g], m, &kind);
    f = (uint8_t)(sd | kKeepO | ((sd & 1u) ? kKeepS : 0) | ((sd & 2u) ? kKeepD : 0));      // no cull here: every row and child stays
    flags[g] = f;
    kinds[g] = kind;
  }
  const uint32_t total = block_count<kChan, kRefWaves>(f, lw);
  if (threadIdx.x < kChan) blk[(int64_t)blockIdx.x * kChan + threadIdx.x] = total;
}

// the four arrays a split changes, for the N + samps n_split + n_dup rows of a plan without a cull
__global__ __launch_bounds__(kRefBlock) void pvg_refine_geometry_kernel(
    int64_t N, int samps, int no_time_split, float T, const uint8_t *__restrict__ flags, const uint8_t *__restrict__ kinds,
    const uint32_t *__restrict__ ranks, const int64_t *__restrict__ totals, const float *__restrict__ samples,
    const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ log_scales,
    const float *__restrict__ velocity, const float *__restrict__ taus, const float *__restrict__ betas, float *__restrict__ new_means,
    float *__restrict__ new_log_scales, float *__restrict__ new_taus, float *__restrict__ new_betas) {
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (g >= N) return;
  const uint8_t f = flags[g];
  if (!(f & (kKeepO | kKeepS | kKeepD))) return;
  const RefineDest d(g, samps, ranks, totals);
  const float m[3] = {means[g * 3], means[g * 3 + 1], means[g * 3 + 2]};
  const float ls[3] = {log_scales[g * 3], log_scales[g * 3 + 1], log_scales[g * 3 + 2]};
  const float tau = taus[g], beta = betas[g];
  auto put = [&](int64_t dst, const float *mm, const float *sc, float ta, float be) {
    for (int i = 0; i < 3; i++) { new_means[dst * 3 + i] = mm[i]; new_log_scales[dst * 3 + i] = sc[i]; }
    new_taus[dst] = ta;
    new_betas[dst] = be;
  };
  if (!(f & kSplit)) {                      // untouched: the row and, when duplicated, its copy
    if (f & kKeepO) put(d.original(), m, ls, tau, beta);
    if (f & kKeepD) put(d.dup_child(), m, ls, tau, beta);
    return;
  }
  const float q[4] = {quats[g * 4], quats[g * 4 + 1], quats[g * 4 + 2], quats[g * 4 + 3]};
  const float vel[3] = {velocity[g * 3], velocity[g * 3 + 1], velocity[g * 3 + 2]};
  PvgSplitRow row;
  pvg_split_row(q, ls, beta, T, kinds[g], no_time_split, &row);
  if (f & kKeepO) put(d.original(), m, row.shrunk, tau, beta);      // the parent: shrunk scale, its own tau and beta (:323)
  if (f & kKeepS)
    for (int s = 0; s < samps; s++) {
      float nm[3], nt;
      pvg_split_child(row, m, vel, tau, samples + d.sample_row(s) * 4, nm, &nt);
      put(d.split_child(s), nm, row.child_scale, nt, row.child_beta);
    }
  if (f & kKeepD) put(d.dup_child(), m, row.shrunk, tau, beta);      // a copy of the shrunk parent (:367)
}

// cull_gaussians on the rows AFTER the children were appended: rows >= n_old are children (max_2Dsize 0)
__global__ __launch_bounds__(kRefBlock) void pvg_cull_mask_kernel(int64_t N, int64_t n_old, PvgCullCfg c, const float *__restrict__ origin,
                                                                 const float *__restrict__ logits, const float *__restrict__ log_scales,
                                                                 const float *__restrict__ means, const float *__restrict__ max_2Dsize,
                                                                 uint8_t *__restrict__ mask) {
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (g >= N) return;
  for (int i = 0; i < 3; i++) c.origin[i] = origin[i];
  const float ls[3] = {log_scales[g * 3], log_scales[g * 3 + 1], log_scales[g * 3 + 2]};
  const float m[3] = {means[g * 3], means[g * 3 + 1], means[g * 3 + 2]};
  const float m2d = (c.by_screen && g < n_old) ? max_2Dsize[g] : 0.f;
  mask[g] = pvg_cull(c, logits[g], ls, m, m2d) ? 1 : 0;
}

// kept rows of filter_mask [N] -> their index among the kept rows: per-workgroup counts, one-workgroup exclusive scan (blk[nb] = M)
__global__ __launch_bounds__(kRefBlock) void pvg_mask_count_kernel(int64_t N, const uint8_t *__restrict__ mask, uint32_t *__restrict__ blk) {
  __shared__ uint32_t lw[kRefWaves];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  const uint32_t total = block_count<1, kRefWaves>(g < N && mask[g] ? 1u : 0u, lw);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void pvg_mask_scan_kernel(int64_t nb, uint32_t *__restrict__ blk) {
  __shared__ uint32_t lw[kScanThreads / kWave];
  uint32_t total[1];
  workgroup_scan_in_place<kScanThreads, 1>(blk, nb, total, lw);
  if (threadIdx.x == 0) blk[nb] = total[0];
}

__device__ __forceinline__ float pvg_radius(const void *radii, int radii_float, int64_t r) {
  return radii_float ? static_cast<const float *>(radii)[r] : (float)static_cast<const int32_t *>(radii)[r];
}

// after_train (pvg.py:100-133).  Row r of grad2d / radii is the r-th class row with filter_mask set; a mask with more than M set
// rows touches nothing beyond row M - 1.
__global__ __launch_bounds__(kRefBlock) void pvg_stats_kernel(int64_t N, int64_t M, const uint8_t *__restrict__ mask,
                                                             const uint32_t *__restrict__ blk, const float *__restrict__ grad2d, float sx,
                                                             float sy, const void *__restrict__ radii, int radii_float,
                                                             const float *__restrict__ taus_grad, float last_size, int first,
                                                             float *__restrict__ xys_grad_norm, float *__restrict__ t_grad_accum,
                                                             float *__restrict__ vis_counts, float *__restrict__ max_2Dsize) {
#pragma clang fp contract(off)
  __shared__ uint32_t lw[kRefWaves];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  const bool set = g < N && mask[g];
  uint32_t rank[1];
  block_rank<1>(set ? 1u : 0u, rank, lw);
  if (g >= N) return;
  const int64_t r = (int64_t)rank[0] + blk[blockIdx.x];
  const bool kept = set && r < M;
  const float rad = kept ? pvg_radius(radii, radii_float, r) : 0.f;
  const bool vis = kept && rad > 0.f;
  float n = 0.f, tg = 0.f;
  if (kept && (first || vis)) {
    n = pvg_grad_norm(grad2d[r * 2], grad2d[r * 2 + 1], sx, sy);
    tg = fabsf(taus_grad[g]);
  }
  if (first) {                        // :114-120, :128-133
    xys_grad_norm[g] = n;
    t_grad_accum[g] = tg;
    vis_counts[g] = 1.f;
    max_2Dsize[g] = vis ? fmaxf(0.f, rad / last_size) : 0.f;
  } else if (vis) {                   // :122-125, :131-133
    vis_counts[g] = vis_counts[g] + 1.f;
    xys_grad_norm[g] = n + xys_grad_norm[g];
    t_grad_accum[g] = tg + t_grad_accum[g];
    max_2Dsize[g] = fmaxf(max_2Dsize[g], rad / last_size);
  }
}

// velocity_reg (pvg.py:430-435): the sum of |velocity| over the kept rows with cur_radii > 0 and their number, in a fixed order
// (lanes by a shuffle tree, waves and workgroups in sequence): two runs give the same bits.  vis [N] marks the rows for the backward.
__device__ __forceinline__ void pvg_block_sum(float &v, uint32_t &c, float *lds_f, uint32_t *lds_c) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    v += __shfl_down(v, o);
    c += __shfl_down(c, o);
  }
  const int nw = blockDim.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) { lds_f[threadIdx.x / kWave] = v; lds_c[threadIdx.x / kWave] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    v = lds_f[0]; c = lds_c[0];
    for (int w = 1; w < nw; w++) { v += lds_f[w]; c += lds_c[w]; }
  }
}

__global__ __launch_bounds__(kRefBlock) void pvg_velocity_reg_fwd_kernel(int64_t N, int64_t M, float T, const uint8_t *__restrict__ mask,
                                                                        const uint32_t *__restrict__ blk,
                                                                        const void *__restrict__ radii, int radii_float,
                                                                        const float *__restrict__ velocity, const float *__restrict__ betas,
                                                                        uint8_t *__restrict__ vis, float *__restrict__ part_sum,
                                                                        uint32_t *__restrict__ part_cnt) {
  __shared__ uint32_t lw[kRefWaves];
  __shared__ float lf[kRefWaves];
  __shared__ uint32_t lc[kRefWaves];
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  const bool set = g < N && mask[g];
  uint32_t rank[1];
  block_rank<1>(set ? 1u : 0u, rank, lw);
  const int64_t r = (int64_t)rank[0] + blk[blockIdx.x];
  const bool seen = set && r < M && pvg_radius(radii, radii_float, r) > 0.f;
  float v = 0.f;
  uint32_t c = seen ? 1u : 0u;
  if (seen) {
    const float vel[3] = {velocity[g * 3], velocity[g * 3 + 1], velocity[g * 3 + 2]};
    v = pvg_velocity_norm(vel, betas[g], T);
  }
  if (g < N) vis[g] = seen ? 1 : 0;
  pvg_block_sum(v, c, lf, lc);
  if (threadIdx.x == 0) { part_sum[blockIdx.x] = v; part_cnt[blockIdx.x] = c; }
}

// the ordered pass over the per-workgroup partials: out = {sum, count} (double: a count up to 2^31 is exact)
__global__ __launch_bounds__(kScanThreads) void pvg_velocity_reg_final_kernel(int64_t nb, const float *__restrict__ part_sum,
                                                                             const uint32_t *__restrict__ part_cnt,
                                                                             double *__restrict__ out) {
  __shared__ float lf[kScanThreads / kWave];
  __shared__ uint32_t lc[kScanThreads / kWave];
  const int64_t seg = (nb + kScanThreads - 1) / kScanThreads;
  const int64_t lo = threadIdx.x * seg < nb ? threadIdx.x * seg : nb, hi = lo + seg < nb ? lo + seg : nb;
  float v = 0.f;
  uint32_t c = 0;
  for (int64_t i = lo; i < hi; i++) { v += part_sum[i]; c += part_cnt[i]; }
  pvg_block_sum(v, c, lf, lc);
  if (threadIdx.x == 0) { out[0] = (double)v; out[1] = (double)c; }
}

// gradient of (sum * scale[0]) towards _velocity and _betas; rows outside the set get exact zeros
__global__ __launch_bounds__(kRefBlock) void pvg_velocity_reg_bwd_kernel(int64_t N, float T, const uint8_t *__restrict__ vis,
                                                                        const float *__restrict__ scale,
                                                                        const float *__restrict__ velocity, const float *__restrict__ betas,
                                                                        float *__restrict__ g_velocity, float *__restrict__ g_betas) {
  const int64_t g = (int64_t)blockIdx.x * kRefBlock + threadIdx.x;
  if (g >= N) return;
  float gv[3] = {0.f, 0.f, 0.f}, gb = 0.f;
  if (vis[g]) {
    const float vel[3] = {velocity[g * 3], velocity[g * 3 + 1], velocity[g * 3 + 2]};
    pvg_velocity_norm_vjp(vel, betas[g], T, scale[0], gv, &gb);
  }
  for (int i = 0; i < 3; i++) g_velocity[g * 3 + i] = gv[i];
  g_betas[g] = gb;
}

}  // namespace bds

using namespace bds;

extern "C" size_t bds_refine_plan_temp_bytes(int64_t N) {
  if (N < 0) return 0;
  return (size_t)(cdiv(N, kRefBlock) + 1) * kChan * sizeof(uint32_t);
}

// What every class's plan has in common: the checks on the plan's own arrays, the empty set (zero totals, nothing launched: no
// pointer but `totals` is needed) and, behind the class's flags kernel, the block scan and the ranks.  `inputs_ok`: the class's own
// argument checks; `launch_flags(nb, blk, stream)` starts its flags kernel, which leaves flags [N] and the per-workgroup counts.
template <class LaunchFlags>
static int refine_plan_run(int64_t N, bool inputs_ok, uint8_t *flags, uint32_t *ranks, int64_t *totals, void *temp, size_t temp_bytes,
                           bds_stream_t stream, LaunchFlags launch_flags) {
  BDS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && totals);
  hipStream_t st = as_stream(stream);
  if (N == 0) {
    if (hipMemsetAsync(totals, 0, kChan * sizeof(int64_t), st) != hipSuccess) return BDS_ELAUNCH;
    return BDS_OK;
  }
  BDS_REQUIRE(inputs_ok && flags && ranks && temp && temp_bytes >= bds_refine_plan_temp_bytes(N) && aligned16(ranks));
  const int64_t nb = cdiv(N, kRefBlock);
  uint32_t *blk = static_cast<uint32_t *>(temp);
  launch_flags(nb, blk, st);
  hipLaunchKernelGGL(refine_blockscan_kernel, dim3(1), dim3(kScanThreads), 0, st, nb, blk, totals);
  hipLaunchKernelGGL(refine_ranks_kernel, dim3((unsigned)nb), dim3(kRefBlock), 0, st, N, flags, blk, ranks);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_refine_plan(int64_t N, const float *xys_grad_norm, const float *vis_counts, const float *max_2Dsize,
                               const float *log_scales, const float *logits, const uint8_t *extra_cull, int do_densify,
                               float grad_thresh,
                               float size_thresh, int split_by_screen, float split_screen_size, int do_cull,
                               float cull_alpha_thresh, int cull_by_scale, float cull_scale_thresh, int cull_by_screen,
                               float cull_screen_size, uint8_t *flags, uint32_t *ranks, int64_t *totals, void *temp,
                               size_t temp_bytes, bds_stream_t stream) {
  RefineCfg c{do_densify, grad_thresh, size_thresh, split_by_screen, split_screen_size, do_cull, cull_alpha_thresh,
              cull_by_scale, cull_scale_thresh, cull_by_screen, cull_screen_size};
  const bool inputs = log_scales && logits && (!do_densify || (xys_grad_norm && vis_counts));
  return refine_plan_run(N, inputs, flags, ranks, totals, temp, temp_bytes, stream, [&](int64_t nb, uint32_t *blk, hipStream_t st) {
    hipLaunchKernelGGL(refine_flags_kernel, dim3((unsigned)nb), dim3(kRefBlock), 0, st, N, c, xys_grad_norm, vis_counts, max_2Dsize,
                       log_scales, logits, extra_cull, flags, blk);
  });
}

extern "C" int bds_refine_geometry(int64_t N, int samps, const uint8_t *flags, const uint32_t *ranks, const int64_t *totals,
                                   const float *samples, const float *means, const float *quats, const float *log_scales,
                                   float *new_means, float *new_log_scales, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && samps >= 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(flags && ranks && totals && means && quats && log_scales && new_means && new_log_scales);
  hipLaunchKernelGGL(refine_geometry_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, samps,
                     flags, ranks, totals, samples, means, quats, log_scales, new_means, new_log_scales);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_refine_rows(int64_t N, int width, int samps, const uint8_t *flags, const uint32_t *ranks,
                               const int64_t *totals, const float *src, float *dst, int zero_children, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && width >= 1 && samps >= 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(flags && ranks && totals && src && dst);
  hipLaunchKernelGGL(refine_rows_kernel, dim3((unsigned)cdiv(N * width, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, width,
                     samps, flags, ranks, totals, src, dst, zero_children);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_refine_out_of_bound(int64_t N, const float *means, const int64_t *point_ids, int64_t n_instances,
                                       const float *instances_size, uint8_t *mask, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && n_instances >= 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(means && point_ids && instances_size && mask);
  hipLaunchKernelGGL(refine_out_of_bound_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, means,
                     point_ids, n_instances, instances_size, mask);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_opacity_reset(int64_t N, float *logits, float reset_value, float *exp_avg, float *exp_avg_sq,
                                 bds_stream_t stream) {
  BDS_REQUIRE(N >= 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(logits);
  hipLaunchKernelGGL(opacity_reset_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, logits,
                     reset_value, exp_avg, exp_avg_sq);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_pvg_refine_plan(int64_t N, const float *xys_grad_norm, const float *t_grad_accum, const float *vis_counts,
                                   const float *max_2Dsize, const float *log_scales, const float *betas, const float *means,
                                   const float *scene_origin, float scene_scale, float grad_thresh, float t_grad_thresh,
                                   float size_thresh, float t_size_thresh, int split_by_screen, float split_screen_size, uint8_t *flags,
                                   uint8_t *kinds, uint32_t *ranks, int64_t *totals, void *temp, size_t temp_bytes,
                                   bds_stream_t stream) {
  PvgRefineCfg c{grad_thresh, t_grad_thresh, size_thresh, t_size_thresh, split_by_screen, split_screen_size, scene_scale, {0.f, 0.f, 0.f}};
  const bool inputs = xys_grad_norm && t_grad_accum && vis_counts && max_2Dsize && log_scales && betas && means && scene_origin && kinds &&
                      scene_scale > 0.f;
  return refine_plan_run(N, inputs, flags, ranks, totals, temp, temp_bytes, stream, [&](int64_t nb, uint32_t *blk, hipStream_t st) {
    hipLaunchKernelGGL(pvg_refine_flags_kernel, dim3((unsigned)nb), dim3(kRefBlock), 0, st, N, c, scene_origin, xys_grad_norm, t_grad_accum,
                       vis_counts, max_2Dsize, log_scales, betas, means, flags, kinds, blk);
  });
}

extern "C" int bds_pvg_refine_geometry(int64_t N, int samps, int no_time_split, double T, const uint8_t *flags, const uint8_t *kinds,
                                       const uint32_t *ranks, const int64_t *totals, const float *samples, const float *means,
                                       const float *quats, const float *log_scales, const float *velocity, const float *taus,
                                       const float *betas, float *new_means, float *new_log_scales, float *new_taus, float *new_betas,
                                       bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && samps >= 1 && T > 0.0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(flags && kinds && ranks && totals && means && quats && log_scales && velocity && taus && betas);
  BDS_REQUIRE(new_means && new_log_scales && new_taus && new_betas && aligned16(ranks));
  hipLaunchKernelGGL(pvg_refine_geometry_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, samps,
                     no_time_split, (float)T, flags, kinds, ranks, totals, samples, means, quats, log_scales, velocity, taus, betas,
                     new_means, new_log_scales, new_taus, new_betas);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_pvg_cull_mask(int64_t N, int64_t n_old, const float *logits, const float *log_scales, const float *means,
                                 const float *max_2Dsize, const float *scene_origin, float scene_scale, float cull_alpha_thresh,
                                 int cull_by_scale, float cull_scale_thresh, int cull_by_screen, float cull_screen_size, uint8_t *mask,
                                 bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && n_old >= 0 && n_old <= N);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(logits && log_scales && means && scene_origin && mask && scene_scale > 0.f);
  const int by_screen = cull_by_scale && cull_by_screen;
  BDS_REQUIRE(!by_screen || n_old == 0 || max_2Dsize);
  PvgCullCfg c{cull_alpha_thresh, cull_by_scale, cull_scale_thresh, by_screen, cull_screen_size, scene_scale, {0.f, 0.f, 0.f}};
  hipLaunchKernelGGL(pvg_cull_mask_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, n_old, c,
                     scene_origin, logits, log_scales, means, max_2Dsize, mask);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" size_t bds_pvg_mask_temp_bytes(int64_t N) {
  if (N <= 0) return 0;
  return (size_t)(cdiv(N, kRefBlock) + 1) * 3 * sizeof(uint32_t);      // offsets (+ total), partial sums, partial counts
}

static void pvg_mask_offsets(int64_t N, const uint8_t *mask, uint32_t *blk, hipStream_t st) {
  const int64_t nb = cdiv(N, kRefBlock);
  hipLaunchKernelGGL(pvg_mask_count_kernel, dim3((unsigned)nb), dim3(kRefBlock), 0, st, N, mask, blk);
  hipLaunchKernelGGL(pvg_mask_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, nb, blk);
}

extern "C" int bds_pvg_densify_stats(int64_t N, int64_t M, const uint8_t *filter_mask, const float *grad2d, float sx, float sy,
                                     const void *radii, int radii_float, const float *taus_grad, int last_size, int first,
                                     float *xys_grad_norm, float *t_grad_accum, float *vis_counts, float *max_2Dsize, void *temp,
                                     size_t temp_bytes, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && M >= 0 && M <= N && last_size > 0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(filter_mask && taus_grad && xys_grad_norm && t_grad_accum && vis_counts && max_2Dsize);
  BDS_REQUIRE(M == 0 || (grad2d && radii));
  BDS_REQUIRE(temp && temp_bytes >= bds_pvg_mask_temp_bytes(N));
  hipStream_t st = as_stream(stream);
  uint32_t *blk = static_cast<uint32_t *>(temp);
  pvg_mask_offsets(N, filter_mask, blk, st);
  hipLaunchKernelGGL(pvg_stats_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, st, N, M, filter_mask, blk, grad2d, sx, sy,
                     radii, radii_float, taus_grad, (float)last_size, first, xys_grad_norm, t_grad_accum, vis_counts, max_2Dsize);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_pvg_velocity_reg_fwd(int64_t N, int64_t M, double T, const uint8_t *filter_mask, const void *radii, int radii_float,
                                        const float *velocity, const float *betas, uint8_t *vis, double *out, void *temp,
                                        size_t temp_bytes, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31) && M >= 0 && M <= N && T > 0.0 && out);
  hipStream_t st = as_stream(stream);
  if (N == 0) {
    if (hipMemsetAsync(out, 0, 2 * sizeof(double), st) != hipSuccess) return BDS_ELAUNCH;
    return BDS_OK;
  }
  BDS_REQUIRE(filter_mask && velocity && betas && vis && (M == 0 || radii));
  BDS_REQUIRE(temp && temp_bytes >= bds_pvg_mask_temp_bytes(N));
  const int64_t nb = cdiv(N, kRefBlock);
  uint32_t *blk = static_cast<uint32_t *>(temp);
  float *part_sum = reinterpret_cast<float *>(blk + nb + 1);
  uint32_t *part_cnt = blk + 2 * (nb + 1);
  pvg_mask_offsets(N, filter_mask, blk, st);
  hipLaunchKernelGGL(pvg_velocity_reg_fwd_kernel, dim3((unsigned)nb), dim3(kRefBlock), 0, st, N, M, (float)T, filter_mask, blk, radii,
                     radii_float, velocity, betas, vis, part_sum, part_cnt);
  hipLaunchKernelGGL(pvg_velocity_reg_final_kernel, dim3(1), dim3(kScanThreads), 0, st, nb, part_sum, part_cnt, out);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_pvg_velocity_reg_bwd(int64_t N, double T, const uint8_t *vis, const float *scale, const float *velocity,
                                        const float *betas, float *g_velocity, float *g_betas, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && T > 0.0);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(vis && scale && velocity && betas && g_velocity && g_betas);
  hipLaunchKernelGGL(pvg_velocity_reg_bwd_kernel, dim3((unsigned)cdiv(N, kRefBlock)), dim3(kRefBlock), 0, as_stream(stream), N, (float)T,
                     vis, scale, velocity, betas, g_velocity, g_betas);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
