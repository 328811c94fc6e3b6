// TEST-ONLY host shim of the periodic-vibration Gaussians' density-control math (csrc/pvg_math.h, the functions the pvg_* kernels of
// csrc/refine.hip run) on the CPU, so that tests/test_pvg_refine_cpu.py can compare it with the float64 restatement without a GPU.
// Not part of libbds.so, never loaded by the product.  Every row is evaluated on its own (no ranks, no compaction).
#include "../bilateral_driving_amd/csrc/pvg_math.h"

using namespace bds;

// flags[i]: bit 0 split, bit 1 dup; kinds[i]: PvgKind bits
extern "C" void hm_pvg_refine_decide(int n, float grad_thresh, float t_grad_thresh, float size_thresh, float t_size_thresh, int split_by_screen,
                                     float split_screen_size, float scene_scale, const float *origin, const float *xys_grad_norm,
                                     const float *t_grad_accum, const float *vis_counts, const float *max_2Dsize, const float *log_scales,
                                     const float *betas, const float *means, unsigned char *flags, unsigned char *kinds) {
  PvgRefineCfg c{grad_thresh, t_grad_thresh, size_thresh, t_size_thresh, split_by_screen, split_screen_size, scene_scale,
                 {origin[0], origin[1], origin[2]}};
  for (int i = 0; i < n; i++)
    flags[i] = (unsigned char)pvg_refine_decide(c, xys_grad_norm[i], t_grad_accum[i], vis_counts[i], max_2Dsize[i], log_scales + i * 3, betas[i],
                                                means + i * 3, kinds + i);
}

// every row as a split parent with `samps` children: samples [n, samps, 4]
extern "C" void hm_pvg_refine_split(int n, int samps, int no_time_split, double T, const unsigned char *kinds, const float *samples,
                                    const float *means, const float *quats, const float *log_scales, const float *velocity, const float *taus,
                                    const float *betas, float *shrunk, float *child_scale, float *child_beta, float *child_means,
                                    float *child_taus) {
  for (int i = 0; i < n; i++) {
    PvgSplitRow row;
    pvg_split_row(quats + i * 4, log_scales + i * 3, betas[i], (float)T, kinds[i], no_time_split, &row);
    for (int k = 0; k < 3; k++) {
      shrunk[i * 3 + k] = row.shrunk[k];
      child_scale[i * 3 + k] = row.child_scale[k];
    }
    child_beta[i] = row.child_beta;
    for (int s = 0; s < samps; s++)
      pvg_split_child(row, means + i * 3, velocity + i * 3, taus[i], samples + ((size_t)i * samps + s) * 4,
                      child_means + ((size_t)i * samps + s) * 3, child_taus + (size_t)i * samps + s);
  }
}

extern "C" void hm_pvg_cull(int n, float cull_alpha, int by_scale, float cull_scale, int by_screen, float cull_screen, float scene_scale,
                            const float *origin, const float *logits, const float *log_scales, const float *means, const float *max_2Dsize,
                            unsigned char *mask) {
  PvgCullCfg c{cull_alpha, by_scale, cull_scale, by_scale && by_screen, cull_screen, scene_scale, {origin[0], origin[1], origin[2]}};
  for (int i = 0; i < n; i++) mask[i] = pvg_cull(c, logits[i], log_scales + i * 3, means + i * 3, max_2Dsize[i]) ? 1 : 0;
}

extern "C" void hm_pvg_grad_norm(int n, float sx, float sy, const float *grad2d, float *out) {
  for (int i = 0; i < n; i++) out[i] = pvg_grad_norm(grad2d[i * 2], grad2d[i * 2 + 1], sx, sy);
}

extern "C" void hm_pvg_velocity(int n, double T, float go, const float *velocity, const float *betas, float *norm, float *g_velocity,
                                float *g_betas) {
  for (int i = 0; i < n; i++) {
    norm[i] = pvg_velocity_norm(velocity + i * 3, betas[i], (float)T);
    pvg_velocity_norm_vjp(velocity + i * 3, betas[i], (float)T, go, g_velocity + i * 3, g_betas + i);
  }
}
