// TEST-ONLY host shim of the periodic-vibration Gaussians' per-row math (csrc/pvg_math.h, the functions the kernels of csrc/pvg.hip
// run) on the CPU, so that tests/test_pvg_cpu.py can compare it with float64 autograd without a GPU.  Not part of libbds.so, never
// loaded by the product.  Every row is evaluated (no compaction); keep[i] is the kernel's decision marg > 0.05.
#include "../bilateral_driving_amd/csrc/pvg_math.h"

using namespace bds;

static PvgTime hm_time(float cur_time, float delta_t, int smooth, double T) {
  PvgTime t;
  t.cur_time = cur_time;
  t.delta_t = delta_t;
  t.T = (float)T;
  t.a = (float)(1.0 / T * 3.141592653589793 * 2.0);
  t.smooth = smooth;
  return t;
}

// deg 0..3: the SH colour of coeffs [n,K,3] (band 0 first), deg 4 (kPvgSigmoid): sigmoid of band 0
extern "C" void hm_pvg_fwd(int n, int K, int deg, float cur_time, float delta_t, int smooth, double T, const float *mean, const float *vel,
                           const float *tau, const float *beta, const float *logit, const float *log_scale, const float *quat,
                           const float *coeffs, const float *cam, float *o_mean, float *o_opacity, float *o_rgb, float *o_scale,
                           float *o_quat, unsigned char *keep) {
  const PvgTime t = hm_time(cur_time, delta_t, smooth, T);
  for (int i = 0; i < n; i++) {
    const float marg = pvg_marginal(tau[i], beta[i], cur_time);
    keep[i] = marg > kPvgKeep;
    pvg_forward(t, mean + i * 3, vel + i * 3, tau[i], beta[i], logit[i], log_scale + i * 3, quat + i * 4, marg, o_mean + i * 3, o_opacity + i,
                o_scale + i * 3, o_quat + i * 4);
    const float *c = coeffs + (size_t)i * K * 3;
    if (deg == kPvgSigmoid) {
      for (int k = 0; k < 3; k++) o_rgb[i * 3 + k] = pvg_sigmoid(c[k]);
      continue;
    }
    float B[16];
    pvg_bases(deg, o_mean + i * 3, cam, B);
    for (int k = 0; k < 3; k++) {
      float raw = 0.0f;
      for (int b = 0; b < (deg + 1) * (deg + 1); b++) raw += B[b] * c[b * 3 + k];
      o_rgb[i * 3 + k] = pvg_clamp01(raw + 0.5f);
    }
  }
}

extern "C" void hm_pvg_bwd(int n, float cur_time, float delta_t, int smooth, double T, const float *vel, const float *tau, const float *beta,
                           const float *logit, const float *log_scale, const float *quat, const float *v_mean, const float *v_opacity,
                           const float *v_scale, const float *v_quat, float *g_vel, float *g_tau, float *g_beta, float *g_logit,
                           float *g_log_scale, float *g_quat) {
  const PvgTime t = hm_time(cur_time, delta_t, smooth, T);
  for (int i = 0; i < n; i++)
    pvg_backward(t, vel + i * 3, tau[i], beta[i], logit[i], log_scale + i * 3, quat + i * 4, v_mean + i * 3, v_opacity[i], v_scale + i * 3,
                 v_quat + i * 4, g_vel + i * 3, g_tau + i, g_beta + i, g_logit + i, g_log_scale + i * 3, g_quat + i * 4);
}
