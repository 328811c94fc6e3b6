// Per-row math of the periodic-vibration Gaussians' time transform (PeriodicVibrationGaussians.get_gaussians,
// models/gaussians/pvg.py:374-425 with get_marginal_t :81, temporal_means :65-73, temporal_opacities :75-78, velocity / rho :83-88),
// used by csrc/pvg.hip and by the host shim tests/hostmath_pvg_shim.hip.  With d = tau - cur_time, s_t = exp(beta), a = 2 pi / T:
//   marg     = exp(-0.5 d^2 / s_t^2)                    keep = marg > 0.05 (float32; a NaN tau / beta drops the row)
//   mean'    = mean + velocity sin((cur_time - tau) a) / a  [+ velocity exp(-0.5 s_t / T) delta_t when smoothing]
//   opacity  = sigmoid(logit) marg,  scale = exp(log_scale),  quat = q / |q|
//   rgb      = clamp(SH(deg, normalise(mean' - cam_pos)) + 0.5, 0, 1)   (mode kPvgSigmoid, the class's sh_degree == 0: sigmoid(dc))
// The operations keep the reference's order (the Python scalars meet float32 tensors as float32); exp and sin are the accurate
// library forms: the sine's argument reaches tens of radians at the shipped T = 0.2.
#pragma once
#include <math.h>
#include "gs_math.h"

namespace bds {

constexpr int kPvgSigmoid = 4;        // colour mode: 0..3 = SH degrees to use, 4 = sigmoid of band 0
constexpr float kPvgKeep = 0.05f;     // pvg.py:389

struct PvgTime {
  float cur_time, delta_t, a, T;      // a = 1 / T * pi * 2 evaluated in double on the double T and rounded once, T rounded once (pvg.py:66, :86)
  int smooth;
};

BDS_HD float pvg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// get_marginal_t (pvg.py:81): the value the keep decision compares with 0.05
BDS_HD float pvg_marginal(float tau, float beta, float cur_time) {
  const float d = tau - cur_time, st = expf(beta);
  return expf((-0.5f * (d * d)) / (st * st));
}

// temporal_means of a kept row (pvg.py:65-73)
BDS_HD void pvg_means(const PvgTime &t, const float *mean, const float *vel, float tau, float beta, float *o_mean) {
  const float s = sinf((t.cur_time - tau) * t.a);
  float drift = 0.0f;
  if (t.smooth) drift = expf(-0.5f * (expf(beta) / t.T));
  for (int k = 0; k < 3; k++) {
    float m = mean[k] + vel[k] * s / t.a;
    if (t.smooth) m = m + (vel[k] * drift) * t.delta_t;
    o_mean[k] = m;
  }
}

// temporal_opacities and the activations of a kept row; `marg` is pvg_marginal of the same row
BDS_HD void pvg_activations(float logit, const float *log_scale, const float *q, float marg, float *o_opacity, float *o_scale,
                            float *o_quat) {
  for (int k = 0; k < 3; k++) o_scale[k] = expf(log_scale[k]);
  *o_opacity = pvg_sigmoid(logit) * marg;
  const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);   // a zero row gives NaN, as x / x.norm()
  for (int k = 0; k < 4; k++) o_quat[k] = q[k] * inv;
}

// the four small outputs of a kept row
BDS_HD void pvg_forward(const PvgTime &t, const float *mean, const float *vel, float tau, float beta, float logit, const float *log_scale,
                        const float *q, float marg, float *o_mean, float *o_opacity, float *o_scale, float *o_quat) {
  pvg_means(t, mean, vel, tau, beta, o_mean);
  pvg_activations(logit, log_scale, q, marg, o_opacity, o_scale, o_quat);
}

// SH bases of the view direction of a transformed mean (detached in the reference: no gradient flows back through it)
BDS_HD void pvg_bases(int deg, const float *o_mean, const float *cam_pos, float *B) {
  const float x = o_mean[0] - cam_pos[0], y = o_mean[1] - cam_pos[1], z = o_mean[2] - cam_pos[2];
  const float inorm = 1.0f / sqrtf(x * x + y * y + z * z);
  sh_bases(deg, x * inorm, y * inorm, z * inorm, B);
}

// torch.clamp: a NaN stays a NaN (both comparisons are false for it; fmaxf / fminf would turn it into 0 and hide it from the NaN check)
BDS_HD float pvg_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// Gradients of a kept row's time parameters and small tensors.  tau and beta receive both the opacity's term (through marg) and the
// means' (sine phase; the smoothing drift's exp(-0.5 s_t / T) for beta).
BDS_HD void pvg_backward(const PvgTime &t, const float *vel, float tau, float beta, float logit, const float *log_scale, const float *q,
                         const float *v_mean, float v_opacity, const float *v_scale, const float *v_quat, float *g_vel, float *g_tau,
                         float *g_beta, float *g_logit, float *g_log_scale, float *g_quat) {
  const float d = tau - t.cur_time, st = expf(beta), ist2 = 1.0f / (st * st);
  const float marg = expf((-0.5f * (d * d)) * ist2);
  const float ph = (t.cur_time - tau) * t.a, s = sinf(ph), c = cosf(ph);
  const float drift = t.smooth ? expf(-0.5f * (st / t.T)) : 0.0f;
  const float w = s / t.a + drift * t.delta_t;          // d mean' / d velocity (drift = 0 without smoothing)
  float dot = 0.0f;
  for (int k = 0; k < 3; k++) {
    g_vel[k] = v_mean[k] * w;
    dot += v_mean[k] * vel[k];
    g_log_scale[k] = v_scale[k] * expf(log_scale[k]);
  }
  const float sg = pvg_sigmoid(logit);
  const float v_marg = v_opacity * sg * marg;           // times d log(marg) below
  *g_logit = v_opacity * marg * sg * (1.0f - sg);
  *g_tau = -dot * c - v_marg * d * ist2;
  *g_beta = v_marg * (d * d) * ist2 + dot * t.delta_t * drift * (-0.5f / t.T) * st;
  const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float u[4], du = 0.0f;
  for (int k = 0; k < 4; k++) {
    u[k] = q[k] * inv;
    du += u[k] * v_quat[k];
  }
  for (int k = 0; k < 4; k++) g_quat[k] = (v_quat[k] - u[k] * du) * inv;
}

// torch.clamp passes the gradient on the closed interval; raw = the SH value before + 0.5
BDS_HD float pvg_clamp_grad(float raw, float v) {
  const float x = raw + 0.5f;
  return (x >= 0.0f && x <= 1.0f) ? v : 0.0f;
}

}  // namespace bds
