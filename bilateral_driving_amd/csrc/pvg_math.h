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
#include "refine_math.h"

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

// ---- density control (PeriodicVibrationGaussians.refinement_after, pvg.py:148-265) ------------------------------------------------
// Per-row math of csrc/refine.hip's pvg_* kernels and of the host shim tests/hostmath_pvg_refine_shim.hip.  Every function keeps the
// reference's operations apart (no FMA contraction), as refine_classify does: the decisions compare float32 values.  What a split does
// in every class -- the 1 / 1.6 shrink, the sample's rotation, R (scale * noise) + mean -- is csrc/refine_math.h.

// what a row's decision is made of; thresholds that the reference forms from Python floats are formed in double and rounded once
struct PvgRefineCfg {
  float grad_thresh, t_grad_thresh;   // densify_grad_thresh, densify_t_grad_thresh
  float size_thresh;                  // densify_size_thresh * scene_scale
  float t_size_thresh;                // densify_t_size_thresh
  int split_by_screen;                // step < stop_screen_size_at
  float split_screen_size;
  float scene_scale, origin[3];       // gamma (pvg.py:90-98)
};

struct PvgCullCfg {
  float cull_alpha;
  int by_scale;                       // step > reset_alpha_interval
  float cull_scale;                   // cull_scale_thresh * scene_scale
  int by_screen;                      // by_scale and step < stop_screen_size_at
  float cull_screen;
  float scene_scale, origin[3];
};

enum PvgKind : unsigned char { kPvgKeepsScale = 1, kPvgKeepsBeta = 2 };   // second plan array: what a split's children do NOT shrink

// gamma (pvg.py:90-98): max(1, |mean - scene_origin| scene_scale - 1) / scene_scale
BDS_HD float pvg_gamma(const float *mean, const float *origin, float scene_scale) {
#pragma clang fp contract(off)
  const float x = mean[0] - origin[0], y = mean[1] - origin[1], z = mean[2] - origin[2];
  float g = sqrtf(x * x + y * y + z * z) * scene_scale - 1.0f;
  if (g <= 1.0f) g = 1.0f;            // torch.where(gamma <= 1, 1, gamma): a NaN stays
  return g / scene_scale;
}

// pvg.py:165-202.  Returns bit 0 split, bit 1 dup; *kind: kPvgKeepsScale when the (shrunk) parent is not over the size threshold
// (:339-342, evaluated after :323), kPvgKeepsBeta when its time scale is not over densify_t_size_thresh (:347).  The dup mask is
// evaluated after split_gaussians has shrunk EVERY split parent's scales in place (:323 runs before :195); betas are not shrunk.
BDS_HD unsigned pvg_refine_decide(const PvgRefineCfg &c, float xys_grad_norm, float t_grad_accum, float vis_count, float max_2Dsize,
                                  const float *log_scale, float beta, const float *mean, unsigned char *kind) {
#pragma clang fp contract(off)
  const bool high_xyz = (xys_grad_norm / vis_count) > c.grad_thresh;
  const bool high_t = (t_grad_accum / vis_count) > c.t_grad_thresh;
  const bool high = high_xyz || high_t;
  const float lmax = fmaxf(fmaxf(log_scale[0], log_scale[1]), log_scale[2]);
  const float smax = expf(lmax);      // exp is monotone: max_i exp(s_i) = exp(max_i s_i)
  const float thr = c.size_thresh * pvg_gamma(mean, c.origin, c.scene_scale);
  const float st = expf(beta);
  const bool big_t = st > c.t_size_thresh;
  bool split = (smax > thr) || (big_t && high_t);
  if (c.split_by_screen) split = split || (max_2Dsize > c.split_screen_size);
  split = split && high;
  const float s_post = split ? expf(refine_shrink_log(lmax)) : smax;
  const bool small_xyz = s_post <= thr, small_t = st <= c.t_size_thresh;
  const bool dup = (small_xyz || (small_t && high_t)) && high;
  *kind = (unsigned char)((small_xyz ? kPvgKeepsScale : 0) | (small_t ? kPvgKeepsBeta : 0));
  return (split ? 1u : 0u) | (dup ? 2u : 0u);
}

// what every child of one split parent shares (pvg.py:298-354): its log-scale and beta, and the parent's shrunk log-scale
struct PvgSplitRow {
  float R[9], scale[3];               // rotation; exp(scale BEFORE the shrink)
  float st, drift;                    // exp(beta); exp(-0.5 exp(beta) / T) of the velocity property (:83-88)
  float shrunk[3], child_scale[3], child_beta;
};

BDS_HD void pvg_split_row(const float *quat, const float *log_scale, float beta, float T, unsigned kind, int no_time_split, PvgSplitRow *o) {
#pragma clang fp contract(off)
  refine_split_rotation(quat, o->R);
  o->st = expf(beta);
  o->drift = expf(-0.5f * (o->st / T));
  for (int i = 0; i < 3; i++) {
    o->scale[i] = expf(log_scale[i]);
    o->shrunk[i] = refine_shrink_log(log_scale[i]);
    // :343-345 log(get_scaling) of the row the shrink has already rewritten
    o->child_scale[i] = (kind & kPvgKeepsScale) ? logf(expf(o->shrunk[i])) : o->shrunk[i];
  }
  o->child_beta = (no_time_split || (kind & kPvgKeepsBeta)) ? logf(o->st) : logf(o->st / 1.6f);
}

// one child: sample = {n_x, n_y, n_z, z_t} (:305 randn, :332 normal(0, std) = std z_t)
BDS_HD void pvg_split_child(const PvgSplitRow &r, const float *mean, const float *vel, float tau, const float *sample, float *o_mean,
                            float *o_tau) {
#pragma clang fp contract(off)
  const float samples_t = 0.0f + r.st * sample[3];
  float nm[3];
  refine_split_mean(r.R, r.scale, sample, mean, nm);
  for (int i = 0; i < 3; i++) o_mean[i] = nm[i] + (vel[i] * r.drift) * samples_t;
  *o_tau = samples_t + tau;
}

// cull_gaussians (pvg.py:267-284) of one row of the NEW set; max_2Dsize = 0 for a child
BDS_HD bool pvg_cull(const PvgCullCfg &c, float logit, const float *log_scale, const float *mean, float max_2Dsize) {
#pragma clang fp contract(off)
  bool cull = pvg_sigmoid(logit) < c.cull_alpha;
  if (c.by_scale) {
    const float smax = expf(fmaxf(fmaxf(log_scale[0], log_scale[1]), log_scale[2]));
    cull = cull || (smax > c.cull_scale * pvg_gamma(mean, c.origin, c.scene_scale));
    if (c.by_screen) cull = cull || (max_2Dsize > c.cull_screen);
  }
  return cull;
}

// after_train (pvg.py:100-133) of one kept row: the norm of the scaled 2-D gradient
BDS_HD float pvg_grad_norm(float gx, float gy, float sx, float sy) {
#pragma clang fp contract(off)
  const float x = gx * sx, y = gy * sy;
  return sqrtf(x * x + y * y);
}

// velocity_reg (pvg.py:430-435): |_velocity exp(-0.5 exp(beta) / T)| of one row
BDS_HD float pvg_velocity_norm(const float *vel, float beta, float T) {
  const float w = expf(-0.5f * (expf(beta) / T));
  const float x = vel[0] * w, y = vel[1] * w, z = vel[2] * w;
  return sqrtf(x * x + y * y + z * z);
}

// ... and its gradient times `go`: a zero velocity gets 0 (torch's norm backward), never 0 / 0
BDS_HD void pvg_velocity_norm_vjp(const float *vel, float beta, float T, float go, float *g_vel, float *g_beta) {
  const float st = expf(beta), w = expf(-0.5f * (st / T));
  const float x = vel[0] * w, y = vel[1] * w, z = vel[2] * w;
  const float n = sqrtf(x * x + y * y + z * z);
  if (n == 0.0f) {
    g_vel[0] = g_vel[1] = g_vel[2] = 0.0f;
    *g_beta = 0.0f;
    return;
  }
  const float s = go * w / n;         // d n / d vel_k = w (vel_k w) / n
  g_vel[0] = s * x; g_vel[1] = s * y; g_vel[2] = s * z;
  *g_beta = go * n * (-0.5f / T) * st;   // d n / d beta = n d log(w) / d beta
}

}  // namespace bds
