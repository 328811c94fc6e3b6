// TEST-ONLY host shim for rasterize_mode "antialiased": runs the projection VJP of csrc/gs_math.h with the compensation's gradient (project_one_vjp_aa)
// on the CPU, so that tests/test_antialiased_hostmath.py can compare it with the float64 oracle without a GPU.  Not part of
// libbds.so, never loaded by the product.
#include "../bilateral_driving_amd/csrc/gs_math.h"

using namespace bds;

// forward as the antialiased kernels run it: radii, means2d, depths, conics, comps
extern "C" void hm_aa_project_fwd(int n, const float *means, const float *quats, const float *scales, const float *viewmat,
                                  const float *K, int W, int H, float eps2d, int *radii, float *means2d, float *depths, float *conics,
                                  float *comps) {
  Camera cam = load_camera(viewmat, K);
  for (int i = 0; i < n; i++) {
    Proj p = project_one(means + i * 3, quats + i * 4, scales + i * 3, cam, W, H, eps2d, 0.01f, 1e10f, 0.f, /*kExactComp*/ true);
    radii[i] = p.radius; means2d[i * 2] = p.mx; means2d[i * 2 + 1] = p.my; depths[i] = p.depth;
    conics[i * 3] = p.ca; conics[i * 3 + 1] = p.cb; conics[i * 3 + 2] = p.cc; comps[i] = p.comp;
  }
}

// backward with v_comps; comps_vjp receives the compensation the VJP recomputes (what the list-driven backward multiplies v_eff by)
extern "C" void hm_aa_project_bwd(int n, const float *means, const float *quats, const float *scales, const float *viewmat,
                                  const float *K, int W, int H, float eps2d, const int *radii, const float *v_means2d,
                                  const float *v_depths, const float *v_conics, const float *v_comps, float *v_means, float *v_quats,
                                  float *v_scales, float *v_R /*9*/, float *v_t /*3*/, float *comps_vjp) {
  Camera cam = load_camera(viewmat, K);
  for (int k = 0; k < 9; k++) v_R[k] = 0.f;
  for (int k = 0; k < 3; k++) v_t[k] = 0.f;
  for (int i = 0; i < n; i++) {
    for (int k = 0; k < 3; k++) { v_means[i * 3 + k] = 0.f; v_scales[i * 3 + k] = 0.f; }
    for (int k = 0; k < 4; k++) v_quats[i * 4 + k] = 0.f;
    comps_vjp[i] = 0.f;
    if (radii[i] <= 0) continue;
    ProjGrad g;
    project_one_vjp_aa(means + i * 3, quats + i * 4, scales + i * 3, cam, W, H, eps2d, v_means2d[i * 2], v_means2d[i * 2 + 1],
                       v_depths[i], v_conics[i * 3], v_conics[i * 3 + 1], v_conics[i * 3 + 2], v_comps[i], g, comps_vjp + i);
    for (int k = 0; k < 3; k++) { v_means[i * 3 + k] = g.v_mean[k]; v_scales[i * 3 + k] = g.v_scale[k]; v_t[k] += g.v_t[k]; }
    for (int k = 0; k < 4; k++) v_quats[i * 4 + k] = g.v_quat[k];
    for (int k = 0; k < 9; k++) v_R[k] += g.v_R[k];
  }
}
