// The last stage of the colour transform's backward -- guidance route added to the direct route, clamp(max=1) / sky blend /
// expected-depth backward (csrc/bilagrid.hip ms_guidance_blend_bwd_kernel, csrc/bilagrid_ms.h input_backward_store; models/trainers/base.py:414-419,
// trainers/scene_graph.py:292-294) -- in a form the compositor's backward can run per pixel while it loads its tile: the per-pixel
// result (v_render [4], v_alpha) is then never written to memory and read back, and one launch over the image disappears.
#pragma once
#include "bds_common.h"
#include "bilagrid_math.h"

namespace bds {

struct EdEpilogue {
  int nlevels, W;
  const float *vg[BDS_MAX_LEVELS];   // [Hd*Wd] gradient w.r.t. the low-res guidance of every level (csrc/bilagrid_cells.hip)
  int Wd[BDS_MAX_LEVELS];
  int shift[BDS_MAX_LEVELS];         // log2(factor) of a dividing power-of-two factor; 0: the level works at full resolution
  const float *v_direct;             // [H*W,4] direct-route gradient of the transform's input colour (channels 0-2)
  const float *render;               // [H*W,4] the compositor's forward output (colour before the clamp | D)
  const float *sky;                  // [H*W,3] or null
  const float *v_depth;              // [H*W] or null: gradient of the expected depth D / max(alpha, 1e-10)
  const float *v_alpha_in;           // [H*W] or null: the caller's own gradient of alpha
  float *v_sky;                      // [H*W,3] or null (out)
};

// Guidance adjoint of a level whose power-of-two factor f = 2^shift divides the image: low-res pixel (i, j) was sampled at
// f (i + 1/2) - 1/2, i.e. from the two central rows / columns of its f x f block with weights 1/2, 1/2 -- pixel (y, x) receives 1/4
// of ONE low-res value of vg [., Wd], or nothing
__device__ __forceinline__ void guidance_tap_pow2(float &acc, const float *__restrict__ vg, int Wd, int shift, int y, int x) {
  const int f = 1 << shift, h = f >> 1, fy = y & (f - 1), fx = x & (f - 1);
  if ((fy == h - 1 || fy == h) && (fx == h - 1 || fx == h)) acc += (0.5f * 0.5f) * vg[__mul24(y >> shift, Wd) + (x >> shift)];
}

// v_render[0..3] and v_alpha of pixel (y, x) with opacity `alpha`; writes v_sky
__device__ __forceinline__ void ed_epilogue_pixel(const EdEpilogue &e, int y, int x, int pix, float alpha, float *vr4, float &v_alpha) {
  float vg = 0.f;
#pragma unroll
  for (int l = 0; l < BDS_MAX_LEVELS; l++) {
    if (l >= e.nlevels) break;
    if (e.shift[l] == 0) vg += e.vg[l][pix];
    else guidance_tap_pow2(vg, e.vg[l], e.Wd[l], e.shift[l], y, x);
  }
  const float4 d = reinterpret_cast<const float4 *>(e.v_direct)[pix];
  const float4 r = reinterpret_cast<const float4 *>(e.render)[pix];
  const float v[3] = {d.x + vg * kGrayR, d.y + vg * kGrayG, d.z + vg * kGrayB};
  vr4[0] = v[0]; vr4[1] = v[1]; vr4[2] = v[2];
  float va = 0.f;
  if (e.sky) {
    const int p3 = pix * 3;
    const float rgb[3] = {r.x, r.y, r.z}, sky[3] = {e.sky[p3], e.sky[p3 + 1], e.sky[p3 + 2]};
    const SkyGrad g = sky_clamp_backward(v, rgb, alpha, sky);
    if (e.v_sky) { e.v_sky[p3] = g.v_sky[0]; e.v_sky[p3 + 1] = g.v_sky[1]; e.v_sky[p3 + 2] = g.v_sky[2]; }
    vr4[0] = g.v[0]; vr4[1] = g.v[1]; vr4[2] = g.v[2];
    va = g.alpha_add;
  }
  const EdGrad g = expected_depth_backward(r.w, alpha, e.v_depth ? e.v_depth[pix] : 0.f);
  if (e.v_alpha_in) va += e.v_alpha_in[pix];
  vr4[3] = g.v_D;
  v_alpha = va - g.alpha_sub;
}

// fills `e` from the transform's level list and workspace (csrc/bilagrid.hip); BDS_EINVAL when the configuration cannot defer
int ed_epilogue_fill(int nlevels, const bds_bilagrid_level_t *levels, int H, int W, void *ws, size_t ws_bytes, EdEpilogue *e);

}  // namespace bds
