// Shared by the bilateral-grid translation units (csrc/bilagrid.hip: general kernels + host side; csrc/bilagrid_cells.hip: the
// cell-aligned kernels; csrc/bilagrid_tile.hip: the one-pass forward): launch parameter blocks, index helpers, the input-colour prologue
// (clamp + sky blend) with its backward, the forward kernels' pixel / loss epilogue and the staged trilinear sample.
#pragma once
#include "bds_common.h"
#include "bilagrid_math.h"

namespace bds {

constexpr int kBgBlock = 256;

struct LevelDev {
  const float *grid;   // [n_avg,12,gl,gy,gx]
  float *v_grid;
  float *lo;           // [Hd*Wd,12] low-res affine maps
  float *lg;           // [Hd*Wd] guidance (gray of the down-sampled input colour) of the low-res pixels, kept by the forward
  float *P;            // [H*W,3] input colour of this level                  (bwd scratch)
  float *Q;            // [H*W,3] gradient w.r.t. this level's output          (bwd scratch)
  float *R;            // [H*Wd,12] x-reduced adjoint of the up-sampler        (bwd scratch)
  float *vg;           // [Hd*Wd] gradient w.r.t. the low-res guidance (gray)  (bwd scratch)
  float *aff_out;      // optional [H*W,12]
  int gx, gy, gl, factor, n_avg, Hd, Wd;
  // resampling scales as torch forms them, divided ONCE on the host: up = low / full (taps of the up-sampler), dn = full / low
  float up_x, up_y, dn_x, dn_y;
  float lin_x, lin_y;  // 1 / (Wd - 1), 1 / (Hd - 1): step of torch.linspace(0, 1, n) over the low-res columns / rows
  uint32_t magic_wd;   // ceil(2^32 / Wd): row / column of a low-res index without an integer division (fast_divmod)
  int dn_shift;        // log2(factor) when the factor is a power of two >= 2 that divides H and W (else 0): the bilinear down-sampler
                       // then reads exactly the central 2 x 2 pixels of every factor x factor block with weight 1/4 each
};
struct MsParams {
  int nlevels, H, W;
  uint32_t magic_w;        // ceil(2^32 / W)
  int cs;                  // floats per pixel of `rgb` and of the returned colour gradient: 3, or 4 in the RGB+ED form
  const float *rgb, *alpha, *sky;
  float *depth_out;        // RGB+ED form: [H*W] expected depth = rgb[.,3] / max(alpha, 1e-10)
  const float *v_depth;    // RGB+ED form, backward: gradient of that depth (may be null)
  const float *v_alpha_in; // RGB+ED form, backward: gradient arriving at alpha from the caller (may be null)
  LevelDev lv[BDS_MAX_LEVELS];
};

// n / d and n % d for n < 2^31, d < 2^31 from magic = ceil(2^32 / d): the estimate is exact or one too large (a 64-bit division
// by a launch constant costs ~60 vector instructions per pixel in kernels that are bound by instruction issue)
__device__ __forceinline__ void fast_divmod(uint32_t n, uint32_t d, uint32_t magic, int &q, int &r) {
  uint32_t qq = d == 1u ? n : __umulhi(n, magic);
  int rr = (int)(n - qq * d);
  if (rr < 0) { qq--; rr += (int)d; }
  q = (int)qq; r = rr;
}
// 32-bit element offsets for the image-sized arrays (ms_fill requires 12 H W < 2^31): a 64-bit multiply-add per tap address
// (v_mad_u64_u32, quarter rate) was ~30 % of the full-resolution kernels' issue time.  Rows / columns are < 2^23, so row * width is
// one full-rate v_mul_i32_i24; the small constant factors are shift-adds.
__device__ __forceinline__ int row_major(int row, int width, int col) { return __mul24(row, width) + col; }
__device__ __forceinline__ int times3(int v) { return v + (v << 1); }
static inline uint32_t divmod_magic(int d) { return d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d); }

// Several levels in ONE launch: workgroup ranges per level (the levels are independent, each alone
// under-fills the chip, and a launch boundary costs ~1.5-2 us).
struct LevelSched {
  int n;                               // entries
  int level[BDS_MAX_LEVELS];           // level index of entry k
  int blk_off[BDS_MAX_LEVELS + 1];     // workgroups [blk_off[k], blk_off[k+1]) belong to entry k
  int nblk[BDS_MAX_LEVELS];            // = blk_off[k+1] - blk_off[k]
  long long part_off[BDS_MAX_LEVELS];  // float offset of the entry's partial-grid region
};
__device__ __forceinline__ int sched_find(const LevelSched &s, int bid, int &local) {
  int k = 0;
  while (k + 1 < s.n && bid >= s.blk_off[k + 1]) k++;
  local = bid - s.blk_off[k];
  return k;
}

// input colour of the transform at pixel (y,x): clamp + sky blend fused when sky != null
__device__ __forceinline__ void load_input(const MsParams &p, int y, int x, float &r, float &g, float &b) {
  const int o = row_major(y, p.W, x);
  const int oc = p.cs == 4 ? o << 2 : times3(o), o3 = times3(o);
  r = p.rgb[oc]; g = p.rgb[oc + 1]; b = p.rgb[oc + 2];
  if (p.sky) {
    const float k = 1.f - p.alpha[o];
    r = fminf(r, 1.f) + p.sky[o3] * k;
    g = fminf(g, 1.f) + p.sky[o3 + 1] * k;
    b = fminf(b, 1.f) + p.sky[o3 + 2] * k;
  }
}

// backward of load_input and of the expected depth next to it (RGB+ED form: cs == 4) at pixel `pix`, for the gradient v[3] of the
// transform's input colour: the final v_in (cs floats per pixel, at `oc`), and v_sky / v_alpha where the caller has them
__device__ __forceinline__ void input_backward_store(const MsParams &p, int pix, int oc, const float *v, float *__restrict__ v_in,
                                                     float *__restrict__ v_alpha, float *__restrict__ v_sky) {
  const int p3 = times3(pix);
  float vc[3] = {v[0], v[1], v[2]};
  float va = 0.f;
  if (p.sky) {
    const float colour[3] = {p.rgb[oc], p.rgb[oc + 1], p.rgb[oc + 2]}, sky[3] = {p.sky[p3], p.sky[p3 + 1], p.sky[p3 + 2]};
    const SkyGrad g = sky_clamp_backward(v, colour, p.alpha[pix], sky);
    if (v_sky) { v_sky[p3] = g.v_sky[0]; v_sky[p3 + 1] = g.v_sky[1]; v_sky[p3 + 2] = g.v_sky[2]; }
    vc[0] = g.v[0]; vc[1] = g.v[1]; vc[2] = g.v[2];
    va = g.alpha_add;
  }
  v_in[oc] = vc[0]; v_in[oc + 1] = vc[1]; v_in[oc + 2] = vc[2];
  if (p.cs == 4) {   // plus the caller's own alpha gradient
    const EdGrad e = expected_depth_backward(p.rgb[(pix << 2) + 3], p.alpha[pix], p.v_depth ? p.v_depth[pix] : 0.f);
    v_in[(pix << 2) + 3] = e.v_D;
    if (p.v_alpha_in) va += p.v_alpha_in[pix];
    va -= e.alpha_sub;
    if (v_alpha) v_alpha[pix] = va;
  } else if (p.sky && v_alpha) {
    v_alpha[pix] = va;
  }
}

__device__ __forceinline__ void lowres_colour(const MsParams &p, const Tap &ty, const Tap &tx, float &r, float &g, float &b) {
  float r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11;
  load_input(p, ty.i0, tx.i0, r00, g00, b00);
  load_input(p, ty.i0, tx.i1, r01, g01, b01);
  load_input(p, ty.i1, tx.i0, r10, g10, b10);
  load_input(p, ty.i1, tx.i1, r11, g11, b11);
  const float wx = tx.w1, wy = ty.w1;
  r = (r00 * (1.f - wx) + r01 * wx) * (1.f - wy) + (r10 * (1.f - wx) + r11 * wx) * wy;
  g = (g00 * (1.f - wx) + g01 * wx) * (1.f - wy) + (g10 * (1.f - wx) + g11 * wx) * wy;
  b = (b00 * (1.f - wx) + b01 * wx) * (1.f - wy) + (b10 * (1.f - wx) + b11 * wx) * wy;
}

// ---- TV of several grid pyramids' levels in ONE launch each way (the levels are tiny: a launch costs more than a level) ----
struct TvLevels {
  int n;
  const float *x[BDS_MAX_LEVELS];
  float *v_x[BDS_MAX_LEVELS];
  long long total[BDS_MAX_LEVELS];
  int gx[BDS_MAX_LEVELS], gy[BDS_MAX_LEVELS], gl[BDS_MAX_LEVELS];
  float sl[BDS_MAX_LEVELS], sy[BDS_MAX_LEVELS], sx[BDS_MAX_LEVELS];
  int blk_off[BDS_MAX_LEVELS + 1];
};

// value and gradient of the TV term at the element (level by workgroup, element by thread) that workgroup `bid` of a
// T.blk_off[T.n]-workgroup range owns: returns its share of the value, ADDS v_loss * d(TV)/d(element) to the level's gradient slice
__device__ __forceinline__ float tv_train_element(const TvLevels &L, int bid, float v_loss) {
  int k = 0;
  while (k + 1 < L.n && bid >= L.blk_off[k + 1]) k++;
  const int64_t e = (int64_t)(bid - L.blk_off[k]) * kBgBlock + threadIdx.x;
  float acc = 0.f;
  if (e < L.total[k]) {
    const int gx = L.gx[k], gy = L.gy[k], gl = L.gl[k];
    const float *x = L.x[k];
    const int ix = (int)(e % gx), iy = (int)((e / gx) % gy), il = (int)((e / ((int64_t)gx * gy)) % gl);
    const int64_t sl = (int64_t)gx * gy;
    const float v = x[e];
    float g = 0.f;
    if (ix > 0) { const float d = v - x[e - 1]; acc += d * d * L.sx[k]; g += 2.f * d * L.sx[k]; }
    if (ix < gx - 1) g -= 2.f * (x[e + 1] - v) * L.sx[k];
    if (iy > 0) { const float d = v - x[e - gx]; acc += d * d * L.sy[k]; g += 2.f * d * L.sy[k]; }
    if (iy < gy - 1) g -= 2.f * (x[e + gx] - v) * L.sy[k];
    if (il > 0) { const float d = v - x[e - sl]; acc += d * d * L.sl[k]; g += 2.f * d * L.sl[k]; }
    if (il < gl - 1) g -= 2.f * (x[e + sl] - v) * L.sl[k];
    if (L.v_x[k]) atomicAdd(L.v_x[k] + e, g * v_loss);
  }
  return acc;
}

// the training loss folded into the full-resolution forward (bds_bilagrid_ms_fwd with a `target`): L1 against `target` over the pixels this
// launch produces, TV of the grids by tv_blocks extra workgroups behind the pix_blocks pixel workgroups
constexpr int kLossSlotStride = BDS_LOSS_SLOT_STRIDE;   // floats between two slots: every slot in a 256-byte segment of its own
struct TrainLoss {
  const float *target;   // [H,W,3]
  float *v_out;          // [H,W,3]  sign(out - target) * v_loss / (3 H W)
  float *loss;           // [loss_slots * kLossSlotStride], zeroed by the caller: slot (workgroup % loss_slots) += its share of
                         // mean|out - target| + TV terms.  (8100 float atomics on ONE address cost 65 us at the end of the launch.)
  int loss_slots;        // power of two
  float inv_n, v_loss;
  int pix_blocks, tv_blocks;
  TvLevels T;
};

__device__ __forceinline__ float block_sum_to_thread0(float acc, float *red /* [kBgBlock / kWave] shared */) {
  acc = wave_sum_all(acc);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int w = 0; w < kBgBlock / kWave; w++) t += red[w];
  return t;
}

// ---- the loss epilogue of the three full-resolution forward kernels, in three pieces -----------------------------------------------
// thread 0's block sum `t` into the workgroup's loss slot
__device__ __forceinline__ void loss_commit(const TrainLoss &tl, float t) {
  if (threadIdx.x == 0 && t != 0.f) atomicAdd(tl.loss + (size_t)(blockIdx.x & (tl.loss_slots - 1)) * kLossSlotStride, t);
}
// the workgroups behind the pixel workgroups own the TV term of the loss, one grid element per thread: true = this was one of them
template <bool kTrain>
__device__ __forceinline__ bool train_tv_workgroup(const TrainLoss &tl, float *red) {
  if (!kTrain || (int)blockIdx.x < tl.pix_blocks) return false;
  loss_commit(tl, block_sum_to_thread0(tv_train_element(tl.T, (int)blockIdx.x - tl.pix_blocks, tl.v_loss), red));
  return true;
}
// pixel `pix` leaves the transform as (r, g, b): store it, the expected depth next to it (RGB+ED form) and, training, the gradient
// of the photometric L1 against the target; returns the pixel's L1
template <bool kTrain>
__device__ __forceinline__ float emit_pixel(const MsParams &p, const TrainLoss &tl, float *__restrict__ out, int pix, float r, float g,
                                            float b) {
  const int p3 = times3(pix);
  out[p3] = r; out[p3 + 1] = g; out[p3 + 2] = b;
  if (p.depth_out) p.depth_out[pix] = expected_depth(p.rgb[(pix << 2) + 3], p.alpha[pix]);
  if (!kTrain) return 0.f;
  const float gs = tl.v_loss * tl.inv_n;
  const float d0 = r - tl.target[p3], d1 = g - tl.target[p3 + 1], d2 = b - tl.target[p3 + 2];
  tl.v_out[p3] = sign_scaled(d0, gs); tl.v_out[p3 + 1] = sign_scaled(d1, gs); tl.v_out[p3 + 2] = sign_scaled(d2, gs);
  return fabsf(d0) + fabsf(d1) + fabsf(d2);
}
// the workgroup's L1 sum into its loss slot (contains a barrier: every thread of the workgroup calls it)
__device__ __forceinline__ void l1_commit(const TrainLoss &tl, float l1, float *red) {
  loss_commit(tl, block_sum_to_thread0(l1, red) * tl.inv_n);
}

// ---- trilinear sample of the 12 channels from a STAGED copy of the grid ([node][12] as three float4) --------------------------------
// g0 / g1: the two guidance planes; o..: float4 offsets of the cell's four corners; w..: their in-plane weights (corner_weights).
// slice_sample_n's order.  Load: how a 16-byte read is made.
struct LoadPlain {
  static __device__ __forceinline__ float4 ld(const float4 *p) { return *p; }
};
// a 16-byte LDS read the compiler may not narrow: where a component of the result is unused it splits the access into ds_read_b96 +
// ds_read2_b32 (8 + 4 LDS cycles instead of 4: measured as the first cost of the cell-aligned backward, which is bound by the LDS pipeline)
struct LoadLds16 {
  static __device__ __forceinline__ float4 ld(const float4 *p) {
    float4 v = *p;
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
  }
};
template <bool kOut, bool kDz, class Load = LoadPlain>
__device__ __forceinline__ void trilinear12(const float4 *__restrict__ g0, const float4 *__restrict__ g1, int o00, int o01, int o10, int o11,
                                            float w00, float w01, float w10, float w11, float fz, float *out12, float *dz12) {
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const float4 a00 = Load::ld(g0 + o00 + q), a01 = Load::ld(g0 + o01 + q), a10 = Load::ld(g0 + o10 + q), a11 = Load::ld(g0 + o11 + q);
    const float4 b00 = Load::ld(g1 + o00 + q), b01 = Load::ld(g1 + o01 + q), b10 = Load::ld(g1 + o10 + q), b11 = Load::ld(g1 + o11 + q);
    const float a[4] = {a00.x * w00 + a01.x * w01 + a10.x * w10 + a11.x * w11, a00.y * w00 + a01.y * w01 + a10.y * w10 + a11.y * w11,
                        a00.z * w00 + a01.z * w01 + a10.z * w10 + a11.z * w11, a00.w * w00 + a01.w * w01 + a10.w * w10 + a11.w * w11};
    const float b[4] = {b00.x * w00 + b01.x * w01 + b10.x * w10 + b11.x * w11, b00.y * w00 + b01.y * w01 + b10.y * w10 + b11.y * w11,
                        b00.z * w00 + b01.z * w01 + b10.z * w10 + b11.z * w11, b00.w * w00 + b01.w * w01 + b10.w * w10 + b11.w * w11};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (kOut) out12[q * 4 + k] = a[k] * (1.f - fz) + b[k] * fz;
      if (kDz) dz12[q * 4 + k] = b[k] - a[k];
    }
  }
}
// ---- cell-aligned kernels (csrc/bilagrid_cells.hip) -------------------------------------------------------------------------
// A level qualifies when it has ONE grid (n_avg == 1) with gl <= kCellMaxGl planes; its low-resolution pixels are then processed
// in jobs that lie inside ONE (y, x) cell of the grid.
constexpr int kCellMaxGl = 8;
inline bool cells_level_ok(const LevelDev &L) { return L.n_avg == 1 && L.gl >= 1 && L.gl <= kCellMaxGl; }
// whole transform in one launch each way: one level at full resolution (BilateralAffineTransform, models/modules.py:317-346)
inline bool cells_fused_ok(const MsParams &p) {
  return p.nlevels == 1 && p.lv[0].Hd == p.H && p.lv[0].Wd == p.W && cells_level_ok(p.lv[0]) && p.lv[0].aff_out == nullptr;
}
// low-resolution stage of the levels in `mask` (bit l): slice -> lo, lg | y pass of the up-sampler adjoint + slice vjp -> v_grid, vg
int cells_lowres_fwd(const MsParams &p, unsigned mask, hipStream_t st);
int cells_lowres_bwd(const MsParams &p, unsigned mask, hipStream_t st);
// single full-resolution level: slice + apply (+ L1 / TV loss) | the whole backward
int cells_fused_fwd(const MsParams &p, float *out, const TrainLoss *train, hipStream_t st);
int cells_fused_bwd(const MsParams &p, const float *v_out, float *v_in, float *v_alpha, float *v_sky, hipStream_t st);
// pyramid forward in one pass over the image (csrc/bilagrid_tile.hip): every factor a power of two >= 2 dividing the image
bool tile_fwd_ok(const MsParams &p);
int tile_fwd(const MsParams &p, float *out, const TrainLoss *train, hipStream_t st);

}  // namespace bds
