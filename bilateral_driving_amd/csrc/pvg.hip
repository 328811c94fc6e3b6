// Time transform of the periodic-vibration Gaussians (PeriodicVibrationGaussians.get_gaussians, models/gaussians/pvg.py:374-425): the
// five tensors the rasterizer takes, for the rows whose marginal exceeds 0.05 only, compacted in the original order (the
// reference's x[filter_mask]), with the NaN / Inf flags of those tensors.  The per-row math lives in pvg_math.h.
//   forward, three launches:
//     count  one thread per row: marg, the keep byte (the bool mask) and the kept rows per 256-row block (ballot + popcount);
//     scan   one workgroup: exclusive scan of the block counts in place (any number of blocks: scan.h); M and the cleared flag word
//            go to the workspace header;
//     write  one thread per row: rank = block offset + waves in front + mbcnt of the wave's ballot; a kept row computes its outputs
//            and stores them at its rank, and ORs its NaN / Inf bits into the header (integer, only when a value is not finite).
//   backward, one launch over the N rows: the rank is formed the same way, the output gradients are read by rank, every row of the
//     nine parameter gradients is stored (zeros for a dropped row).  No atomics: bit-identical run to run.
// Everything is streamed once: non-temporal loads and stores, as the dense Adam pass (csrc/optim.hip).
#include "bds_common.h"
#include "pvg_math.h"
#include "scan.h"

namespace bds {

constexpr int kPvgBlock = 256;                       // 4 waves
constexpr int kPvgWaves = kPvgBlock / kWave;
constexpr int kPvgHeader = 4;                        // workspace words in front of the block table: {M, flags, -, -}

typedef float pvg_f4u __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at 4-byte alignment (rows of 3 (K-1) floats)

__device__ __forceinline__ float pvg_ld(const float *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void pvg_st(float *p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void pvg_ld_n(const float *__restrict__ p, float *o, int n) {
  for (int k = 0; k < n; k++) o[k] = pvg_ld(p + k);
}
__device__ __forceinline__ void pvg_st_n(float *__restrict__ p, const float *v, int n) {
  for (int k = 0; k < n; k++) pvg_st(p + k, v[k]);
}

__global__ __launch_bounds__(kPvgBlock) void pvg_count_kernel(int64_t N, float cur_time, const float *__restrict__ taus,
                                                             const float *__restrict__ betas, uint8_t *__restrict__ mask,
                                                             uint32_t *__restrict__ counts) {
  __shared__ uint32_t s_cnt[kPvgWaves];
  const int64_t p = (int64_t)blockIdx.x * kPvgBlock + threadIdx.x;
  bool keep = false;
  if (p < N) {
    keep = pvg_marginal(pvg_ld(taus + p), pvg_ld(betas + p), cur_time) > kPvgKeep;    // (false for NaN)
    mask[p] = keep ? 1 : 0;
  }
  const uint32_t total = block_count<1, kPvgWaves>(keep, s_cnt);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[nb] -> exclusive offsets in place; header = {M, 0 (flags), 0, 0}
__global__ __launch_bounds__(kPvgBlock) void pvg_scan_kernel(int64_t nb, uint32_t *__restrict__ header, uint32_t *__restrict__ counts) {
  __shared__ uint32_t lw[kPvgWaves];
  uint32_t M;
  workgroup_scan_in_place<kPvgBlock>(counts, nb, &M, lw);
  if (threadIdx.x < kPvgHeader) header[threadIdx.x] = threadIdx.x == 0 ? M : 0u;
}

// bit 2 i: NaN in tensor i, bit 2 i + 1: Inf in tensor i (i in the order of get_gaussians' dict: means, opacities, rgbs, scales, quats)
__device__ __forceinline__ uint32_t pvg_bits(const float *v, int n, int i) {
  uint32_t r = 0;
  for (int k = 0; k < n; k++) r |= (isnan(v[k]) ? 1u : 0u) | (isinf(v[k]) ? 2u : 0u);
  return r << (2 * i);
}

// The SH colour of a kept row from the split storage (features_dc [N,3], features_rest [N,K-1,3]), accumulated piece by piece:
// 16-byte loads at 4-byte alignment (unaligned vector access is on for gfx950 compute); raw = before + 0.5 and the clamp.
template <int MODE>
__device__ __forceinline__ void pvg_colour(int64_t p, int K, const float *__restrict__ dc, const float *__restrict__ rest,
                                           const float *o_mean, const float *cam, float *raw) {
  float c0[3];
  pvg_ld_n(dc + p * 3, c0, 3);
  if (MODE == kPvgSigmoid) {
    for (int k = 0; k < 3; k++) raw[k] = c0[k];
    return;
  }
  constexpr int deg = MODE == kPvgSigmoid ? 0 : MODE;
  constexpr int nb = (deg + 1) * (deg + 1), nr = (nb - 1) * 3;     // bases used, floats of `rest` used
  float B[16];
  pvg_bases(deg, o_mean, cam, B);
  for (int k = 0; k < 3; k++) raw[k] = B[0] * c0[k];
  if (nr == 0) return;
  float cf[nr > 0 ? nr : 1];
  const float *r = rest + p * (int64_t)(K - 1) * 3;
#pragma unroll
  for (int i = 0; i + 4 <= nr; i += 4) {
    const pvg_f4u u = __builtin_nontemporal_load(reinterpret_cast<const pvg_f4u *>(r + i));
    cf[i] = u.x; cf[i + 1] = u.y; cf[i + 2] = u.z; cf[i + 3] = u.w;
  }
#pragma unroll
  for (int i = nr / 4 * 4; i < nr; i++) cf[i] = pvg_ld(r + i);
#pragma unroll
  for (int b = 1; b < nb; b++)
    for (int k = 0; k < 3; k++) raw[k] += B[b] * cf[(b - 1) * 3 + k];
}

template <int MODE>
// (second launch bound: 8 waves per SIMD, i.e. at most 64 VGPRs -- the degree 2 / 3 forms otherwise land a few registers above)
__global__ __launch_bounds__(kPvgBlock, 8) void pvg_write_kernel(int64_t N, int K, PvgTime t, const float *__restrict__ means,
                                                             const float *__restrict__ velocity, const float *__restrict__ taus,
                                                             const float *__restrict__ betas, const float *__restrict__ logits,
                                                             const float *__restrict__ log_scales, const float *__restrict__ quats,
                                                             const float *__restrict__ dc, const float *__restrict__ rest,
                                                             const float *__restrict__ cam_pos, const uint8_t *__restrict__ mask,
                                                             const uint32_t *__restrict__ offsets, uint32_t *__restrict__ header,
                                                             float *__restrict__ o_means, float *__restrict__ o_opac,
                                                             float *__restrict__ o_rgbs, float *__restrict__ o_scales,
                                                             float *__restrict__ o_quats, float *__restrict__ o_raw) {
  __shared__ uint32_t s_cnt[kPvgWaves];
  const int64_t p = (int64_t)blockIdx.x * kPvgBlock + threadIdx.x;
  const bool keep = p < N && mask[p] != 0;
  uint32_t rank;
  block_rank<1>(keep, &rank, s_cnt);
  const int64_t r = (int64_t)offsets[blockIdx.x] + rank;
  if (!keep) return;
  // the means and the colour first, stored before the other parameters are loaded: fewer values live at once (the degree-3 form
  // holds 45 coefficients and 16 bases)
  float m[3], v[3], om[3], raw[3], rgb[3];
  pvg_ld_n(means + p * 3, m, 3);
  pvg_ld_n(velocity + p * 3, v, 3);
  const float tau = pvg_ld(taus + p), beta = pvg_ld(betas + p);
  pvg_means(t, m, v, tau, beta, om);
  const float cam[3] = {cam_pos[0], cam_pos[1], cam_pos[2]};
  pvg_colour<MODE>(p, K, dc, rest, om, cam, raw);
  for (int k = 0; k < 3; k++) rgb[k] = MODE == kPvgSigmoid ? pvg_sigmoid(raw[k]) : pvg_clamp01(raw[k] + 0.5f);
  pvg_st_n(o_means + r * 3, om, 3);
  pvg_st_n(o_rgbs + r * 3, rgb, 3);
  pvg_st_n(o_raw + r * 3, raw, 3);
  uint32_t bits = pvg_bits(om, 3, 0) | pvg_bits(rgb, 3, 2);
  float ls[3], q[4], os[3], oq[4], oo;
  pvg_ld_n(log_scales + p * 3, ls, 3);
  pvg_ld_n(quats + p * 4, q, 4);
  pvg_activations(pvg_ld(logits + p), ls, q, pvg_marginal(tau, beta, t.cur_time), &oo, os, oq);
  pvg_st(o_opac + r, oo);
  pvg_st_n(o_scales + r * 3, os, 3);
  pvg_st_n(o_quats + r * 4, oq, 4);
  bits |= pvg_bits(&oo, 1, 1) | pvg_bits(os, 3, 3) | pvg_bits(oq, 4, 4);
  if (bits) atomicOr(header + 1, bits);
}

template <int MODE>
__global__ __launch_bounds__(kPvgBlock) void pvg_bwd_kernel(int64_t N, int K, PvgTime t, const float *__restrict__ velocity,
                                                           const float *__restrict__ taus, const float *__restrict__ betas,
                                                           const float *__restrict__ logits, const float *__restrict__ log_scales,
                                                           const float *__restrict__ quats, const float *__restrict__ cam_pos,
                                                           const uint8_t *__restrict__ mask, const uint32_t *__restrict__ offsets,
                                                           const float *__restrict__ o_means, const float *__restrict__ o_raw,
                                                           const float *__restrict__ v_om, const float *__restrict__ v_oo,
                                                           const float *__restrict__ v_orgb, const float *__restrict__ v_os,
                                                           const float *__restrict__ v_oq, float *__restrict__ g_means,
                                                           float *__restrict__ g_vel, float *__restrict__ g_taus,
                                                           float *__restrict__ g_betas, float *__restrict__ g_logits,
                                                           float *__restrict__ g_ls, float *__restrict__ g_quats,
                                                           float *__restrict__ g_dc, float *__restrict__ g_rest) {
  __shared__ uint32_t s_cnt[kPvgWaves];
  const int64_t p = (int64_t)blockIdx.x * kPvgBlock + threadIdx.x;
  const bool keep = p < N && mask[p] != 0;
  uint32_t rank;
  block_rank<1>(keep, &rank, s_cnt);
  const int64_t r = (int64_t)offsets[blockIdx.x] + rank;
  if (p >= N) return;
  float gm[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
  float gt = 0.f, gb = 0.f, gl = 0.f, vc[3] = {0.f, 0.f, 0.f}, B[16];
  for (int k = 0; k < 16; k++) B[k] = 0.f;
  if (keep) {
    float v[3], ls[3], q[4], vs[3], vq[4], om[3], raw[3], vrgb[3];
    pvg_ld_n(velocity + p * 3, v, 3);
    pvg_ld_n(log_scales + p * 3, ls, 3);
    pvg_ld_n(quats + p * 4, q, 4);
    pvg_ld_n(v_om + r * 3, gm, 3);
    pvg_ld_n(v_os + r * 3, vs, 3);
    pvg_ld_n(v_oq + r * 4, vq, 4);
    pvg_ld_n(v_orgb + r * 3, vrgb, 3);
    pvg_ld_n(o_raw + r * 3, raw, 3);
    pvg_backward(t, v, pvg_ld(taus + p), pvg_ld(betas + p), pvg_ld(logits + p), ls, q, gm, pvg_ld(v_oo + r), vs, vq, gv, &gt, &gb, &gl, gs,
                 gq);
    if (MODE == kPvgSigmoid) {
      for (int k = 0; k < 3; k++) {
        const float sg = pvg_sigmoid(raw[k]);
        gc[k] = vrgb[k] * sg * (1.0f - sg);
      }
    } else {
      pvg_ld_n(o_means + r * 3, om, 3);
      const float cam[3] = {cam_pos[0], cam_pos[1], cam_pos[2]};
      pvg_bases(MODE, om, cam, B);
      for (int k = 0; k < 3; k++) {
        vc[k] = pvg_clamp_grad(raw[k], vrgb[k]);
        gc[k] = B[0] * vc[k];
      }
    }
  }
  pvg_st_n(g_means + p * 3, gm, 3);
  pvg_st_n(g_vel + p * 3, gv, 3);
  pvg_st(g_taus + p, gt);
  pvg_st(g_betas + p, gb);
  pvg_st(g_logits + p, gl);
  pvg_st_n(g_ls + p * 3, gs, 3);
  pvg_st_n(g_quats + p * 4, gq, 4);
  pvg_st_n(g_dc + p * 3, gc, 3);
  // the whole row of v_features_rest: the bases in use times the colour gradient, zeros behind them and in a dropped row
  constexpr int nb = MODE == kPvgSigmoid ? 1 : (MODE + 1) * (MODE + 1);
  const int nr = (K - 1) * 3;
  float *gr = g_rest + p * (int64_t)nr;
#pragma unroll
  for (int i = 0; i < 48; i += 4) {
    if (i >= nr) continue;
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int e = i + j, b = e / 3 + 1;      // (compile-time after unrolling)
      w[j] = b < nb ? B[b < 16 ? b : 0] * vc[e % 3] : 0.f;
    }
    if (i + 4 <= nr) {
      pvg_f4u u;
      u.x = w[0]; u.y = w[1]; u.z = w[2]; u.w = w[3];
      __builtin_nontemporal_store(u, reinterpret_cast<pvg_f4u *>(gr + i));
    } else {
      for (int j = 0; j < 4; j++)
        if (i + j < nr) pvg_st(gr + i + j, w[j]);
    }
  }
}

static size_t pvg_temp_bytes(int64_t N) { return align_up((size_t)(kPvgHeader + cdiv(N, kPvgBlock)) * sizeof(uint32_t), 256); }
static bool pvg_k_ok(int K) { return K == 1 || K == 4 || K == 9 || K == 16; }

}  // namespace bds

using namespace bds;

extern "C" size_t bds_pvg_temp_bytes(int64_t N) { return N > 0 ? pvg_temp_bytes(N) : 0; }

static int pvg_mode(int K, int degrees_to_use) { return K == 1 ? kPvgSigmoid : degrees_to_use; }
static PvgTime pvg_time(float cur_time, float delta_t, int in_smooth, double T) {
  PvgTime t;
  t.cur_time = cur_time;
  t.delta_t = delta_t;
  t.T = (float)T;
  t.a = (float)(1.0 / T * 3.141592653589793 * 2.0);
  t.smooth = in_smooth ? 1 : 0;
  return t;
}

extern "C" int bds_pvg_fwd(int64_t N, int K, int degrees_to_use, float cur_time, float delta_t, int in_smooth, double T, const float *means,
                           const float *velocity, const float *taus, const float *betas, const float *logits, const float *log_scales,
                           const float *quats, const float *features_dc, const float *features_rest, const float *cam_pos,
                           float *out_means, float *out_opacities, float *out_rgbs, float *out_scales, float *out_quats, float *out_sh_raw,
                           uint8_t *filter_mask, void *temp, size_t temp_bytes, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N <= INT32_MAX && pvg_k_ok(K) && degrees_to_use >= 0 && (degrees_to_use + 1) * (degrees_to_use + 1) <= K);
  BDS_REQUIRE(T > 0.0 && (float)T > 0.0f);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(means && velocity && taus && betas && logits && log_scales && quats && features_dc && (features_rest || K == 1) && cam_pos);
  BDS_REQUIRE(out_means && out_opacities && out_rgbs && out_scales && out_quats && out_sh_raw && filter_mask);
  BDS_REQUIRE(temp && aligned16(temp) && temp_bytes >= pvg_temp_bytes(N));
  hipStream_t st = as_stream(stream);
  uint32_t *header = static_cast<uint32_t *>(temp), *table = header + kPvgHeader;
  const int64_t nb = cdiv(N, kPvgBlock);
  const dim3 grid((unsigned)nb), block(kPvgBlock);
  const PvgTime t = pvg_time(cur_time, delta_t, in_smooth, T);
  hipLaunchKernelGGL(pvg_count_kernel, grid, block, 0, st, N, cur_time, taus, betas, filter_mask, table);
  BDS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pvg_scan_kernel, dim3(1), block, 0, st, nb, header, table);
  BDS_LAUNCH_CHECK();
#define BDS_PVG_WRITE(M)                                                                                                                \
  hipLaunchKernelGGL((pvg_write_kernel<M>), grid, block, 0, st, N, K, t, means, velocity, taus, betas, logits, log_scales, quats,       \
                     features_dc, features_rest, cam_pos, (const uint8_t *)filter_mask, (const uint32_t *)table, header, out_means,     \
                     out_opacities, out_rgbs, out_scales, out_quats, out_sh_raw)
  switch (pvg_mode(K, degrees_to_use)) {
    case 0: BDS_PVG_WRITE(0); break;
    case 1: BDS_PVG_WRITE(1); break;
    case 2: BDS_PVG_WRITE(2); break;
    case 3: BDS_PVG_WRITE(3); break;
    default: BDS_PVG_WRITE(kPvgSigmoid); break;
  }
#undef BDS_PVG_WRITE
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_pvg_bwd(int64_t N, int64_t M, int K, int degrees_to_use, float cur_time, float delta_t, int in_smooth, double T,
                           const float *velocity, const float *taus, const float *betas, const float *logits, const float *log_scales,
                           const float *quats, const float *cam_pos, const uint8_t *filter_mask, const void *temp, size_t temp_bytes,
                           const float *out_means, const float *out_sh_raw, const float *v_out_means, const float *v_out_opacities,
                           const float *v_out_rgbs, const float *v_out_scales, const float *v_out_quats, float *v_means, float *v_velocity,
                           float *v_taus, float *v_betas, float *v_logits, float *v_log_scales, float *v_quats, float *v_features_dc,
                           float *v_features_rest, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && N <= INT32_MAX && M >= 0 && M <= N && pvg_k_ok(K) && degrees_to_use >= 0 &&
              (degrees_to_use + 1) * (degrees_to_use + 1) <= K);
  BDS_REQUIRE(T > 0.0 && (float)T > 0.0f);
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(velocity && taus && betas && logits && log_scales && quats && cam_pos && filter_mask);
  BDS_REQUIRE(M == 0 || (out_means && out_sh_raw && v_out_means && v_out_opacities && v_out_rgbs && v_out_scales && v_out_quats));
  BDS_REQUIRE(v_means && v_velocity && v_taus && v_betas && v_logits && v_log_scales && v_quats && v_features_dc && (v_features_rest || K == 1));
  BDS_REQUIRE(temp && aligned16(temp) && temp_bytes >= pvg_temp_bytes(N));
  const uint32_t *table = static_cast<const uint32_t *>(temp) + kPvgHeader;
  const dim3 grid((unsigned)cdiv(N, kPvgBlock)), block(kPvgBlock);
  const PvgTime t = pvg_time(cur_time, delta_t, in_smooth, T);
#define BDS_PVG_BWD(MD)                                                                                                                 \
  hipLaunchKernelGGL((pvg_bwd_kernel<MD>), grid, block, 0, as_stream(stream), N, K, t, velocity, taus, betas, logits, log_scales, quats, \
                     cam_pos, filter_mask, table, out_means, out_sh_raw, v_out_means, v_out_opacities, v_out_rgbs, v_out_scales,        \
                     v_out_quats, v_means, v_velocity, v_taus, v_betas, v_logits, v_log_scales, v_quats, v_features_dc, v_features_rest)
  switch (pvg_mode(K, degrees_to_use)) {
    case 0: BDS_PVG_BWD(0); break;
    case 1: BDS_PVG_BWD(1); break;
    case 2: BDS_PVG_BWD(2); break;
    case 3: BDS_PVG_BWD(3); break;
    default: BDS_PVG_BWD(kPvgSigmoid); break;
  }
#undef BDS_PVG_BWD
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
