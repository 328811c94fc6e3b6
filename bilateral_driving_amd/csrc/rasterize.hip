// K7/K8: per-pixel front-to-back alpha compositing, forward and backward.
// rasterize_to_pixels stage of gsplat.rendering.rasterization as called at
// /root/reference/project/models/trainers/base.py:393-408 (render_mode "RGB+ED" -> CH = 4,
// viewer "RGB" -> CH = 3).
//
// Data (gfx950): the compositor reads SPLAT RECORDS -- one 48-byte record per (camera, Gaussian), or per visible
// Gaussian in depth-rank order -- through the per-tile index lists: one record is one or two cache lines instead of
// four gathers from four arrays.  A record is 3 x float4:
//     (mean2d.x, mean2d.y, ea, eb) (ec, opacity, colour0, colour1) (colour2, colour3, -, radius as int bits)
// with the conic pre-scaled into the exponent's base-2 units, (ea, eb, ec) = -log2(e) * (a/2, b, c/2), so that
// alpha = opacity * 2^(ea dx^2 + eb dx dy + ec dy^2): one multiply per (pixel, Gaussian) less than exp(-sigma), in both
// directions, with the forward and the backward taking bit-identical alpha decisions.
// The backward accumulates into GRADIENT RECORDS of 16 floats (64-byte aligned: colour 0-3 | conic a,b,c 4-6 | mean2d 7-8 |
// |mean2d| 9-10 (absgrad) | opacity 11): the 12 lanes that commit a (tile, Gaussian) pair's sums hit ONE 64-byte segment
// (measured on MI355X, scripts/ubench/valu_rate.hip: 4.1x the atomic throughput of five separate arrays).
//
// Mapping: ONE wave64 per 16x16 tile, four pixels per lane (lane l: column l % 16, rows l / 16 + 4q): the tile's
// depth-ordered list is staged through LDS in chunks of 64 (one record per lane, next chunk prefetched into registers),
// then every lane walks the chunk reading LDS at a wave-uniform address (broadcast reads); dx and the x-terms of the
// quadratic form are shared by the lane's four pixels.  Early termination: a pixel stops at T*(1-a) <= 1e-4, the wave
// leaves once all its pixels are done (ballot).  Both kernels are bound by VALU issue (SQ counters: ~100 % VALU busy), so the
// inner loops are written branch-free per pixel: a pixel that does not blend a Gaussian runs the same instructions with
// alpha = 0 (exec-masked branches cost the compiler ~50 register copies per pair for the accumulator phis).
// Workgroup ids are remapped so that each XCD rasterises one contiguous band of the image (its private L2 then serves
// the re-reads of records shared by neighbouring tiles).
#include "bds_common.h"
#include "ed_epilogue.h"
#include "gs_math.h"

namespace bds {

constexpr int kTile = 16;
constexpr int kPackBlock = 256;
constexpr int kGradStride = BDS_GRAD_RECORD_FLOATS;  // 16
constexpr int kUnboundedRadius = 1 << 20;   // record radius slot when the caller has no radii: the bounding square covers any image
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// Work item of a workgroup: the XCD-contiguous position, optionally redirected through a schedule
// (bds_rasterize_bwd_schedule: each XCD's range re-ordered longest tile first, see below).
// Schedule buffer (int32, bds_rasterize_schedule_ints): word 0 tags the form.
//   sorted (tag 1): [1 | order[total] | work[total]] -- bds_rasterize_bwd_schedule(_sort): every XCD's range of tiles ordered by a
//                   counting sort over 1024 linear bins of the tiles' visited lengths;
//   binned (tag 0): [0 | count[8][32] | list[8][32][total / 8 + 1]] -- device-count form: every compositing wave of the FORWARD drops
//                   its tile into the bin of its visited length (32 bins a factor 2^(1/4) apart, longest first) of its XCD's range
//                   with one atomic; the backward's workgroup resolves (range, slot) -> bin by a prefix walk over the 32 counts.  No sort launch
//                   between the passes; the header is cleared by the record pack in front of the forward (bds_splat_pack / bds_splat_pack_sh).
constexpr int kSchedXcd = 8, kSchedLogBins = 32, kSchedHeader = 1 + kSchedXcd * kSchedLogBins;
__host__ __device__ __forceinline__ int sched_stride(int total) { return total / kSchedXcd + 1; }
__device__ __forceinline__ int sched_bin(int w) {   // 0 = longest ... kSchedLogBins - 1 = nothing to do
  if (w <= 0) return kSchedLogBins - 1;
  const int lz = 31 - __clz(w);
  const int h = 4 * lz + (lz >= 2 ? ((w >> (lz - 2)) & 3) : 0);   // floor(4 log2 w) (to the next two mantissa bits)
  return min(max(57 - h, 0), kSchedLogBins - 2);                   // bin 0: >= 20 480 entries; bin 30: < 128
}

// may_be_missing: the SPLIT launch keeps its long tiles out of the bins, so a range has fewer entries than workgroups and a slot without
// an entry means "nothing to do" (-1); everywhere else every tile sits in some bin, and a slot without a valid entry can only mean a
// header nobody cleared / filled: plain order, every tile still processed
__device__ __forceinline__ int pick_item(const int32_t *__restrict__ order, int bid, int total, bool may_be_missing = false) {
  const int p = xcd_contiguous(bid, total);
  if (!order) return p;
  if (order[0] != 0) return order[1 + p];
  // (all counts are read unconditionally -- wave-uniform addresses: a few wide scalar loads and a scalar prefix walk, no vector
  // registers and no chain of dependent loads in front of a kernel that sits on its register budget)
  const int x = bid % kSchedXcd, slot = bid / kSchedXcd;
  const int32_t *__restrict__ cnt = order + 1 + x * kSchedLogBins;
  int acc = 0, sel = -1, before = 0;
#pragma unroll
  for (int b = 0; b < kSchedLogBins; b++) {
    const int c = cnt[b];
    if (sel < 0 && slot < acc + c) { sel = b; before = acc; }
    acc += c;
  }
  if (sel >= 0) {
    const int item = order[kSchedHeader + (x * kSchedLogBins + sel) * sched_stride(total) + (slot - before)];
    if ((unsigned)item < (unsigned)total) return item;   // (anything else: a header the pack did not clear -- plain order)
  }
  return (acc == 0 || !may_be_missing) ? p : -1;
}

// ---- splat records --------------------------------------------------------------------------------------
// rec[r] = record of entry ids[r] (ids == null: r itself) of the per-(camera, Gaussian) arrays
template <int CH>
__global__ __launch_bounds__(kPackBlock) void splat_pack_kernel(int64_t n_cap, const uint64_t *__restrict__ n_dev,
                                                               const int32_t *__restrict__ ids,
                                                               const float *__restrict__ means2d, const float *__restrict__ conics,
                                                               const float *__restrict__ colors, const float *__restrict__ opacities,
                                                               const int32_t *__restrict__ radii, float4 *__restrict__ rec,
                                                               float4 *__restrict__ zero_rec, float4 *__restrict__ zero_tail,
                                                               int zero_tail_f4, int32_t *__restrict__ schedule) {
  // (fused view: the gradient record of every packed row -- what the composite backward accumulates into -- and the camera-pose
  // gradient slots behind them are cleared here instead of by a fill launch of their own; likewise the header of the binned
  // backward schedule the forward compositor is about to fill)
  if (zero_tail && blockIdx.x == 0)
    for (int i = threadIdx.x; i < zero_tail_f4; i += kPackBlock) zero_tail[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (schedule && blockIdx.x == 0)
    for (int i = threadIdx.x; i < kSchedHeader; i += kPackBlock) schedule[i] = 0;
  const int64_t n = list_length(n_cap, n_dev);
  const int64_t r = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
  if (r >= n) return;
  if (zero_rec) {
#pragma unroll
    for (int i = 0; i < kGradStride / 4; i++) zero_rec[r * (kGradStride / 4) + i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t g = ids ? (int64_t)ids[r] : r;
  const float2 xy = *reinterpret_cast<const float2 *>(means2d + g * 2);
  const float *cn = conics + g * 3;
  const float *cl = colors + g * CH;
  rec[r * 3] = make_float4(xy.x, xy.y, (-0.5f * kLog2e) * cn[0], -kLog2e * cn[1]);
  rec[r * 3 + 1] = make_float4((-0.5f * kLog2e) * cn[2], opacities[g], cl[0], CH > 1 ? cl[CH > 1 ? 1 : 0] : 0.f);
  // last slot: the projection's pixel radius (gsplat's bounding square; "unbounded" without radii) -- read by the coarse-list filter
  rec[r * 3 + 2] = make_float4(CH > 2 ? cl[CH > 2 ? 2 : 0] : 0.f, CH > 3 ? cl[CH > 3 ? 3 : 0] : 0.f, 0.f,
                               __int_as_float(radii ? radii[g] : kUnboundedRadius));
}

// The same for the fused view, with the colour evaluated on the way (models/gaussians/vanilla.py:383-389: SH of the normalised view
// direction means - cam_pos, + 0.5, clamp to [0, 1]; channel 3 = depth for the RGB+ED composite): record r is the visible Gaussian
// ids[r].  Evaluating the SH colours HERE, for the visible Gaussians only and in list order, replaces a pass over all N Gaussians
// that wrote two dense per-Gaussian arrays nobody reads for the culled 85 %.  sh_rgb_out [n,3] keeps the un-clamped colour of record
// r: the backward needs to know where the clamp was active.
constexpr int kPackShBlock = 128;   // (x 208 bytes of staged coefficients per thread at degree 3)
template <int DEG>
__global__ __launch_bounds__(kPackShBlock) void splat_pack_sh_kernel(int64_t n_cap, const uint64_t *__restrict__ n_dev,
                                                                  const int32_t *__restrict__ ids, int K,
                                                                  const float *__restrict__ means, const float *__restrict__ cam_pos,
                                                                  const float *__restrict__ coeffs, const float *__restrict__ coeffs_rest,
                                                                  const float *__restrict__ means2d,
                                                                  const float *__restrict__ conics, const float *__restrict__ depths,
                                                                  const float *__restrict__ opacities, const int32_t *__restrict__ radii,
                                                                  float4 *__restrict__ rec, float *__restrict__ sh_rgb_out,
                                                                  float4 *__restrict__ zero_rec, float4 *__restrict__ zero_tail,
                                                                  int zero_tail_f4, int32_t *__restrict__ schedule, const ProjLayout pl) {
  constexpr int nb = (DEG + 1) * (DEG + 1);
  constexpr int n4 = (nb * 3 + 3) / 4;       // 16-byte pieces of a coefficient row the colour needs
  constexpr int ldr = n4 * 4 + 4;            // LDS row stride (floats): 16-byte aligned, an odd number of 16-byte pieces
  // A thread gathering its own 192-byte row piece by piece touches 64 rows per load instruction; instead the workgroup's rows are
  // staged through LDS with n4 consecutive lanes per row (each row's pieces leave memory as whole cache lines), as the list-driven
  // SH backward writes them (csrc/sh.hip).
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int32_t s_g[kPackShBlock];
  if (zero_tail && blockIdx.x == 0)   // (as splat_pack_kernel: the gradient records / pose slots are cleared on the way)
    for (int i = threadIdx.x; i < zero_tail_f4; i += kPackShBlock) zero_tail[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (schedule && blockIdx.x == 0)
    for (int i = threadIdx.x; i < kSchedHeader; i += kPackShBlock) schedule[i] = 0;
  const int64_t n = list_length(n_cap, n_dev);
  const int64_t r0 = (int64_t)blockIdx.x * kPackShBlock;
  if (r0 >= n) return;
  const int cnt = (int)(n - r0 < (int64_t)kPackShBlock ? n - r0 : (int64_t)kPackShBlock);
  const int tid = threadIdx.x;
  const int64_t r = r0 + tid;
  if (tid < cnt) s_g[tid] = ids[r];
  __syncthreads();
  if (coeffs_rest != nullptr) {
    // split storage (the reference's parameters: band 0 [N,3] in `coeffs`, bands 1.. [N,K-1,3] in `coeffs_rest`,
    // models/gaussians/vanilla.py:96-104,382): rows of 4-byte alignment, staged float by float
    // (the first form: float by float, 48 scalar loads per thread at degree 3 -- 70 us for the 310 k visible rows of the headline
    //  view where the one-array form takes 33).  Now n4 lanes per row as below: piece 0 = band 0 + the first float of `coeffs_rest`,
    //  piece c >= 1 = floats 4c-3 .. 4c of the row's `coeffs_rest`, ONE 16-byte load at 4-byte alignment each (gfx950 runs with
    //  unaligned vector access enabled; a piece that would run past the row's end goes float by float -- K = (DEG+1)^2 = 9 only, whose
    //  27 floats are no multiple of 4: at K = 4 and K = 16 the last piece ends on the row's last float)
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    const int64_t row_rest = (int64_t)(K - 1) * 3;
    const int total = cnt * n4;
#pragma unroll 4
    for (int e = tid; e < total; e += kPackShBlock) {
      const int rr = e / n4, c = e - rr * n4;
      const int64_t g = s_g[rr];
      const float *rest = coeffs_rest + g * row_rest;
      float4 v;
      if (c == 0) {
        v = make_float4(coeffs[g * 3], coeffs[g * 3 + 1], coeffs[g * 3 + 2], row_rest > 0 ? rest[0] : 0.f);
      } else if (4 * c + 1 <= row_rest) {
        const f4u u = *reinterpret_cast<const f4u *>(rest + 4 * c - 3);
        v = make_float4(u.x, u.y, u.z, u.w);
      } else {
        const int b = 4 * c - 3;
        v = make_float4(b < row_rest ? rest[b] : 0.f, b + 1 < row_rest ? rest[b + 1] : 0.f, b + 2 < row_rest ? rest[b + 2] : 0.f, 0.f);
      }
      *reinterpret_cast<float4 *>(lds + rr * ldr + c * 4) = v;
    }
  } else {
    const int total = cnt * n4;
    const int64_t row = (int64_t)K * 3;
#pragma unroll 4
    for (int e = tid; e < total; e += kPackShBlock) {
      const int rr = e / n4, c = e - rr * n4;
      const float4 v = reinterpret_cast<const float4 *>(coeffs + (int64_t)s_g[rr] * row)[c];   // 16-byte aligned (checked by the caller)
      *reinterpret_cast<float4 *>(lds + rr * ldr + c * 4) = v;
    }
  }
  __syncthreads();
  if (tid >= cnt) return;
  if (zero_rec) {
#pragma unroll
    for (int i = 0; i < kGradStride / 4; i++) zero_rec[r * (kGradStride / 4) + i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t g = s_g[tid];
  const float x = means[g * 3] - cam_pos[0], y = means[g * 3 + 1] - cam_pos[1], z = means[g * 3 + 2] - cam_pos[2];
  const float inorm = 1.0f / sqrtf(x * x + y * y + z * z);
  float B[16];
  sh_bases(DEG, x * inorm, y * inorm, z * inorm, B);
  float cf[n4 * 4];
#pragma unroll
  for (int i = 0; i < n4; i++) {
    const float4 v = *reinterpret_cast<const float4 *>(lds + tid * ldr + i * 4);
    cf[i * 4] = v.x; cf[i * 4 + 1] = v.y; cf[i * 4 + 2] = v.z; cf[i * 4 + 3] = v.w;
  }
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
  for (int k = 0; k < nb; k++) {
    o0 += B[k] * cf[k * 3];
    o1 += B[k] * cf[k * 3 + 1];
    o2 += B[k] * cf[k * 3 + 2];
  }
  sh_rgb_out[r * 3] = o0; sh_rgb_out[r * 3 + 1] = o1; sh_rgb_out[r * 3 + 2] = o2;
  // (the projection's outputs: five arrays, or the columns of one [N,8] row block -- bds_common.h ProjLayout)
  const float2 xy = *reinterpret_cast<const float2 *>(means2d + g * pl.s2);
  const float *cn = conics + g * pl.sc;
  rec[r * 3] = make_float4(xy.x, xy.y, (-0.5f * kLog2e) * cn[0], -kLog2e * cn[1]);
  rec[r * 3 + 1] = make_float4((-0.5f * kLog2e) * cn[2], opacities[g * pl.so], fminf(fmaxf(o0 + 0.5f, 0.f), 1.f), fminf(fmaxf(o1 + 0.5f, 0.f), 1.f));
  rec[r * 3 + 2] = make_float4(fminf(fmaxf(o2 + 0.5f, 0.f), 1.f), depths[g * pl.sd], 0.f, __int_as_float(proj_radius(pl, means2d, radii, g)));
}

// exponent (base 2) of a Gaussian at a pixel of the lane's column: ea dx^2 + (ec dy + eb dx) dy, <= 0 for a valid conic.
// ONE definition shared by the forward and the backward: their alpha decisions have to agree bit for bit.
__device__ __forceinline__ float splat_exponent(float eadx2, float ebdx, float ec, float dy) {
  return __builtin_fmaf(__builtin_fmaf(ec, dy, ebdx), dy, eadx2);
}

// ---- coarse lists -------------------------------------------------------------------------------------------
// The depth-ordered lists may be built for LIST tiles of list_div x list_div compositing tiles (64 x 64 px for list_div = 4): the
// tile stage then emits and sorts one pair per (list tile, Gaussian) -- a fraction of the (16-px tile, Gaussian) pairs, most of
// which the compositor never reaches because its pixels saturate first -- and every compositing wave filters the chunk of its
// list tile's list it is about to blend: lane l tests candidate l against the wave's own 16 x 16 rectangle of pixel centres
// (the span test of the tile stage, gs_math.h row_tile_span, on the record's base-2 quadratic form) and the survivors
// are compacted into LDS in list order.  The test has the two parts that define a (16-px tile, Gaussian) pair of the fine lists:
// the tile lies in gsplat's bounding square of the Gaussian (tile_rect on the record's radius -- the reference CLIPS a splat there,
// at 3 sigma, even where alpha is still above 1/255), and a pixel centre of the tile reaches alpha >= 1/255 (a candidate that fails
// this part contributes nothing anyway).  With the radii in the records the image, and the gradients, are those of 16-px lists;
// records packed without radii carry an unbounded square, which gives gsplat's own semantics for lists of larger tiles
// (tile_size = 32, 64, ...: clipped at that tile granularity).  Forward and backward share ONE definition of the test.
struct ListGeom {
  int div, w, h;   // compositing tiles per list tile (per axis); list tiles per row / column
  int total;       // C * w * h lists
  int sched;       // forward's tile_work argument: 0 = a work array, 1 = the binned schedule buffer (see pick_item)
};

// (row0, nrows: the band of the tile's pixel rows the caller composites -- the whole tile, or one 16 x 4 strip of a LONG tile: the
//  bounding-square part stays at tile granularity, as gsplat clips, the alpha part is taken over the band)
__device__ __forceinline__ bool tile_candidate_hit(const float4 &A, const float4 &B, const float4 &Cr, int tx, int ty, int tile_w,
                                                   int tile_h, int row0 = 0, int nrows = kTile) {
#pragma clang fp contract(off)
  int x0, y0, x1, y1;
  tile_rect(A.x, A.y, __float_as_int(Cr.w), kTile, tile_w, tile_h, x0, y0, x1, y1);
  if (tx < x0 || tx >= x1 || ty < y0 || ty >= y1) return false;
  // alpha >= 1/255  <=>  q(d) = a dx^2 + 2 b dx dy + c dy^2 <= log2(255 opacity) =: tau in the record's base-2 units.
  // Same construction as gs_math.h row_tile_span (x-extent of the ellipse cut by the tile's band of pixel-centre rows) with
  // hardware rcp / sqrt (1 ulp) and a slack that covers them: conservative -- a spurious survivor only costs its blend.
  const float tau = __builtin_amdgcn_logf(B.y * 255.f) + 1e-3f;
  if (!(tau > 0.f)) return false;
  const float a = -A.z, b = -0.5f * A.w, c = -B.x;
  const float det = a * c - b * b;
  const float ia = __builtin_amdgcn_rcpf(a), tid = tau * __builtin_amdgcn_rcpf(det);
  const float hy = __builtin_amdgcn_sqrtf(a * tid), hx = __builtin_amdgcn_sqrtf(c * tid);
  constexpr float kSlack = 0.03f;
  float e0 = ((float)(ty * kTile + row0) + 0.5f) - A.y, e1 = e0 + (float)(nrows - 1);
  if (e0 > hy + kSlack || e1 < -hy - kSlack) return false;
  e0 = fminf(fmaxf(e0, -hy), hy);
  e1 = fminf(fmaxf(e1, -hy), hy);
  const float aq = a * tau;
  const float r0 = __builtin_amdgcn_sqrtf(fmaxf(aq - det * e0 * e0, 0.f)), r1 = __builtin_amdgcn_sqrtf(fmaxf(aq - det * e1 * e1, 0.f));
  float xr = fmaxf(r0 - b * e0, r1 - b * e1) * ia;
  float xl = fminf(-r0 - b * e0, -r1 - b * e1) * ia;
  const float dyR = -b * hx * __builtin_amdgcn_rcpf(c);   // height of the ellipse's right-most point (left-most: -dyR)
  if (dyR >= e0 && dyR <= e1) xr = hx;
  if (-dyR >= e0 && -dyR <= e1) xl = -hx;
  const float c0 = ((float)(tx * kTile) + 0.5f) - A.x, c1 = c0 + (float)(kTile - 1);   // the tile's pixel-centre columns
  const float slack = kSlack + 4e-6f * (fabsf(xl) + fabsf(xr));
  return !(xr + slack < c0 || xl - slack > c1);   // (NaN from a degenerate conic: keep the candidate)
}

// list range [start, end) of a compositing tile
template <bool kCoarse>
__device__ __forceinline__ void list_range(const int32_t *__restrict__ offsets, int item, int n_items, int cam, int tx, int ty,
                                           const ListGeom &lg, int64_t M, int &start, int &end) {
  const int li = kCoarse ? (cam * lg.h + ty / lg.div) * lg.w + tx / lg.div : item;
  const int total = kCoarse ? lg.total : n_items;
  start = offsets[li];
  end = (li == total - 1) ? (int)M : offsets[li + 1];
}

// min(0.999, ov) for ov >= 0 as ONE v_med3_f32 (fminf costs a canonicalising v_max in front of the v_min)
__device__ __forceinline__ float clamp_alpha(float ov) { return __builtin_amdgcn_fmed3f(ov, kAlphaMax, -1.f); }

// ---- forward ----------------------------------------------------------------------------------------------
// every pixel of a lane finished (T < 0)
template <int NQ>
__device__ __forceinline__ bool lane_done(const float *T) {
  float m = T[0];
#pragma unroll
  for (int q = 1; q < NQ; q++) m = fmaxf(m, T[q]);
  return m < 0.f;
}

// One wave, one tile (NQ = 4: lane l owns column l % 16, rows l / 16 + 4 q) or one 16 x 4 STRIP q0 of a tile (NQ = 1: one pixel per
// lane; bds_rasterize_*_dev(split_len): a tile whose list is that long is composited by four waves).  bid: the workgroup's index in a
// launch of one workgroup per tile.
template <int CH, bool kCoarse, bool kStrip, int NQ>
__device__ __forceinline__ void rasterize_fwd_wave_body(
    int bid, int q0, int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec,
    const float *__restrict__ backgrounds, int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets,
    const int32_t *__restrict__ flatten, float *__restrict__ render, float *__restrict__ alphas, float *__restrict__ t_final, int32_t *__restrict__ last_ids,
    const ListGeom &lg, int32_t *__restrict__ tile_work, float4 *sA, float4 *sB, float4 *sC, int item_in = -1, int ov_start = -1,
    int ov_end = -1) {
  // (ov_start / ov_end: the tile's list is [ov_start, ov_end) of `flatten` instead of its list tile's -- a long tile's REFINED list)
  const int64_t M = M_dev ? (int64_t)*M_dev : M_host;   // (the list length may live on the device: M_dev of bds_rasterize_fwd)
  const int n_tiles = tile_w * tile_h;
  const int item = item_in >= 0 ? item_in : xcd_contiguous(bid, C * n_tiles);
  const int cam = item / n_tiles, tile = item - cam * n_tiles;
  const int ty = tile / tile_w, tx = tile - ty * tile_w;
  const int lane = threadIdx.x;
  const int j = tx * kTile + (lane & 15);
  const int i0 = ty * kTile + (lane >> 4) + 4 * q0;
  const float px = (float)j + 0.5f;
  int start, end;
  list_range<kCoarse>(offsets, item, C * n_tiles, cam, tx, ty, lg, M, start, end);
  if (ov_start >= 0) { start = ov_start; end = ov_end; }
  // T[q] > 0: running transmittance; T[q] < 0: the pixel is finished and |T[q]| is its final transmittance
  // (pixels outside the image start finished).  One register instead of a flag + a value per pixel.
  float T[NQ], pyc[NQ];
  int cur[NQ];
  float out[NQ][4];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    cur[q] = 0;
    T[q] = ((i0 + 4 * q) < H && j < W) ? 1.f : -1.f;
    pyc[q] = (float)(i0 + 4 * q) + 0.5f;
#pragma unroll
    for (int k = 0; k < 4; k++) out[q][k] = 0.f;
  }
  const int nbatch = (end - start + kWave - 1) / kWave;
  // the next chunk's records are fetched into registers while the current chunk is blended, so the
  // two dependent gather latencies (index -> record) are off the critical path of this single-wave workgroup
  float4 pA = make_float4(0.f, 0.f, 0.f, 0.f), pB = pA, pC = pA;
  if (start + lane < end) {
    const int64_t r = flatten[start + lane];
    pA = rec[r * 3]; pB = rec[r * 3 + 1];
    if (CH > 2 || kCoarse) pC = rec[r * 3 + 2];
  }
  for (int b = 0; b < nbatch; b++) {
    if (__all(lane_done<NQ>(T))) break;
    const int bstart = start + b * kWave;
    int bs = min(kWave, end - bstart);
    __syncthreads();
    if (kCoarse) {
      // keep the candidates that reach this tile, in list order; their list position rides in the record's spare slot
      const bool hit = (bstart + lane < end) && tile_candidate_hit(pA, pB, pC, tx, ty, tile_w, tile_h, NQ == 4 ? 0 : 4 * q0, 4 * NQ);
      const uint64_t m = __ballot(hit);
      bs = __popcll(m);
      if (hit) {
        const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        pC.z = __int_as_float(bstart + lane);
        sA[pos] = pA; sB[pos] = pB; sC[pos] = pC;
      }
    } else if (bstart + lane < end) {
      sA[lane] = pA; sB[lane] = pB;
      if (CH > 2) sC[lane] = pC;
    }
    __syncthreads();
    if (bstart + kWave + lane < end) {
      const int64_t r = flatten[bstart + kWave + lane];
      pA = rec[r * 3]; pB = rec[r * 3 + 1];
      if (CH > 2 || kCoarse) pC = rec[r * 3 + 2];
    }
    // one staged entry against the lane's four pixels
    auto blend_entry = [&](int t) {
      const float4 A = sA[t], B = sB[t];
      const float dx = A.x - px;
      const float ebdx = A.w * dx, eadx2 = A.z * dx * dx;
      float4 Cc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (CH > 2 || kCoarse) Cc = sC[t];
      const int pos_t = kCoarse ? __float_as_int(Cc.z) : bstart + t;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        // branch-free per pixel (as the backward): a pixel that does not blend this Gaussian adds vis = 0 and keeps T, cur.
        // (Exec-masked branches cost ~16 scalar instructions per pixel row here: the kernel was issuing 0.7 scalar per vector op.)
        const float e = splat_exponent(eadx2, ebdx, B.x, A.y - pyc[q]);
        const float ov = B.y * __builtin_amdgcn_exp2f(e);
        const float alpha = clamp_alpha(ov);
        const bool valid = !((e > 0.f) | (ov < kAlphaMin));   // (bitwise: no short-circuit exec masking)
        if (kStrip && !__any(valid)) continue;   // no pixel of this 16 x 4 strip reaches the Gaussian
        // No test of T > 0: a finished pixel (T < 0) has nT = T (1 - alpha) < 0 with 1 - alpha >= 0.001, so `live` is false for it
        // and the update below hands it -|T| = T back.  A live pixel that this Gaussian would take below the transmittance floor is
        // finished, not blended: it gets -|T| = -T.
        const float nT = T[q] * (1.f - alpha);
        const bool live = nT > kTStop;
        const bool blend = valid & live;
        const float vis = blend ? alpha * T[q] : 0.f;
        out[q][0] = __builtin_fmaf(B.z, vis, out[q][0]);
        if (CH > 1) out[q][1] = __builtin_fmaf(B.w, vis, out[q][1]);
        if (CH > 2) out[q][2] = __builtin_fmaf(Cc.x, vis, out[q][2]);
        if (CH > 3) out[q][3] = __builtin_fmaf(Cc.y, vis, out[q][3]);
        cur[q] = blend ? pos_t : cur[q];
        T[q] = valid ? (live ? nT : -fabsf(T[q])) : T[q];
      }
    };
    // the all-pixels-finished test runs every second entry: an entry blended against a finished tile changes nothing
    for (int t = 0; t < bs; t += 2) {
      if (__all(lane_done<NQ>(T))) break;
      blend_entry(t);
      if (t + 1 < bs) blend_entry(t + 1);
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int i = i0 + 4 * q;
    if (i < H && j < W) {
      const int64_t pix = ((int64_t)cam * H + i) * W + j;
      const float Tf = fabsf(T[q]);
      alphas[pix] = 1.f - Tf;
      if (t_final) t_final[pix] = Tf;     // (1 - Tf rounds the last bits of a small Tf away: the backward starts from the value itself)
      last_ids[pix] = cur[q];
      float *r = render + pix * CH;
#pragma unroll
      for (int k = 0; k < CH; k++) r[k] = backgrounds ? out[q][k] + Tf * backgrounds[cam * CH + k] : out[q][k];
    }
  }
  if (tile_work && NQ == 4) {   // (the strips of a long tile stay out of the schedule: the backward finds them in the long-tile list)
    // the backward's schedule key: how far into its list this tile blended (what tile_work_kernel re-derives from last_ids; pixels
    // outside the image and pixels that blended nothing hold 0)
    int mc = cur[0];
#pragma unroll
    for (int q = 1; q < NQ; q++) mc = max(mc, cur[q]);
    const int m = wave_max_i32(mc);
    const int w = max(0, m - start + 1);
    if (lane == 0) {
      if (lg.sched) {   // binned: the tile joins its length's bin of this XCD's range (the range xcd_contiguous gave this workgroup)
        const int x = bid % kSchedXcd, slot = x * kSchedLogBins + sched_bin(w), stride = sched_stride(C * n_tiles);
        const int pos = atomicAdd(tile_work + 1 + slot, 1);
        if (pos < stride) tile_work[kSchedHeader + slot * stride + pos] = item;
      } else {
        tile_work[item] = w;
      }
    }
  }
}

template <int CH, bool kCoarse, bool kStrip>
__global__ __launch_bounds__(kWave) void rasterize_fwd_wave_kernel(
    int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, const float *__restrict__ backgrounds,
    int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
    float *__restrict__ render, float *__restrict__ alphas, float *__restrict__ t_final, int32_t *__restrict__ last_ids, ListGeom lg,
    int32_t *__restrict__ tile_work) {
  __shared__ float4 sA[kWave], sB[kWave], sC[kWave];
  rasterize_fwd_wave_body<CH, kCoarse, kStrip, 4>((int)blockIdx.x, 0, C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, flatten,
                                                  render, alphas, t_final, last_ids, lg, tile_work, sA, sB, sC);
}

// ---- long tiles: four waves per tile ---------------------------------------------------------------------------------------------
// One wave per tile runs as long as the tile's list: where thousands of small splats fall into a few tiles (the vanishing point of a
// street seen from a lidar-initialised scene: 8 300 listed / 4 700 blended entries in one tile against 160 on average) the launch waits
// for those waves -- 2.3 ms forward, 3.1 ms backward for a view whose other tiles are done in 0.3 / 0.6.  A tile whose (list-tile)
// list holds >= split_len entries is therefore composited strip by strip, one 16 x 4 strip per wave -- one pixel per lane, the
// candidate filter taken over the strip's rows, so a small splat is blended by the strips it touches only.  Same pixels, same order
// per pixel: the image is bit-identical.  The launch: [4 x cap strip workgroups of the long tiles, FIRST | one workgroup per tile,
// which leaves at once for a long tile]; the long tiles are listed by a one-workgroup kernel in front (an earlier form with four
// workgroups for EVERY tile, three of which left at once, cost 1.3 ms per launch in empty workgroups alone: profiles/NOTES.md).
// Split area behind the schedule words (bds_rasterize_schedule_ints): [count | 7 unused | flag[total] | list[total]].
constexpr int kSplitHead = 8, kLongBlock = 1024;
static int64_t split_area_offset(int64_t total) {
  const int64_t sorted = 1 + 2 * total, binned = kSchedHeader + (int64_t)kSchedXcd * kSchedLogBins * sched_stride((int)total);
  return sorted > binned ? sorted : binned;
}
__global__ __launch_bounds__(kLongBlock) void long_tiles_kernel(const int32_t *__restrict__ offsets, ListGeom lg, int64_t M_host,
                                                                 const uint64_t *__restrict__ M_dev, int tile_w, int tile_h, int split_len,
                                                                 int cap, int32_t *__restrict__ area) {
  __shared__ int wsum[kLongBlock / kWave];
  const int n_tiles = tile_w * tile_h, per = (n_tiles + kLongBlock - 1) / kLongBlock;
  const int64_t M = M_dev ? (int64_t)*M_dev : M_host;
  const int t0 = (int)threadIdx.x * per;
  int n = 0;
  for (int t = t0; t < min(t0 + per, n_tiles); t++) {
    int start, end;
    list_range<true>(offsets, t, n_tiles, 0, t % tile_w, t / tile_w, lg, M, start, end);
    n += (end - start >= split_len) ? 1 : 0;
  }
  // exclusive scan of n over the workgroup (positions in tile order: deterministic)
  int inc = n;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == kWave - 1) wsum[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kLongBlock / kWave; w++) {
    if (w < wv) base += wsum[w];
    tot += wsum[w];
  }
  int pos = base + inc - n;
  for (int t = t0; t < min(t0 + per, n_tiles); t++) {
    int start, end;
    list_range<true>(offsets, t, n_tiles, 0, t % tile_w, t / tile_w, lg, M, start, end);
    int flag = -1;
    if (end - start >= split_len) {
      if (pos < cap) { flag = pos; area[kSplitHead + n_tiles + pos] = t; }   // (beyond the capacity: one wave, as every other tile)
      pos++;
    }
    area[kSplitHead + t] = flag;
  }
  if (threadIdx.x == 0) { area[0] = min(tot, cap); area[1] = 0; area[2] = tot; }   // (area[1]: the refined lists' pool cursor; [2]: all long tiles)
}

// ---- refined lists of the long tiles ----------------------------------------------------------------------------------------------
// A strip wave of a long tile used to walk the whole list of its 64-px list tile chunk by chunk (the front camera of a lidar-
// initialised street: 36 355 entries = 568 dependent gathers per strip, 64 strips per list tile, forward and again backward) to keep the
// ~1 in 4 entries that reach its 16-px tile.  Now, per view: (A) long_tiles_masks_kernel -- the sub-tiles of a long list tile share ITS
// list: each of their workgroups takes one segment of it and leaves, per entry, the bit mask of the list tile's sub-tiles the entry
// reaches (one record gather per entry instead of one per entry AND sub-tile); (B) long_tiles_refine_kernel -- one workgroup per long
// tile reads its bit of those masks (coalesced, no gather), and writes the tile's own candidates -- same order -- into a pool behind
// the long-tile list; the tile's four strips (forward AND backward) walk that.  Area behind the long-tile list:
// [ref_off[cap] | ref_cnt[cap] | pool[pool_cap] | masks: uint16[M capacity]]; ref_cnt = -1: not refined (the pool ran out, the list
// exceeds kRefMaxChunks x 64 entries, more long tiles than the capacity lists, or list tiles of more than 4 x 4 tiles): the strips walk
// the list tile's list as before.  A refined tile's last_ids are positions in the pool -- forward and backward agree on that, nothing
// else reads them.
constexpr int kRefBlock = 1024, kRefMaxChunks = 2048, kMaskBlock = 256;
__global__ __launch_bounds__(kMaskBlock) void long_tiles_masks_kernel(const float4 *__restrict__ rec, const int32_t *__restrict__ offsets,
                                                                      const int32_t *__restrict__ flatten, ListGeom lg, int64_t M_host,
                                                                      const uint64_t *__restrict__ M_dev, int tile_w, int tile_h, int cap,
                                                                      const int32_t *__restrict__ area, uint16_t *__restrict__ masks) {
  const int total = tile_w * tile_h, jl = (int)blockIdx.x;
  if (jl >= area[0] || area[2] > cap) return;       // (a long tile the capacity does not list would leave its segment undone)
  const int64_t M = M_dev ? (int64_t)*M_dev : M_host;
  const int tile = area[kSplitHead + total + jl], ty = tile / tile_w, tx = tile - ty * tile_w;
  int start, end;
  list_range<true>(offsets, tile, total, 0, tx, ty, lg, M, start, end);
  // this workgroup's segment of the list: sub-tile ordinal o of the nsx x nsy sub-tiles of the list tile that exist
  const int lx = tx / lg.div, ly = ty / lg.div, bx = lx * lg.div, by = ly * lg.div;
  const int nsx = min(lg.div, tile_w - bx), nsy = min(lg.div, tile_h - by), nsub = nsx * nsy;
  const int o = (ty - by) * nsx + (tx - bx);
  const int len = end - start, seg = (len + nsub - 1) / nsub;
  const int s0 = start + o * seg, s1 = min(s0 + seg, end);
  for (int i = s0 + (int)threadIdx.x; i < s1; i += kMaskBlock) {
    const int64_t r = flatten[i];
    const float4 A = rec[r * 3], B = rec[r * 3 + 1], Cr = rec[r * 3 + 2];
    uint32_t m = 0;
    for (int dy = 0; dy < nsy; dy++)
      for (int dx = 0; dx < nsx; dx++)
        if (tile_candidate_hit(A, B, Cr, bx + dx, by + dy, tile_w, tile_h)) m |= 1u << (dy * lg.div + dx);
    masks[i] = (uint16_t)m;
  }
}

__global__ __launch_bounds__(kRefBlock) void long_tiles_refine_kernel(const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
                                                                      ListGeom lg, int64_t M_host, const uint64_t *__restrict__ M_dev,
                                                                      int tile_w, int tile_h, int cap, int32_t *__restrict__ area,
                                                                      int pool_cap, const uint16_t *__restrict__ masks) {
  __shared__ uint64_t bm[kRefMaxChunks];
  __shared__ int pre[kRefMaxChunks];
  __shared__ int wsum[kRefBlock / kWave];
  __shared__ int s_base;
  const int total = tile_w * tile_h, jl = (int)blockIdx.x;
  if (jl >= area[0]) return;
  int32_t *ref_off = area + kSplitHead + 2 * total, *ref_cnt = ref_off + cap, *pool = ref_cnt + cap;
  const int64_t M = M_dev ? (int64_t)*M_dev : M_host;
  const int tile = area[kSplitHead + total + jl], ty = tile / tile_w, tx = tile - ty * tile_w;
  int start, end;
  list_range<true>(offsets, tile, total, 0, tx, ty, lg, M, start, end);
  const int nchunks = (end - start + kWave - 1) / kWave;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
  constexpr int kWaves = kRefBlock / kWave;
  if (nchunks > kRefMaxChunks || pool_cap <= 0 || area[2] > cap) {
    if (tid == 0) ref_cnt[jl] = -1;
    return;
  }
  const int bit = (ty % lg.div) * lg.div + (tx % lg.div);
  for (int c = wv; c < nchunks; c += kWaves) {
    const int i = start + c * kWave + lane;
    const bool hit = i < end && ((masks[i] >> bit) & 1u);
    const uint64_t m = __ballot(hit);
    if (lane == 0) bm[c] = m;
  }
  __syncthreads();
  // exclusive scan of the chunks' counts: a thread owns kRefMaxChunks / kRefBlock consecutive chunks
  constexpr int kPer = kRefMaxChunks / kRefBlock;
  int n = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const int c = tid * kPer + k;
    n += c < nchunks ? __popcll(bm[c]) : 0;
  }
  int inc = n;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == kWave - 1) wsum[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kRefBlock / kWave; w++) {
    if (w < wv) base += wsum[w];
    tot += wsum[w];
  }
  int run = base + inc - n;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    const int c = tid * kPer + k;
    if (c < nchunks) { pre[c] = run; run += __popcll(bm[c]); }
  }
  if (tid == 0) {
    const int b = atomicAdd(area + 1, tot);
    s_base = (b + tot <= pool_cap) ? b : -1;
  }
  __syncthreads();
  const int pb = s_base;
  if (pb < 0) {
    if (tid == 0) ref_cnt[jl] = -1;
    return;
  }
  for (int c = wv; c < nchunks; c += kRefBlock / kWave) {
    const uint64_t m = bm[c];
    if ((m >> lane) & 1ull) {
      const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      pool[pb + pre[c] + pos] = flatten[start + c * kWave + lane];
    }
  }
  if (tid == 0) { ref_off[jl] = pb; ref_cnt[jl] = tot; }
}

template <int CH, bool kStrip>
__global__ __launch_bounds__(kWave) void rasterize_fwd_split_kernel(
    int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, const float *__restrict__ backgrounds,
    int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
    float *__restrict__ render, float *__restrict__ alphas, float *__restrict__ t_final, int32_t *__restrict__ last_ids, ListGeom lg,
    int32_t *__restrict__ tile_work, const int32_t *__restrict__ area, int cap, int pool_cap) {
  __shared__ float4 sA[kWave], sB[kWave], sC[kWave];
  const int total = C * tile_w * tile_h, b = (int)blockIdx.x;
  if (b < 4 * cap) {
    const int jl = b >> 2;
    if (jl >= area[0]) return;
    const int32_t *fl = flatten;
    int ovs = -1, ove = -1;
    if (pool_cap > 0) {      // the tile's refined list (long_tiles_refine_kernel)
      const int32_t *ref_off = area + kSplitHead + 2 * total, *ref_cnt = ref_off + cap;
      const int cnt = ref_cnt[jl];
      if (cnt >= 0) { fl = ref_cnt + cap; ovs = ref_off[jl]; ove = ovs + cnt; }
    }
    rasterize_fwd_wave_body<CH, true, kStrip, 1>(0, b & 3, C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, fl, render,
                                                 alphas, t_final, last_ids, lg, tile_work, sA, sB, sC, area[kSplitHead + total + jl], ovs, ove);
  } else {
    const int bid = b - 4 * cap;
    if (area[kSplitHead + xcd_contiguous(bid, total)] >= 0) return;      // a long tile: its strips do it
    rasterize_fwd_wave_body<CH, true, kStrip, 4>(bid, 0, C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, flatten, render,
                                                 alphas, t_final, last_ids, lg, tile_work, sA, sB, sC);
  }
}

// ---- backward -----------------------------------------------------------------------------------------------
// Lane l owns column l % 16 and rows (l / 16) + 4q, q = 0..3.  The four pixels share dx, so the conic / mean gradients
// need only three per-lane moments of d(loss)/d(sigma) (S0 = sum vs, S1 = sum vs dy, S2 = sum vs dy^2) that are expanded
// once per (lane, Gaussian); 12 per-lane sums then go through ONE 12-value transpose-reduce and 12 lanes commit them to the
// Gaussian's gradient record.  The list is replayed back to front from the tile's deepest blended entry.
// kEpi: the image gradient is not read but FORMED per pixel from the colour transform's deferred backward (ed_epilogue.h: direct route +
// guidance route, clamp / sky blend / expected-depth backward; also writes v_sky) -- the lanes wait for their tile's first records
// anyway, and the transform's third pass over the image (45 us, 172 MB at 1080p) goes away with its two image-sized intermediates.
template <int CH, bool ABS, bool kCoarse, bool kStrip, bool kEpi, int NQ = 4>
__device__ __forceinline__ void rasterize_bwd_wave_body(
    int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, const float *__restrict__ backgrounds,
    int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
    const float *__restrict__ alphas, const float *__restrict__ t_final, const int32_t *__restrict__ last_ids, const float *__restrict__ v_render,
    const float *__restrict__ v_alphas, float *__restrict__ v_rec, const int32_t *__restrict__ tile_order, const ListGeom &lg,
    const EdEpilogue &ep, float4 *sA, float4 *sB, float4 *sC, int32_t *sId, int bid, int q0 = 0, int item_in = -1, int ov_start = -1,
    int ov_end = -1) {
  // (NQ = 4: the whole tile, four pixels per lane; NQ = 1: strip q0 of a LONG tile, one pixel per lane -- see rasterize_fwd_split_kernel)
  const int64_t M = M_dev ? (int64_t)*M_dev : M_host;
  const int n_tiles = tile_w * tile_h;
  const int item = item_in >= 0 ? item_in : pick_item(tile_order, bid, C * n_tiles);
  if (item < 0) return;   // (a schedule slot without a tile: the split launch keeps its long tiles out of the bins)
  const int cam = item / n_tiles, tile = item - cam * n_tiles;
  const int ty = tile / tile_w, tx = tile - ty * tile_w;
  const int lane = threadIdx.x;
  int start, end;
  list_range<kCoarse>(offsets, item, C * n_tiles, cam, tx, ty, lg, M, start, end);
  if (ov_start >= 0) { start = ov_start; end = ov_end; }     // (a long tile's refined list: see long_tiles_refine_kernel)
  if (!kEpi && end <= start) return;   // (kEpi: the tile's pixels still owe their sky gradient)
  const int j = tx * kTile + (lane & 15);
  const float px = (float)j + 0.5f;
  const int i0 = ty * kTile + (lane >> 4) + 4 * q0;
  // Bd[q] = sum_k buffer_k * v_render_k - T_final * (v_alpha - bg . v_render): the only combination of the accumulated
  // colour `buffer` that the gradient needs, kept as ONE scalar per pixel
  float T[NQ], Bd[NQ], vr[NQ][4], pyc[NQ];
  int bin_final[NQ];
  int max_bin = -1;
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const int i = i0 + 4 * q;
    const bool inside = i < H && j < W;
    pyc[q] = (float)i + 0.5f;
    const int64_t pix = ((int64_t)cam * H + (inside ? i : 0)) * W + (inside ? j : 0);
    const float T_final = inside ? (t_final ? t_final[pix] : 1.f - alphas[pix]) : 1.f;
    T[q] = T_final;
    bin_final[q] = inside ? last_ids[pix] : -1;   // -1: never valid (pixel outside the image)
    max_bin = max(max_bin, bin_final[q]);
    float vra = 0.f, bgdot = 0.f;
    if (kEpi) {
      vr[q][0] = vr[q][1] = vr[q][2] = vr[q][3] = 0.f;
      if (inside) ed_epilogue_pixel(ep, i, j, (int)pix, 1.f - T_final, vr[q], vra);
      // one pixel's ~14 loaded values at a time: hoisting all four pixels' loads together costs 15 registers and a resident wave
      __builtin_amdgcn_sched_barrier(0);
    } else {
      vra = inside ? v_alphas[pix] : 0.f;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        vr[q][k] = (k < CH && inside) ? v_render[pix * CH + (k < CH ? k : 0)] : 0.f;
        if (backgrounds && k < CH) bgdot += backgrounds[cam * CH + k] * vr[q][k];
      }
    }
    Bd[q] = -T_final * (vra - bgdot);
  }
  const int tile_bin_final = wave_max_i32(max_bin);
  if (tile_bin_final < start || end <= start) return;   // no pixel of this tile blended anything (last_ids stays 0 then)
  // gradient-record slot this lane commits after the transpose-reduce (one committing lane per quad)
  const int slot = butterfly_slot12(lane);
  const bool commit = butterfly_commit12(lane) && (slot < 4 ? slot < CH : (ABS || (slot != 9 && slot != 10)));
  const int nbatch = (end - start + kWave - 1) / kWave;
  const int b0 = (end - 1 - tile_bin_final) / kWave;  // chunks in front of it lie behind every pixel's last Gaussian
  // register prefetch of the next chunk (see the forward kernel)
  int32_t pg = 0;
  float4 pA = make_float4(0.f, 0.f, 0.f, 0.f), pB = pA, pC = pA;
  {
    const int idx = end - 1 - kWave * b0 - lane;
    if (idx >= start) {
      pg = flatten[idx];
      pA = rec[(int64_t)pg * 3]; pB = rec[(int64_t)pg * 3 + 1];
      if (CH > 2 || kCoarse) pC = rec[(int64_t)pg * 3 + 2];
    }
  }
  for (int b = b0; b < nbatch; b++) {
    const int batch_end = end - 1 - kWave * b;
    __syncthreads();
    int bs = min(kWave, batch_end + 1 - start);
    int t0 = max(0, batch_end - tile_bin_final);
    // -1 / opacity of candidate `lane`, once per staged candidate: it rides in the record's radius slot, which only the filter reads
    // (the entry loop below would otherwise take the reciprocal of a wave-uniform value on 64 lanes for every visited pair)
    const float nrop = -__builtin_amdgcn_rcpf(pB.y);
    if (kCoarse) {
      // survivors of this chunk (same test as the forward), compacted in replay order; entries behind the tile's deepest blended
      // one are dropped here instead of being skipped through t0
      const int idx = batch_end - lane;
      const bool hit = idx >= start && idx <= tile_bin_final &&
                       tile_candidate_hit(pA, pB, pC, tx, ty, tile_w, tile_h, NQ == 4 ? 0 : 4 * q0, 4 * NQ);
      const uint64_t m = __ballot(hit);
      bs = __popcll(m);
      t0 = 0;
      if (hit) {
        const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        pC.z = __int_as_float(idx);
        pC.w = nrop;
        sId[pos] = pg; sA[pos] = pA; sB[pos] = pB; sC[pos] = pC;
      }
    } else if (batch_end - lane >= start) {
      sId[lane] = pg; sA[lane] = pA; sB[lane] = pB;
      if (CH > 2) { pC.w = nrop; sC[lane] = pC; }
    }
    __syncthreads();
    {
      const int idx = batch_end - kWave - lane;
      if (idx >= start) {
        pg = flatten[idx];
        pA = rec[(int64_t)pg * 3]; pB = rec[(int64_t)pg * 3 + 1];
        if (CH > 2 || kCoarse) pC = rec[(int64_t)pg * 3 + 2];
      }
    }
    for (int t = t0; t < bs; t++) {
      float4 Cc = make_float4(0.f, 0.f, 0.f, 0.f);
      if (CH > 2 || kCoarse) Cc = sC[t];
      const int gidx = kCoarse ? __float_as_int(Cc.z) : batch_end - t;   // position of this entry in the list
      const float4 A = sA[t], B = sB[t];
      const float dx = A.x - px;
      const float opac = B.y, ec = B.x;
      const float eadx = A.z * dx, ebdx = A.w * dx;
      const float eadx2 = eadx * dx;
      float e[NQ], ov[NQ], dyq[NQ];
      bool valid[NQ];
      bool any = false;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        dyq[q] = A.y - pyc[q];
        e[q] = splat_exponent(eadx2, ebdx, ec, dyq[q]);
        ov[q] = opac * __builtin_amdgcn_exp2f(e[q]);
        valid[q] = (gidx <= bin_final[q]) & !((e[q] > 0.f) | (ov[q] < kAlphaMin));
        any |= valid[q];
      }
      if (!__any(any)) continue;
      float col[4] = {B.z, B.w, 0.f, 0.f};
      if (CH > 2) { col[2] = Cc.x; col[3] = Cc.y; }
      const float two_eadx = eadx + eadx, two_ec = ec + ec;
      // per-lane sums over the four pixels (branch-free: a pixel that did not blend this Gaussian contributes alpha = 0)
      float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, S0 = 0.f, S1 = 0.f, S2 = 0.f, ax = 0.f, ay = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; q++) {
        // q = one 16 x 4 strip of the tile: a strip none of whose pixels blends this Gaussian adds exact zeros (and T *= 1)
        if (kStrip && !__any(valid[q])) continue;
        const float dy = dyq[q];
        const float am = valid[q] ? clamp_alpha(ov[q]) : 0.f;
        const float ovm = (valid[q] & (ov[q] <= kAlphaMax)) ? ov[q] : 0.f;   // opacity x falloff; the 0.999 clamp passes no gradient
        const float ra = __builtin_amdgcn_rcpf(1.f - am);                   // exactly 1 for am = 0
        T[q] *= ra;
        const float fac = am * T[q];
        float cdot = col[0] * vr[q][0];   // colour . v_render
        g0 = __builtin_fmaf(fac, vr[q][0], g0);
        if (CH > 1) { cdot = __builtin_fmaf(col[1], vr[q][1], cdot); g1 = __builtin_fmaf(fac, vr[q][1], g1); }
        if (CH > 2) { cdot = __builtin_fmaf(col[2], vr[q][2], cdot); g2 = __builtin_fmaf(fac, vr[q][2], g2); }
        if (CH > 3) { cdot = __builtin_fmaf(col[3], vr[q][3], cdot); g3 = __builtin_fmaf(fac, vr[q][3], g3); }
        const float v_alpha = __builtin_fmaf(-ra, Bd[q], T[q] * cdot);
        Bd[q] = __builtin_fmaf(fac, cdot, Bd[q]);
        const float vs = -ovm * v_alpha;   // d(loss)/d(sigma), sigma = -ln2 * e
        S0 += vs;
        S1 = __builtin_fmaf(vs, dy, S1);
        S2 = __builtin_fmaf(vs * dy, dy, S2);
        if (ABS) {
          ax = __builtin_fmaf(fabsf(vs), fabsf(__builtin_fmaf(A.w, dy, two_eadx)), ax);
          ay = __builtin_fmaf(fabsf(vs), fabsf(__builtin_fmaf(two_ec, dy, ebdx)), ay);
        }
      }
      // d(loss)/d(opacity) = sum vm v_alpha = -S0 / opacity (vs = -(opacity vm) v_alpha term by term): no accumulator of its own
      // (-1 / opacity was taken at staging where the entry's third record word is staged: S0 * (-r) and -S0 * r are the same float.
      //  The 1- and 2-channel kernels over 16-px lists stage no third word and keep the reciprocal here.)
      const float go = (CH > 2 || kCoarse) ? S0 * Cc.w : -S0 * __builtin_amdgcn_rcpf(opac);
      // expand the moments: d sigma / d (a, b, c) = (dx^2 / 2, dx dy, dy^2 / 2); d sigma / d mean = -ln2 * d e / d (dx, dy)
      float acc[12];
      acc[0] = g0; acc[1] = g1; acc[2] = g2; acc[3] = g3;
      const float dxS0 = dx * S0;
      acc[4] = 0.5f * dx * dxS0;
      acc[5] = dx * S1;
      acc[6] = 0.5f * S2;
      acc[7] = -kLn2 * __builtin_fmaf(two_eadx, S0, A.w * S1);
      acc[8] = -kLn2 * __builtin_fmaf(A.w, dxS0, two_ec * S1);
      acc[9] = kLn2 * ax; acc[10] = kLn2 * ay;
      acc[11] = go;
      const float tot = butterfly_sum12(acc, lane);
      // the Gaussian's id is wave-uniform: its record's address is formed in scalar registers, the lane adds its constant slot
      float *const grec = v_rec + (int64_t)__builtin_amdgcn_readfirstlane(sId[t]) * kGradStride;
      if (commit) atomicAdd(grec + slot, tot);
    }
  }
}

template <int CH, bool ABS, bool kCoarse, bool kStrip>
__global__ __launch_bounds__(kWave) void rasterize_bwd_wave_kernel(
    int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, const float *__restrict__ backgrounds,
    int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
    const float *__restrict__ alphas, const float *__restrict__ t_final, const int32_t *__restrict__ last_ids, const float *__restrict__ v_render,
    const float *__restrict__ v_alphas, float *__restrict__ v_rec, const int32_t *__restrict__ tile_order, ListGeom lg) {
  __shared__ float4 sA[kWave], sB[kWave], sC[kWave];
  __shared__ int32_t sId[kWave];
  const EdEpilogue none{};
  rasterize_bwd_wave_body<CH, ABS, kCoarse, kStrip, false>(C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, flatten, alphas, t_final,
                                                           last_ids, v_render, v_alphas, v_rec, tile_order, lg, none, sA, sB, sC, sId,
                                                           (int)blockIdx.x);
}
// the split launch's backward: [strip workgroups of the listed long tiles | one workgroup per schedule slot] (rasterize_fwd_split_kernel)
template <int CH, bool ABS>
__global__ __launch_bounds__(kWave) void rasterize_bwd_split_kernel(
    int C, int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, const float *__restrict__ backgrounds,
    int W, int H, int tile_w, int tile_h, const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten,
    const float *__restrict__ alphas, const float *__restrict__ t_final, const int32_t *__restrict__ last_ids, const float *__restrict__ v_render,
    const float *__restrict__ v_alphas, float *__restrict__ v_rec, const int32_t *__restrict__ tile_order, ListGeom lg,
    const int32_t *__restrict__ area, int cap, int pool_cap) {
  __shared__ float4 sA[kWave], sB[kWave], sC[kWave];
  __shared__ int32_t sId[kWave];
  const EdEpilogue none{};
  const int total = C * tile_w * tile_h, b = (int)blockIdx.x;
  if (b < 4 * cap) {
    const int jl = b >> 2;
    if (jl >= area[0]) return;
    const int32_t *fl = flatten;
    int ovs = -1, ove = -1;
    if (pool_cap > 0) {      // the forward refined this tile's list: its last_ids are positions in the pool
      const int32_t *ref_off = area + kSplitHead + 2 * total, *ref_cnt = ref_off + cap;
      const int cnt = ref_cnt[jl];
      if (cnt >= 0) { fl = ref_cnt + cap; ovs = ref_off[jl]; ove = ovs + cnt; }
    }
    rasterize_bwd_wave_body<CH, ABS, true, false, false, 1>(C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, fl, alphas, t_final,
                                                            last_ids, v_render, v_alphas, v_rec, tile_order, lg, none, sA, sB, sC, sId, 0, b & 3,
                                                            area[kSplitHead + total + jl], ovs, ove);
  } else {
    const int bid = b - 4 * cap;
    const int item = pick_item(tile_order, bid, total, true);
    if (item < 0 || area[kSplitHead + item] >= 0) return;
    rasterize_bwd_wave_body<CH, ABS, true, false, false, 4>(C, M_host, M_dev, rec, backgrounds, W, H, tile_w, tile_h, offsets, flatten, alphas, t_final,
                                                            last_ids, v_render, v_alphas, v_rec, tile_order, lg, none, sA, sB, sC, sId, bid, 0, item);
  }
}
// the same with the colour transform's deferred epilogue in the prologue (RGB+ED, one camera).  108 VGPRs (four waves per SIMD
// against the plain kernel's five): held to five with __launch_bounds__(64, 5) it spills 32-76 bytes per lane and runs 8 % slower
template <bool ABS, bool kCoarse>
__global__ __launch_bounds__(kWave) void rasterize_bwd_epi_kernel(
    int64_t M_host, const uint64_t *__restrict__ M_dev, const float4 *__restrict__ rec, int W, int H, int tile_w, int tile_h,
    const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten, const float *__restrict__ alphas, const float *__restrict__ t_final,
    const int32_t *__restrict__ last_ids, float *__restrict__ v_rec, const int32_t *__restrict__ tile_order, ListGeom lg, EdEpilogue ep) {
  __shared__ float4 sA[kWave], sB[kWave], sC[kWave];
  __shared__ int32_t sId[kWave];
  rasterize_bwd_wave_body<4, ABS, kCoarse, false, true>(1, M_host, M_dev, rec, nullptr, W, H, tile_w, tile_h, offsets, flatten, alphas, t_final, last_ids,
                                                        nullptr, nullptr, v_rec, tile_order, lg, ep, sA, sB, sC, sId, (int)blockIdx.x);
}
// ---- backward schedule: longest tile first inside each XCD's range ------------------------------------
// One wave per tile finishes when its LAST pixel does, and the chip holds only ~2 rounds of tiles
// (8160 tiles at 1080p over 1024 SIMDs x 4 resident waves), so tiles dispatched late that happen to be long
// leave most SIMDs idle at the end of the launch.  The visited length of every tile is known exactly after the
// forward pass (max last_id - list start); dispatching each XCD's contiguous range longest-first (LPT rule)
// removes that tail while keeping the range -> XCD assignment (L2 locality) unchanged.
constexpr int kWorkBlock = 256;
__global__ __launch_bounds__(kWorkBlock) void tile_work_kernel(int C, int W, int H, int tile_w, int tile_h,
                                                               const int32_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ last_ids,
                                                               int32_t *__restrict__ work, ListGeom lg) {
  const int n_tiles = tile_w * tile_h, total = C * n_tiles;
  const int item = blockIdx.x * (kWorkBlock / kWave) + (threadIdx.x >> 6);
  if (item >= total) return;
  const int lane = threadIdx.x & 63;
  const int cam = item / n_tiles, tile = item - cam * n_tiles;
  const int ty = tile / tile_w, tx = tile - ty * tile_w;
  const int j = tx * kTile + (lane & 15);
  int m = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = ty * kTile + (lane >> 4) + 4 * q;
    if (i < H && j < W) m = max(m, last_ids[((int64_t)cam * H + i) * W + j]);
  }
  m = wave_max_i32(m);
  // (an empty list leaves last_ids at 0: the estimate is then 0, or 1 for the very first tile)
  // (coarse lists: the length of the candidate range -- proportional to the blended length within a neighbourhood)
  const int li = lg.div > 1 ? (cam * lg.h + ty / lg.div) * lg.w + tx / lg.div : item;
  if (lane == 0) work[item] = max(0, m - offsets[li] + 1);
}

constexpr int kSchedThreads = 1024, kSchedBins = 1024;
__global__ __launch_bounds__(kSchedThreads) void tile_order_kernel(int total, const int32_t *__restrict__ work,
                                                                   int32_t *__restrict__ order, int32_t *__restrict__ tag) {
  __shared__ int hist[kSchedBins];
  __shared__ int s_max;
  constexpr int kXcd = 8;
  const int per = total / kXcd, rem = total % kXcd, x = blockIdx.x;
  const int cnt = per + (x < rem ? 1 : 0), first = x * per + (x < rem ? x : rem);
  const int tid = threadIdx.x;
  if (tid == 0) s_max = 0;
  if (tid == 0 && x == 0) *tag = 1;   // (the sorted form of the schedule buffer: pick_item)
  for (int b = tid; b < kSchedBins; b += kSchedThreads) hist[b] = 0;
  __syncthreads();
  int lmax = 0;
  for (int i = tid; i < cnt; i += kSchedThreads) lmax = max(lmax, work[first + i]);
  lmax = wave_max_i32(lmax);
  if ((tid & 63) == 0) atomicMax(&s_max, lmax);
  __syncthreads();
  int shift = 0;
  while ((s_max >> shift) >= kSchedBins) shift++;
  // bin 0 = longest
  for (int i = tid; i < cnt; i += kSchedThreads) atomicAdd(&hist[kSchedBins - 1 - (work[first + i] >> shift)], 1);
  __syncthreads();
  // exclusive scan of the 1024 bins (one bin per thread, Hillis-Steele in LDS)
  const int mine = hist[tid];
  int incl = mine;
  for (int o = 1; o < kSchedBins; o <<= 1) {
    __syncthreads();
    hist[tid] = incl;
    __syncthreads();
    if (tid >= o) incl += hist[tid - o];
  }
  __syncthreads();
  hist[tid] = incl - mine;   // becomes the bin's running cursor
  __syncthreads();
  for (int i = tid; i < cnt; i += kSchedThreads) {
    const int pos = atomicAdd(&hist[kSchedBins - 1 - (work[first + i] >> shift)], 1);
    order[first + pos] = first + i;
  }
}

}  // namespace bds

using namespace bds;

extern "C" int bds_splat_pack(int64_t n, const uint64_t *n_dev, int CH, const int32_t *ids, const float *means2d, const float *conics,
                              const float *colors, const float *opacities, const int32_t *radii, float *records, float *zero_records,
                              float *zero_tail, int64_t zero_tail_floats, int32_t *schedule, bds_stream_t stream) {
  BDS_REQUIRE(n >= 0 && (CH == 1 || CH == 3 || CH == 4));
  BDS_REQUIRE(zero_tail_floats >= 0 && zero_tail_floats % 4 == 0 && zero_tail_floats < ((int64_t)1 << 24));
  BDS_REQUIRE(!zero_records || aligned16(zero_records));
  BDS_REQUIRE(!zero_tail || aligned16(zero_tail));
  if (n == 0) {
    if (zero_tail && zero_tail_floats &&
        hipMemsetAsync(zero_tail, 0, sizeof(float) * zero_tail_floats, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    if (schedule && hipMemsetAsync(schedule, 0, sizeof(int32_t) * kSchedHeader, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    return BDS_OK;
  }
  BDS_REQUIRE(means2d && conics && colors && opacities && records && aligned16(records));
  BDS_REQUIRE((reinterpret_cast<uintptr_t>(means2d) & 7u) == 0);
  const dim3 grid((unsigned)cdiv(n, kPackBlock)), block(kPackBlock);
  float4 *rec = reinterpret_cast<float4 *>(records);
  float4 *zr = reinterpret_cast<float4 *>(zero_records), *zt = reinterpret_cast<float4 *>(zero_tail);
  const int zt4 = (int)(zero_tail_floats / 4);
  hipStream_t st = as_stream(stream);
#define BDS_PACK(ch) \
  hipLaunchKernelGGL((splat_pack_kernel<ch>), grid, block, 0, st, n, n_dev, ids, means2d, conics, colors, opacities, radii, rec, zr, zt, zt4, schedule)
  if (CH == 1) BDS_PACK(1);
  else if (CH == 3) BDS_PACK(3);
  else BDS_PACK(4);
#undef BDS_PACK
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

// ---- glue of the gsplat-shaped operator's one-view node (rendering._RasterizeView) ---------------------------------------------------
namespace bds {
// records of the visible entries from post-activation colours [N,3] + depths [N] (RGB+ED / RGB: channel 3 = depth), without a
// dense [N,4] concatenation in front
__global__ __launch_bounds__(kPackBlock) void splat_pack_rgbd_kernel(int64_t n, const int32_t *__restrict__ ids, const float *__restrict__ means2d,
                                                                    const float *__restrict__ conics, const float *__restrict__ colors3,
                                                                    const float *__restrict__ depths, const float *__restrict__ opacities,
                                                                    const int32_t *__restrict__ radii, float4 *__restrict__ rec) {
  const int64_t r = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
  if (r >= n) return;
  const int64_t g = ids ? (int64_t)ids[r] : r;
  const float2 xy = *reinterpret_cast<const float2 *>(means2d + g * 2);
  const float *cn = conics + g * 3, *cl = colors3 + g * 3;
  rec[r * 3] = make_float4(xy.x, xy.y, (-0.5f * kLog2e) * cn[0], -kLog2e * cn[1]);
  rec[r * 3 + 1] = make_float4((-0.5f * kLog2e) * cn[2], opacities[g], cl[0], cl[1]);
  rec[r * 3 + 2] = make_float4(cl[2], depths[g], 0.f, __int_as_float(radii ? radii[g] : kUnboundedRadius));
}
// expected depth of gsplat's "ED" modes (bilagrid_math.h expected_depth; ed = 0: the composited depth as it is) as one image
// out [P,4] = (r, g, b, depth), or, kSplit, as TWO arrays out [P,3] and depth [P,1] -- what the reference's trainer splits the render
// into right away (models/trainers/base.py:409-419 torch.split(renders, [3, 1])): as node outputs of their own they need no slice backward
template <bool kSplit>
__global__ __launch_bounds__(256) void ed_fwd_kernel(int64_t P, int ed, const float4 *__restrict__ render, const float *__restrict__ alphas,
                                                     float *__restrict__ out, float *__restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float4 v = render[i];
  if (ed) v.w = expected_depth(v.w, alphas[i]);
  if (kSplit) {
    out[i * 3] = v.x; out[i * 3 + 1] = v.y; out[i * 3 + 2] = v.z;
    depth[i] = v.w;
  } else {
    reinterpret_cast<float4 *>(out)[i] = v;
  }
}
// its backward, and the widening of a 3-channel ("RGB") image gradient to the compositor's 4 channels: v_render = (v_out.rgb,
// v_out.d / max(alpha, 1e-10) | 0), v_alphas = v_alphas_in - [alpha >= 1e-10] D v_out.d / max(alpha, 1e-10)^2.  The image gradient is
// v_rgb [P,ch] with the depth's in channel 3 where ch == 4, or, kSplit, v_rgb [P,3] and v_depth [P]
template <bool kSplit>
__global__ __launch_bounds__(256) void ed_bwd_kernel(int64_t P, int ch, int ed, const float4 *__restrict__ render, const float *__restrict__ alphas,
                                                     const float *__restrict__ v_rgb, const float *__restrict__ v_depth,
                                                     const float *__restrict__ v_alphas_in, float4 *__restrict__ v_render,
                                                     float *__restrict__ v_alphas) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float va = v_alphas_in ? v_alphas_in[i] : 0.f;
  if (v_rgb) {
    v.x = v_rgb[i * ch]; v.y = v_rgb[i * ch + 1]; v.z = v_rgb[i * ch + 2];
    if (!kSplit && ch == 4) v.w = v_rgb[i * 4 + 3];
  }
  if (kSplit && v_depth) v.w = v_depth[i];
  if (ed) {
    const EdGrad g = expected_depth_backward(render[i].w, alphas[i], v.w);
    v.w = g.v_D;
    va -= g.alpha_sub;
  }
  v_render[i] = v;
  v_alphas[i] = va;
}
}  // namespace bds

extern "C" int bds_splat_pack_rgbd(int64_t n, const int32_t *ids, const float *means2d, const float *conics, const float *colors3,
                                   const float *depths, const float *opacities, const int32_t *radii, float *records,
                                   bds_stream_t stream) {
  BDS_REQUIRE(n >= 0);
  if (n == 0) return BDS_OK;
  BDS_REQUIRE(means2d && conics && colors3 && depths && opacities && records && aligned16(records));
  hipLaunchKernelGGL(splat_pack_rgbd_kernel, dim3((unsigned)cdiv(n, kPackBlock)), dim3(kPackBlock), 0, as_stream(stream), n, ids, means2d, conics,
                     colors3, depths, opacities, radii, reinterpret_cast<float4 *>(records));
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
extern "C" int bds_expected_depth_fwd(int64_t P, const float *render4, const float *alphas, float *out4, bds_stream_t stream) {
  BDS_REQUIRE(P >= 0);
  if (P == 0) return BDS_OK;
  BDS_REQUIRE(render4 && alphas && out4 && aligned16(render4) && aligned16(out4));
  hipLaunchKernelGGL(ed_fwd_kernel<false>, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, as_stream(stream), P, 1,
                     reinterpret_cast<const float4 *>(render4), alphas, out4, static_cast<float *>(nullptr));
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
extern "C" int bds_expected_depth_bwd(int64_t P, int channels, int expected_depth, const float *render4, const float *alphas,
                                      const float *v_out, const float *v_alphas_in, float *v_render4, float *v_alphas,
                                      bds_stream_t stream) {
  BDS_REQUIRE(P >= 0 && (channels == 3 || channels == 4) && !(expected_depth && channels != 4));
  if (P == 0) return BDS_OK;
  BDS_REQUIRE(render4 && alphas && v_render4 && v_alphas && aligned16(render4) && aligned16(v_render4));
  hipLaunchKernelGGL(ed_bwd_kernel<false>, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, as_stream(stream), P, channels, expected_depth,
                     reinterpret_cast<const float4 *>(render4), alphas, v_out, static_cast<const float *>(nullptr), v_alphas_in,
                     reinterpret_cast<float4 *>(v_render4), v_alphas);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_expected_depth_split_fwd(int64_t P, int expected_depth, const float *render4, const float *alphas, float *rgb3,
                                           float *depth1, bds_stream_t stream) {
  BDS_REQUIRE(P >= 0);
  if (P == 0) return BDS_OK;
  BDS_REQUIRE(render4 && alphas && rgb3 && depth1 && aligned16(render4));
  hipLaunchKernelGGL(ed_fwd_kernel<true>, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, as_stream(stream), P, expected_depth,
                     reinterpret_cast<const float4 *>(render4), alphas, rgb3, depth1);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}
extern "C" int bds_expected_depth_split_bwd(int64_t P, int expected_depth, const float *render4, const float *alphas, const float *v_rgb3,
                                           const float *v_depth1, const float *v_alphas_in, float *v_render4, float *v_alphas,
                                           bds_stream_t stream) {
  BDS_REQUIRE(P >= 0);
  if (P == 0) return BDS_OK;
  BDS_REQUIRE(render4 && alphas && v_render4 && v_alphas && aligned16(render4) && aligned16(v_render4));
  hipLaunchKernelGGL(ed_bwd_kernel<true>, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, as_stream(stream), P, 3, expected_depth,
                     reinterpret_cast<const float4 *>(render4), alphas, v_rgb3, v_depth1, v_alphas_in, reinterpret_cast<float4 *>(v_render4),
                     v_alphas);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

// coeffs_rest != NULL: the split storage (coeffs = band 0 [N,3], coeffs_rest = bands 1.. [N,K-1,3])
extern "C" int bds_splat_pack_sh(int64_t n, const uint64_t *n_dev, const int32_t *ids, int K, int deg, const float *means,
                                 const float *cam_pos, const float *coeffs, const float *coeffs_rest, const float *means2d,
                                 const float *conics, const float *depths, const float *opacities, const int32_t *radii, float *records,
                                 float *sh_rgb, float *zero_records, float *zero_tail, int64_t zero_tail_floats, int32_t *schedule,
                                 bds_stream_t stream) {
  BDS_REQUIRE(n >= 0 && deg >= 0 && deg <= 3 && K >= (deg + 1) * (deg + 1) && K <= 16);
  BDS_REQUIRE(zero_tail_floats >= 0 && zero_tail_floats % 4 == 0 && zero_tail_floats < ((int64_t)1 << 24));
  BDS_REQUIRE((!zero_records || aligned16(zero_records)) && (!zero_tail || aligned16(zero_tail)));
  if (n == 0) {
    if (zero_tail && zero_tail_floats &&
        hipMemsetAsync(zero_tail, 0, sizeof(float) * zero_tail_floats, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    if (schedule && hipMemsetAsync(schedule, 0, sizeof(int32_t) * kSchedHeader, as_stream(stream)) != hipSuccess) return BDS_ELAUNCH;
    return BDS_OK;
  }
  BDS_REQUIRE(ids && means && cam_pos && coeffs && means2d && conics && depths && opacities && radii && records && sh_rgb);
  BDS_REQUIRE(aligned16(records) && (reinterpret_cast<uintptr_t>(means2d) & 7u) == 0);
  BDS_REQUIRE(coeffs_rest ? K >= 2 : (aligned16(coeffs) && (K * 3) % 4 == 0));
  const dim3 grid((unsigned)cdiv(n, kPackShBlock)), block(kPackShBlock);
  float4 *rec = reinterpret_cast<float4 *>(records);
  float4 *zr = reinterpret_cast<float4 *>(zero_records), *zt = reinterpret_cast<float4 *>(zero_tail);
  const int zt4 = (int)(zero_tail_floats / 4);
  hipStream_t st = as_stream(stream);
  const ProjLayout pl = proj_layout(means2d, depths, conics, opacities);
#define BDS_PACK_SH(d)                                                                                                                 \
  hipLaunchKernelGGL((splat_pack_sh_kernel<d>), grid, block, sizeof(float) * kPackShBlock * ((((d + 1) * (d + 1) * 3 + 3) / 4) * 4 + 4), st, \
                     n, n_dev, ids, K, means, cam_pos, coeffs, coeffs_rest, means2d, conics, depths, \
                     opacities, radii, rec, sh_rgb, zr, zt, zt4, schedule, pl)
  switch (deg) {
    case 0: BDS_PACK_SH(0); break;
    case 1: BDS_PACK_SH(1); break;
    case 2: BDS_PACK_SH(2); break;
    default: BDS_PACK_SH(3); break;
  }
#undef BDS_PACK_SH
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

// list geometry of a launch: list tiles of list_tile_size px (a multiple of the 16-px compositing tile)
static bool list_geom(int C, int W, int H, int list_tile_size, ListGeom &lg) {
  if (list_tile_size < kTile || list_tile_size % kTile) return false;
  lg.div = list_tile_size / kTile;
  lg.w = (W + list_tile_size - 1) / list_tile_size;
  lg.h = (H + list_tile_size - 1) / list_tile_size;
  lg.total = C * lg.w * lg.h;
  lg.sched = 0;
  return true;
}

extern "C" int bds_rasterize_fwd(int C, int64_t n_records, int64_t M, const uint64_t *M_dev, int CH, const float *records,
                                 const float *backgrounds, int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h,
                                 const int32_t *isect_offsets, const int32_t *flatten, float *render, float *alphas, float *t_final,
                                 int32_t *last_ids, int32_t *tile_order, int split_len, int split_cap, int64_t split_pool,
                                 bds_stream_t stream) {
  // (the host-count form never writes a schedule: the lists it serves are scheduled by bds_rasterize_bwd_schedule)
  BDS_REQUIRE(M_dev ? (M > 0 && split_len >= 0 && split_cap >= 0 && split_pool >= 0) : (!tile_order && split_len == 0));
  // tile_order (optional, bds_rasterize_schedule_ints words): the compositing waves leave the backward's schedule themselves --
  // binned form (option 8, default; header cleared by the record pack in front), or their tiles' keys for bds_rasterize_bwd_schedule_sort
  const bool binned = M_dev && option_get(kOptSchedBins) != 0;
  int32_t *tile_work = !tile_order ? nullptr : (binned ? tile_order : tile_order + 1 + (int64_t)C * tile_w * tile_h);
  BDS_REQUIRE(C >= 1 && n_records >= 0 && M >= 0 && W > 0 && H > 0);
  BDS_REQUIRE(tile_size == kTile);
  ListGeom lg;
  BDS_REQUIRE(list_geom(C, W, H, list_tile_size, lg));
  lg.sched = binned ? 1 : 0;
  BDS_REQUIRE(tile_w == (W + kTile - 1) / kTile && tile_h == (H + kTile - 1) / kTile);
  BDS_REQUIRE(CH == 1 || CH == 3 || CH == 4);
  BDS_REQUIRE(isect_offsets && render && alphas && last_ids);
  BDS_REQUIRE(M == 0 || (records && flatten && aligned16(records)));
  const dim3 grid((unsigned)(C * tile_w * tile_h));
  hipStream_t st = as_stream(stream);
  const float4 *rec = reinterpret_cast<const float4 *>(records);
#define BDS_FWD(ch, co)                                                                                                              \
  hipLaunchKernelGGL((rasterize_fwd_wave_kernel<ch, co, true>), grid, dim3(kWave), 0, st, C, M, M_dev, rec, backgrounds, W, H, tile_w, \
                     tile_h, isect_offsets, flatten, render, alphas, t_final, last_ids, lg, tile_work)
  if (lg.div > 1) {
    if (CH == 1) BDS_FWD(1, true);
    else if (CH == 3) BDS_FWD(3, true);
    else if (split_len > 0) {   // long tiles strip by strip (the fused view's shape: one camera, 4 channels, coarse lists, binned schedule)
      BDS_REQUIRE(C == 1 && tile_work && binned && split_cap > 0);
      const int total = tile_w * tile_h, cap = split_cap < total ? split_cap : total;
      int32_t *area = tile_work + split_area_offset(total);
      BDS_REQUIRE(split_pool >= 0 && split_pool < ((int64_t)1 << 31));
      hipLaunchKernelGGL(long_tiles_kernel, dim3(1), dim3(kLongBlock), 0, st, isect_offsets, lg, M, M_dev, tile_w, tile_h, split_len, cap, area);
      if (split_pool > 0 && lg.div > 4) split_pool = 0;     // (16-bit sub-tile masks: list tiles of at most 4 x 4 tiles are refined)
      if (split_pool > 0) {
        uint16_t *masks = reinterpret_cast<uint16_t *>(area + kSplitHead + 2 * total + 2 * cap + split_pool);
        hipLaunchKernelGGL(long_tiles_masks_kernel, dim3((unsigned)cap), dim3(kMaskBlock), 0, st, rec, isect_offsets, flatten, lg, M, M_dev, tile_w,
                           tile_h, cap, area, masks);
        hipLaunchKernelGGL(long_tiles_refine_kernel, dim3((unsigned)cap), dim3(kRefBlock), 0, st, isect_offsets, flatten, lg, M, M_dev, tile_w,
                           tile_h, cap, area, (int)split_pool, masks);
      }
      hipLaunchKernelGGL((rasterize_fwd_split_kernel<4, true>), dim3((unsigned)(4 * cap + total)), dim3(kWave), 0, st, C, M, M_dev, rec,
                         backgrounds, W, H, tile_w, tile_h, isect_offsets, flatten, render, alphas, t_final, last_ids, lg, tile_work, area, cap,
                         (int)split_pool);
    } else BDS_FWD(4, true);
  } else {
    if (CH == 1) BDS_FWD(1, false);
    else if (CH == 3) BDS_FWD(3, false);
    else BDS_FWD(4, false);
  }
#undef BDS_FWD
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int64_t bds_rasterize_split_pool_ints(int C, int tile_w, int tile_h, int split_cap, int64_t split_pool, int64_t M_capacity) {
  if (C < 1 || tile_w < 1 || tile_h < 1 || split_cap < 0 || split_pool < 0 || M_capacity < 0) return 0;
  const int64_t total = (int64_t)C * tile_w * tile_h, cap = split_cap < total ? split_cap : total;
  // [ref_off | ref_cnt | pool | uint16 masks[M_capacity]] behind bds_rasterize_schedule_ints words
  return split_pool > 0 ? 2 * cap + split_pool + (M_capacity + 1) / 2 : 0;
}

extern "C" int64_t bds_rasterize_schedule_ints(int C, int tile_w, int tile_h) {
  if (C < 1 || tile_w < 1 || tile_h < 1) return 0;
  const int64_t total = (int64_t)C * tile_w * tile_h;
  return split_area_offset(total) + kSplitHead + 2 * total;   // (+ the split launch's long-tile flags and list)
}

extern "C" int bds_rasterize_bwd_schedule_sort(int C, int tile_w, int tile_h, int32_t *tile_order, bds_stream_t stream) {
  BDS_REQUIRE(C >= 1 && tile_w > 0 && tile_h > 0 && tile_order);
  if (option_get(kOptSchedBins) != 0) return BDS_OK;   // (binned form: bds_rasterize_fwd left the finished schedule)
  const int total = C * tile_w * tile_h;
  hipLaunchKernelGGL(tile_order_kernel, dim3(8), dim3(kSchedThreads), 0, as_stream(stream), total, tile_order + 1 + total, tile_order + 1,
                     tile_order);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

static int rasterize_bwd_impl(int C, int64_t n_records, int64_t M, const uint64_t *M_dev, int CH, const float *records,
                              const float *backgrounds, int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h,
                              const int32_t *isect_offsets, const int32_t *flatten, const float *alphas, const float *t_final,
                              const int32_t *last_ids, const float *v_render, const float *v_alphas, float *v_records, int absgrad,
                              const int32_t *tile_order, int split_len, int split_cap, int64_t split_pool, bds_stream_t stream,
                              const EdEpilogue *epi) {
  BDS_REQUIRE(C >= 1 && n_records >= 0 && M >= 0 && W > 0 && H > 0);
  BDS_REQUIRE(tile_size == kTile);
  ListGeom lg;
  BDS_REQUIRE(list_geom(C, W, H, list_tile_size, lg));
  BDS_REQUIRE(tile_w == (W + kTile - 1) / kTile && tile_h == (H + kTile - 1) / kTile);
  BDS_REQUIRE(CH == 1 || CH == 3 || CH == 4);
  if (M == 0 && !epi) return BDS_OK;
  BDS_REQUIRE(records && isect_offsets && flatten && alphas && last_ids && v_records && (epi || (v_render && v_alphas)));
  BDS_REQUIRE(aligned16(records) && aligned16(v_records));
  const dim3 grid((unsigned)(C * tile_w * tile_h));
  hipStream_t st = as_stream(stream);
  const float4 *rec = reinterpret_cast<const float4 *>(records);
  if (epi) {   // one camera, RGB+ED, no backgrounds: the colour transform's deferred epilogue runs in the kernel's prologue
    BDS_REQUIRE(C == 1 && CH == 4 && backgrounds == nullptr);
#define BDS_BWD_EPI(ab, co)                                                                                                              \
  hipLaunchKernelGGL((rasterize_bwd_epi_kernel<ab, co>), grid, dim3(kWave), 0, st, M, M_dev, rec, W, H, tile_w, tile_h, isect_offsets, \
                     flatten, alphas, t_final, last_ids, v_records, tile_order, lg, *epi)
    if (absgrad) { if (lg.div > 1) BDS_BWD_EPI(true, true); else BDS_BWD_EPI(true, false); }
    else         { if (lg.div > 1) BDS_BWD_EPI(false, true); else BDS_BWD_EPI(false, false); }
#undef BDS_BWD_EPI
    BDS_LAUNCH_CHECK();
    return BDS_OK;
  }
  // (kStrip = false: measured on the benchmark scene, skipping untouched 16 x 4 strips costs the backward 3 % -- its per-pixel
  // body is long enough that the extra control flow outweighs the ~19 % of strips it would skip; the forward gains 7 %)
#define BDS_BWD(ch, ab, co)                                                                                                                 \
  hipLaunchKernelGGL((rasterize_bwd_wave_kernel<ch, ab, co, false>), grid, dim3(kWave), 0, st, C, M, M_dev, rec, backgrounds, W, H, tile_w, \
                     tile_h, isect_offsets, flatten, alphas, t_final, last_ids, v_render, v_alphas, v_records, tile_order, lg)
#define BDS_BWD_CH(ab, co)            \
  do {                                \
    if (CH == 1) BDS_BWD(1, ab, co);  \
    else if (CH == 3) BDS_BWD(3, ab, co); \
    else BDS_BWD(4, ab, co);          \
  } while (0)
  if (split_len > 0 && CH == 4 && lg.div > 1) {      // long tiles strip by strip: the forward left their list behind the schedule
    BDS_REQUIRE(C == 1 && tile_order && option_get(kOptSchedBins) != 0 && split_cap > 0);
    const int total = tile_w * tile_h, cap = split_cap < total ? split_cap : total;
    const int32_t *area = tile_order + split_area_offset(total);
    if (lg.div > 4) split_pool = 0;      // (as the forward: no refined lists for list tiles of more than 4 x 4 tiles)
    const dim3 sgrid((unsigned)(4 * cap + total));
    if (absgrad)
      hipLaunchKernelGGL((rasterize_bwd_split_kernel<4, true>), sgrid, dim3(kWave), 0, st, C, M, M_dev, rec, backgrounds, W, H, tile_w, tile_h,
                         isect_offsets, flatten, alphas, t_final, last_ids, v_render, v_alphas, v_records, tile_order, lg, area, cap, (int)split_pool);
    else
      hipLaunchKernelGGL((rasterize_bwd_split_kernel<4, false>), sgrid, dim3(kWave), 0, st, C, M, M_dev, rec, backgrounds, W, H, tile_w, tile_h,
                         isect_offsets, flatten, alphas, t_final, last_ids, v_render, v_alphas, v_records, tile_order, lg, area, cap, (int)split_pool);
  } else if (absgrad) {
    if (lg.div > 1) BDS_BWD_CH(true, true);
    else BDS_BWD_CH(true, false);
  } else {
    if (lg.div > 1) BDS_BWD_CH(false, true);
    else BDS_BWD_CH(false, false);
  }
#undef BDS_BWD_CH
#undef BDS_BWD
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_rasterize_bwd(int C, int64_t n_records, int64_t M, const uint64_t *M_dev, int CH, const float *records,
                                 const float *backgrounds, int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h,
                                 const int32_t *isect_offsets, const int32_t *flatten, const float *alphas, const float *t_final,
                                 const int32_t *last_ids, const float *v_render, const float *v_alphas, float *v_records, int absgrad,
                                 const int32_t *tile_order, int split_len, int split_cap, int64_t split_pool, bds_stream_t stream) {
  // (the long-tile list of a split launch is left by the device-count forward: the host-count form has none)
  BDS_REQUIRE(M_dev ? (M > 0 && split_len >= 0 && split_cap >= 0 && split_pool >= 0 && split_pool < ((int64_t)1 << 31)) : split_len == 0);
  return rasterize_bwd_impl(C, n_records, M, M_dev, CH, records, backgrounds, W, H, tile_size, list_tile_size, tile_w, tile_h, isect_offsets,
                            flatten, alphas, t_final, last_ids, v_render, v_alphas, v_records, absgrad, tile_order, split_len, split_cap,
                            split_pool, stream, nullptr);
}

extern "C" int bds_rasterize_bwd_ms(int64_t n_records, int64_t M_capacity, const uint64_t *M_dev, const float *records, int W, int H,
                                    int tile_size, int list_tile_size, int tile_w, int tile_h, const int32_t *isect_offsets,
                                    const int32_t *flatten, const float *alphas, const float *t_final, const int32_t *last_ids,
                                    float *v_records, int absgrad, const int32_t *tile_order, int nlevels, const bds_bilagrid_level_t *levels, void *ms_ws,
                                    size_t ms_ws_bytes, const float *render, const float *sky, const float *v_depth,
                                    const float *v_alpha_in, const float *v_direct, float *v_sky, bds_stream_t stream) {
  BDS_REQUIRE(render && v_direct && aligned16(render) && aligned16(v_direct) && (sky != nullptr || v_sky == nullptr));
  EdEpilogue e;
  const int rc = ed_epilogue_fill(nlevels, levels, H, W, ms_ws, ms_ws_bytes, &e);
  if (rc != BDS_OK) return rc;
  e.v_direct = v_direct; e.render = render; e.sky = sky; e.v_depth = v_depth; e.v_alpha_in = v_alpha_in; e.v_sky = v_sky;
  return rasterize_bwd_impl(1, n_records, M_capacity, M_dev, 4, records, nullptr, W, H, tile_size, list_tile_size, tile_w, tile_h,
                            isect_offsets, flatten, alphas, t_final, last_ids, nullptr, nullptr, v_records, absgrad, tile_order, 0, 0, 0, stream, &e);
}

extern "C" int bds_rasterize_bwd_schedule(int C, int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h,
                                          const int32_t *isect_offsets, const int32_t *last_ids, int32_t *tile_order,
                                          bds_stream_t stream) {
  BDS_REQUIRE(C >= 1 && W > 0 && H > 0);
  BDS_REQUIRE(tile_size == kTile);
  ListGeom lg;
  BDS_REQUIRE(list_geom(C, W, H, list_tile_size, lg));
  BDS_REQUIRE(tile_w == (W + kTile - 1) / kTile && tile_h == (H + kTile - 1) / kTile);
  BDS_REQUIRE(isect_offsets && last_ids && tile_order);
  const int total = C * tile_w * tile_h;
  hipStream_t st = as_stream(stream);
  int32_t *work = tile_order + 1 + total;   // [tag | order | work] (pick_item)
  constexpr int per_block = kWorkBlock / kWave;
  hipLaunchKernelGGL(tile_work_kernel, dim3((unsigned)((total + per_block - 1) / per_block)), dim3(kWorkBlock), 0, st, C, W,
                     H, tile_w, tile_h, isect_offsets, last_ids, work, lg);
  hipLaunchKernelGGL(tile_order_kernel, dim3(8), dim3(kSchedThreads), 0, st, total, work, tile_order + 1, tile_order);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

// Name of the compositor kernel a launch with these switches runs, as rocprofv3 prints it (bench.py looks the dominant kernel's
// counters up under this name in profiles/: the name lives next to the template it describes, not in the benchmark)
extern "C" int bds_rasterize_kernel_name(int backward, int CH, int absgrad, int list_tile_size, char *buf, int buf_len) {
  BDS_REQUIRE(buf && buf_len > 0 && (CH == 1 || CH == 3 || CH == 4) && list_tile_size >= kTile && list_tile_size % kTile == 0);
  const char *co = list_tile_size > kTile ? "true" : "false";
  int n;
  if (backward == 2)   // with the colour transform's deferred epilogue (bds_rasterize_bwd_ms)
    n = snprintf(buf, (size_t)buf_len, "rasterize_bwd_epi_kernel<%s, %s>", absgrad ? "true" : "false", co);
  else if (backward) n = snprintf(buf, (size_t)buf_len, "rasterize_bwd_wave_kernel<%d, %s, %s, false>", CH, absgrad ? "true" : "false", co);
  else n = snprintf(buf, (size_t)buf_len, "rasterize_fwd_wave_kernel<%d, %s, true>", CH, co);
  return (n > 0 && n < buf_len) ? BDS_OK : BDS_EINVAL;
}
