// Deformation network of deformable Gaussians, forward and backward: ConditionalDeformNetwork / DeformNetwork
// (reference models/modules.py:925-1012) at the shipped size D = 8, W = 256, x / t multires 10, input_ch 3, embed_dim
// 16 (DeformableNodes, models/nodes/deformable.py:35-47) or no condition (DeformableGaussians, models/gaussians/deformgs.py:62-72).
//   h0 = [emb(x) 63 | emb(t) 21 | cond E]  (K0 = 84 + E columns)  -> 8 x (Linear + ReLU), layer 5 reading [h0 | h4]
//   -> gaussian_warp [3] / gaussian_rotation [4] / gaussian_scaling [3] (each Linear from W).
// All products are v_mfma_f32_32x32x2_f32 (exact f32 in, f32 accumulate: parity with the f32 reference; there is no xf32 on gfx950).
//
// Design (one workgroup = 4 waves = one tile of 32 points):
//   * activations are kept in LDS as [point][neuron] rows (stride 260 floats), never in HBM on the forward.  Wave w computes neurons
//     64 w .. 64 w + 63 of the next layer as two 32 x 32 D tiles (rows = neurons, columns = the 32 points) with the layer's weights as
//     the A operand, read straight from global memory (each layer is 256 KB, more than LDS holds; the 2.1 MB of the whole network stay
//     L2-resident across the workgroups of an XCD) as 16-byte row segments, and the LDS rows as the B operand (two 16-byte LDS reads per
//     8 MFMAs).  After a barrier the tiles go back to the same LDS rows with bias and ReLU.  The encoding rows are computed once per
//     tile in LDS (accurate sinf / cosf, csrc/deform_math.h) and read twice: by layer 0 and by the skip layer 5.
//   * the three heads are one padded 32-row tile (rows 0-2 warp, 3-6 rotation, 7-9 scaling), computed by wave 0.
//   * backward, in chunks of kDfChunk points: (1) deform_bwd_data recomputes the forward of its tile, runs the transposed chain
//     (A operand = W^T read column-wise; the ReLU masks of the recompute are kept as one bit per point in LDS) and writes the
//     gradients of cond / x / t; it STASHES the encoding rows, the 8 activations and the 8 pre-activation gradients of the chunk in the
//     caller's workspace (16.9 KB per point).  (2) deform_wgrad forms every weight and bias gradient as a long-K product over the
//     chunk's points, 64 x 64 output tiles x kDfSplit point ranges, each writing its own partial.  (3) deform_wreduce sums the partials
//     in a fixed order and stores (first chunk) or adds (later chunks) the result: deterministic, no float atomics.  Recomputing the
//     activations inside (2) instead would repeat the whole forward per output tile; a stash for all N points would cost 16.9 KB per
//     point (5 GB at 300 k points): the chunked stash bounds the workspace at bds_deform_bwd_temp_bytes (about 294 MB for N >= 16384).
// Bound: the FP32 MFMA rate, 2 * 0.51 M flop per point forward, three times that for forward + backward.
#include "bds_common.h"
#include "deform_math.h"
#include "mfma_tile.h"

namespace bds {

constexpr int kDfW = 256, kDfLayers = 8, kDfSkip = 5;
constexpr int kDfP = 32;          // points per workgroup
constexpr int kDfBlock = 256;       // four waves
constexpr int kDfSH = kDfW + 4;   // LDS row stride of the activations
constexpr int kDfGS = 16;         // head-gradient row (10 used)
constexpr int kDfChunk = 16384;   // backward chunk (points); a multiple of 32 * kDfSplit
constexpr int kDfSplit = 8;       // point ranges per weight-gradient tile and chunk
constexpr int kDfTileFloats = 64 * 64 + 64;   // one partial: 64 x 64 weight entries + 64 bias entries
constexpr int kDfJobs = kDfLayers + 1;        // 8 hidden layers + the heads

template <int E>
struct DfShape {
  static constexpr int K0 = kDfXEmb + kDfTEmb + E;     // 84 / 100
  static constexpr int K0P = (K0 + 15) / 16 * 16;      // 96 / 112
  static constexpr int SE = K0P + 4;
};

struct DfNet {
  const float *w[kDfLayers], *b[kDfLayers];
  const float *warp_w, *warp_b, *rot_w, *rot_b, *scale_w, *scale_b;
};

// head row r (0-2 warp, 3-6 rotation, 7-9 scaling) of the padded head tile; NULL for a head that is off and for the padding
__device__ __forceinline__ const float *df_head_row(const DfNet &net, int r, bool bias) {
  if (r < 3) return bias ? net.warp_b + r : net.warp_w + r * kDfW;
  if (r < 7) return net.rot_w ? (bias ? net.rot_b + (r - 3) : net.rot_w + (r - 3) * kDfW) : nullptr;
  if (r < 10) return net.scale_w ? (bias ? net.scale_b + (r - 7) : net.scale_w + (r - 7) * kDfW) : nullptr;
  return nullptr;
}

// encoding rows of the tile's 32 points: eT[p][c], zero past K0 (the padded k steps multiply zeros)
template <int E>
__device__ __forceinline__ void df_encode(float *__restrict__ eT, int64_t base, int64_t N, const float *__restrict__ x,
                                          const float *__restrict__ t, const float *__restrict__ cond) {
  using S = DfShape<E>;
  for (int i = threadIdx.x; i < kDfP * S::K0P; i += kDfBlock) {
    const int p = i / S::K0P, c = i % S::K0P;
    const int64_t g = base + p < N ? base + p : N - 1;
    float v = 0.f;
    if (c < kDfXEmb) v = df_embed_col<3>(x + g * 3, c);
    else if (c < kDfXEmb + kDfTEmb) v = df_embed_col<1>(t + g, c - kDfXEmb);
    else if (c < S::K0) v = cond[g * E + (c - kDfXEmb - kDfTEmb)];
    eT[p * S::SE + c] = v;
  }
}

// acc[o] += sum_k wr[o][k] * B[col][k], k < Kp (a multiple of 16; wr entries past K -- a multiple of 4 -- read as zero).  Lane (col,
// half) takes k = kc + 8 half + s at step s: 16-byte reads of its weight row (A: row = lane col) and of its point's LDS row (B).
template <int NO>
__device__ __forceinline__ void df_gemm_rows(acc16 (&acc)[NO], const float *const (&wr)[NO], int K, int Kp, const float *__restrict__ B,
                                             int bs, int col, int half) {
  const float *brow = B + col * bs + 8 * half;
  for (int kc = 0; kc < Kp; kc += 16) {
    const float4 b0 = *reinterpret_cast<const float4 *>(brow + kc), b1 = *reinterpret_cast<const float4 *>(brow + kc + 4);
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const int k = kc + 8 * half;
#pragma unroll
    for (int o = 0; o < NO; o++) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a0 = (wr[o] && k < K) ? *reinterpret_cast<const float4 *>(wr[o] + k) : z;
      const float4 a1 = (wr[o] && k + 4 < K) ? *reinterpret_cast<const float4 *>(wr[o] + k + 4) : z;
      const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int s = 0; s < 8; s++) acc[o] = mfma(a[s], b[s], acc[o]);
    }
  }
}

// transposed: acc[o] += sum_n wc[o][n * ldw] * B[col][n], n < 256 (wc = a weight COLUMN, NULL reads zero)
template <int NO>
__device__ __forceinline__ void df_gemm_cols(acc16 (&acc)[NO], const float *const (&wc)[NO], int ldw, const float *__restrict__ B, int bs,
                                             int col, int half) {
  const float *brow = B + col * bs + 8 * half;
  for (int kc = 0; kc < kDfW; kc += 16) {
    const float4 b0 = *reinterpret_cast<const float4 *>(brow + kc), b1 = *reinterpret_cast<const float4 *>(brow + kc + 4);
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const int64_t n = kc + 8 * half;
#pragma unroll
    for (int o = 0; o < NO; o++) {
      float a[8];
#pragma unroll
      for (int s = 0; s < 8; s++) a[s] = wc[o] ? wc[o][(n + s) * ldw] : 0.f;
#pragma unroll
      for (int s = 0; s < 8; s++) acc[o] = mfma(a[s], b[s], acc[o]);
    }
  }
}

// D tile (rows nb + d_row(r, half), column = point col) -> dst[col * stride + row]: four consecutive rows per register group
__device__ __forceinline__ void df_store_tile(float *__restrict__ dst, int stride, int nb, int col, int half, const acc16 &v) {
#pragma unroll
  for (int q = 0; q < 4; q++)
    *reinterpret_cast<float4 *>(dst + (int64_t)col * stride + nb + 8 * q + 4 * half) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// the 8 hidden layers of one tile: on return hT holds a_7.  STASH: also the activations a_i to stash + i * C * 256 (rows of the
// chunk) and the ReLU masks (bit p of masks[i * 256 + neuron]).
template <int E, bool STASH>
__device__ __forceinline__ void df_hidden(const DfNet &net, const float *__restrict__ eT, float *__restrict__ hT, uint32_t *__restrict__ masks,
                                          float *__restrict__ stash, int64_t C, int64_t lrow, int wave, int col, int half) {
  using S = DfShape<E>;
  for (int i = 0; i < kDfLayers; i++) {
    const int ldw = i == 0 ? S::K0 : (i == kDfSkip ? S::K0 + kDfW : kDfW);
    acc16 acc[2];
    const float *wr[2];
#pragma unroll
    for (int o = 0; o < 2; o++) {
      const int nb = 64 * wave + 32 * o;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[o][r] = net.b[i][nb + d_row(r, half)];
      wr[o] = net.w[i] + (int64_t)(nb + col) * ldw;
    }
    if (i == 0 || i == kDfSkip) df_gemm_rows<2>(acc, wr, S::K0, S::K0P, eT, S::SE, col, half);
    if (i != 0) {
      const int c0 = i == kDfSkip ? S::K0 : 0;
      const float *wh[2] = {wr[0] + c0, wr[1] + c0};
      df_gemm_rows<2>(acc, wh, kDfW, kDfW, hT, kDfSH, col, half);
    }
    __syncthreads();   // every wave has read the previous activations
#pragma unroll
    for (int o = 0; o < 2; o++) {
      const int nb = 64 * wave + 32 * o;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[o][r] = fmaxf(acc[o][r], 0.f);
      df_store_tile(hT, kDfSH, nb, col, half, acc[o]);
      if (STASH) {
        df_store_tile(stash + (int64_t)i * C * kDfW + lrow * kDfW, kDfW, nb, col, half, acc[o]);
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const uint64_t bits = __ballot(acc[o][r] > 0.f);
          if (col == 0) masks[i * kDfW + nb + d_row(r, half)] = half ? (uint32_t)(bits >> 32) : (uint32_t)bits;
        }
      }
    }
    __syncthreads();
  }
}

template <int E>
__global__ __launch_bounds__(kDfBlock) void deform_fwd_kernel(int64_t N, const float *__restrict__ x, const float *__restrict__ t,
                                                              const float *__restrict__ cond, DfNet net, float *__restrict__ d_xyz,
                                                              float *__restrict__ rot, float *__restrict__ scale) {
  using S = DfShape<E>;
  __shared__ __attribute__((aligned(16))) float eT[kDfP * S::SE];
  __shared__ __attribute__((aligned(16))) float hT[kDfP * kDfSH];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, col = lane & 31, half = lane >> 5;
  const int64_t base = (int64_t)blockIdx.x * kDfP;
  df_encode<E>(eT, base, N, x, t, cond);
  __syncthreads();
  df_hidden<E, false>(net, eT, hT, nullptr, nullptr, 0, 0, wave, col, half);
  if (wave != 0) return;
  acc16 acc[1];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const float *bp = df_head_row(net, d_row(r, half), true);
    acc[0][r] = bp ? *bp : 0.f;
  }
  const float *wr[1] = {df_head_row(net, col, false)};
  df_gemm_rows<1>(acc, wr, kDfW, kDfW, hT, kDfSH, col, half);
  const int64_t g = base + col;
  if (g >= N) return;
#pragma unroll
  for (int r = 0; r < 8; r++) {   // rows 0-3 / 8-11 (half 0), 4-7 / 12-15 (half 1)
    const int row = d_row(r, half);
    if (row < 3) d_xyz[g * 3 + row] = acc[0][r];
    else if (row < 7) { if (rot) rot[g * 4 + row - 3] = acc[0][r]; }
    else if (row < 10) { if (scale) scale[g * 3 + row - 7] = acc[0][r]; }
  }
}

// workspace of one chunk of C points (C a multiple of 32): [emb C x K0P | head grads C x 16 | a_0..7 8 x C x 256 | dz_0..7 8 x C x 256]
template <int E>
struct DfStash {
  float *emb, *g, *a, *dz;
  __host__ __device__ DfStash(float *ws, int64_t C) {
    emb = ws;
    g = emb + C * DfShape<E>::K0P;
    a = g + C * kDfGS;
    dz = a + (int64_t)kDfLayers * C * kDfW;
  }
  static constexpr size_t floats(int64_t C) { return (size_t)C * (DfShape<E>::K0P + kDfGS + 2 * kDfLayers * kDfW); }
};

// one tile of the chunk [p0, p1): recompute + stash, the data path backward, the gradients of cond / x / t
template <int E>
__global__ __launch_bounds__(kDfBlock) void deform_bwd_data_kernel(int64_t N, int64_t p0, int64_t p1, int64_t C, const float *__restrict__ x,
                                                                   const float *__restrict__ t, const float *__restrict__ cond, DfNet net,
                                                                   const float *__restrict__ v_xyz, const float *__restrict__ v_rot,
                                                                   const float *__restrict__ v_scale, float *__restrict__ v_x,
                                                                   float *__restrict__ v_t, float *__restrict__ v_cond, float *__restrict__ ws) {
  using S = DfShape<E>;
  __shared__ __attribute__((aligned(16))) float eT[kDfP * S::SE];
  __shared__ __attribute__((aligned(16))) float hT[kDfP * kDfSH];
  __shared__ __attribute__((aligned(16))) float gT[kDfP * kDfGS];
  __shared__ uint32_t masks[kDfLayers * kDfW];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, col = lane & 31, half = lane >> 5;
  const int64_t lrow = (int64_t)blockIdx.x * kDfP, base = p0 + lrow;
  DfStash<E> st(ws, C);
  df_encode<E>(eT, base, N, x, t, cond);
  __syncthreads();
  for (int i = threadIdx.x; i < kDfP * S::K0P; i += kDfBlock) st.emb[lrow * S::K0P + i] = eT[(i / S::K0P) * S::SE + i % S::K0P];
  df_hidden<E, true>(net, eT, hT, masks, st.a, C, lrow, wave, col, half);

  // output gradients in the head tile's row order; zero past the chunk (silences every weight-gradient term of those rows)
  for (int i = threadIdx.x; i < kDfP * kDfGS; i += kDfBlock) {
    const int p = i / kDfGS, r = i % kDfGS;
    const int64_t g = base + p;
    float v = 0.f;
    if (g < p1) {
      if (r < 3) v = v_xyz ? v_xyz[g * 3 + r] : 0.f;
      else if (r < 7) v = (v_rot && net.rot_w) ? v_rot[g * 4 + r - 3] : 0.f;
      else if (r < 10) v = (v_scale && net.scale_w) ? v_scale[g * 3 + r - 7] : 0.f;
    }
    gT[i] = v;
    st.g[lrow * kDfGS + i] = v;
  }
  __syncthreads();

  // dz_7 = (W_head^T g) * relu'(a_7): k = head row 8 half + s
#pragma unroll
  for (int o = 0; o < 2; o++) {
    const int nb = 64 * wave + 32 * o;
    acc16 acc = zero16();
#pragma unroll
    for (int s = 0; s < 8; s++) {
      const float *hw = df_head_row(net, 8 * half + s, false);
      acc = mfma(hw ? hw[nb + col] : 0.f, gT[col * kDfGS + 8 * half + s], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = ((masks[(kDfLayers - 1) * kDfW + nb + d_row(r, half)] >> col) & 1u) ? acc[r] : 0.f;
    df_store_tile(hT, kDfSH, nb, col, half, acc);
    df_store_tile(st.dz + (int64_t)(kDfLayers - 1) * C * kDfW + lrow * kDfW, kDfW, nb, col, half, acc);
  }
  __syncthreads();

  // layers 7 .. 1: da_{i-1} = W_i^T dz_i (the h columns), dz_{i-1} = da_{i-1} * relu'(a_{i-1}); layer 5 and layer 0 also feed the
  // encoding rows' gradient dE (rows 32 wave + d_row, K0 valid)
  acc16 dE[1] = {zero16()};
  const int me = 32 * wave + col;
  for (int i = kDfLayers - 1; i >= 1; i--) {
    const int ldw = i == kDfSkip ? S::K0 + kDfW : kDfW, c0 = i == kDfSkip ? S::K0 : 0;
    acc16 acc[2] = {zero16(), zero16()};
    const float *wc[2] = {net.w[i] + c0 + 64 * wave + col, net.w[i] + c0 + 64 * wave + 32 + col};
    df_gemm_cols<2>(acc, wc, ldw, hT, kDfSH, col, half);
    if (i == kDfSkip) {
      const float *we[1] = {me < S::K0 ? net.w[i] + me : nullptr};
      df_gemm_cols<1>(dE, we, ldw, hT, kDfSH, col, half);
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < 2; o++) {
      const int nb = 64 * wave + 32 * o;
#pragma unroll
      for (int r = 0; r < 16; r++) acc[o][r] = ((masks[(i - 1) * kDfW + nb + d_row(r, half)] >> col) & 1u) ? acc[o][r] : 0.f;
      df_store_tile(hT, kDfSH, nb, col, half, acc[o]);
      df_store_tile(st.dz + (int64_t)(i - 1) * C * kDfW + lrow * kDfW, kDfW, nb, col, half, acc[o]);
    }
    __syncthreads();
  }
  {
    const float *we[1] = {me < S::K0 ? net.w[0] + me : nullptr};
    df_gemm_cols<1>(dE, we, S::K0, hT, kDfSH, col, half);
  }
  __syncthreads();
  df_store_tile(hT, kDfSH, 32 * wave, col, half, dE[0]);   // hT rows now hold dE[p][0 .. 127]
  __syncthreads();

  // cond / x / t: thread (point p, part q)
  const int p = threadIdx.x >> 3, q = threadIdx.x & 7;
  const int64_t g = base + p;
  if (g >= p1) return;
  const float *de = hT + p * kDfSH, *e = eT + p * S::SE;
  if (q < 3) {
    if (v_x) {
      float s = de[q];
      for (int k = 0; k < kDfMultires; k++)
        s += (float)(1 << k) * (e[6 + 6 * k + q] * de[3 + 6 * k + q] - e[3 + 6 * k + q] * de[6 + 6 * k + q]);
      v_x[g * 3 + q] = s;
    }
  } else if (q == 3) {
    if (v_t) {
      constexpr int o = kDfXEmb;
      float s = de[o];
      for (int k = 0; k < kDfMultires; k++)
        s += (float)(1 << k) * (e[o + 2 + 2 * k] * de[o + 1 + 2 * k] - e[o + 1 + 2 * k] * de[o + 2 + 2 * k]);
      v_t[g] = s;
    }
  } else if (E > 0 && v_cond) {
#pragma unroll
    for (int c = 4 * (q - 4); c < 4 * (q - 3); c++)
      if (c < E) v_cond[g * E + c] = de[kDfXEmb + kDfTEmb + c];
  }
}

// weight-gradient jobs: G[n][m] = sum_p dz[p][n] in[p][m], in = [in1 (k1 columns) | in2 (k2 columns)], n < nn; bias: sum_p dz[p][n]
struct DfJob {
  const float *dz, *in1, *in2;
  int ldz, nn, ld1, k1, ld2, k2;
  int tile0, tm;     // first tile, tiles along m (64 columns each)
  int64_t e0;        // first entry in the reduce's flat order (weights n * (k1 + k2) + m, then the nn biases)
};
struct DfJobs {
  DfJob j[kDfJobs];
  int tiles;
  int64_t entries;
};
struct DfGrad {
  float *w[kDfLayers], *b[kDfLayers];
  float *warp_w, *warp_b, *rot_w, *rot_b, *scale_w, *scale_b;
};

// one 64 x 64 tile of one job over point range split blockIdx.y of the chunk's `rows` (a multiple of 32) -> its partial
__global__ __launch_bounds__(kDfBlock) void deform_wgrad_kernel(DfJobs jobs, int64_t rows, float *__restrict__ partials) {
  const int tile = blockIdx.x, split = blockIdx.y;
  int jj = 0;
  while (jj + 1 < kDfJobs && tile >= jobs.j[jj + 1].tile0) jj++;
  const DfJob &J = jobs.j[jj];
  const int local = tile - J.tile0, tn = local / J.tm, tmi = local % J.tm;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave, col = lane & 31, half = lane >> 5;
  const int nl = 32 * (wave & 1), ml = 32 * (wave >> 1);
  const int n = 64 * tn + nl + col, m = 64 * tmi + ml + col;
  const float *pa = n < J.nn ? J.dz + n : nullptr;
  const float *pb = m < J.k1 ? J.in1 + m : (m < J.k1 + J.k2 ? J.in2 + (m - J.k1) : nullptr);
  const int64_t lda = J.ldz, ldb = m < J.k1 ? J.ld1 : J.ld2;
  const int64_t per = (rows / 32 + kDfSplit - 1) / kDfSplit * 32;
  const int64_t ps = split * per, pe = ps + per < rows ? ps + per : rows;
  acc16 acc = zero16();
  float bsum = 0.f;
  for (int64_t p = ps; p < pe; p += 16) {
    const int64_t pp = p + 8 * half;
    float a[8], b[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
      a[s] = pa ? pa[(pp + s) * lda] : 0.f;
      b[s] = pb ? pb[(pp + s) * ldb] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 8; s++) {
      acc = mfma(a[s], b[s], acc);
      bsum += a[s];
    }
  }
  float *part = partials + ((int64_t)tile * kDfSplit + split) * kDfTileFloats;
#pragma unroll
  for (int r = 0; r < 16; r++) part[(nl + d_row(r, half)) * 64 + ml + col] = acc[r];
  if (ml == 0) {
    bsum += __shfl_xor(bsum, 32);
    if (half == 0) part[64 * 64 + nl + col] = bsum;
  }
}

// every gradient entry: the kDfSplit partials in order, then stored (accumulate == 0) or added
__global__ __launch_bounds__(256) void deform_wreduce_kernel(DfJobs jobs, DfGrad out, int accumulate, const float *__restrict__ partials) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= jobs.entries) return;
  int jj = 0;
  while (jj + 1 < kDfJobs && e >= jobs.j[jj + 1].e0) jj++;
  const DfJob &J = jobs.j[jj];
  const int K = J.k1 + J.k2;
  const int64_t local = e - J.e0;
  int n, m, tile, idx;
  const bool is_w = local < (int64_t)J.nn * K;
  if (is_w) {
    n = (int)(local / K); m = (int)(local % K);
    tile = J.tile0 + (n / 64) * J.tm + m / 64;
    idx = (n % 64) * 64 + m % 64;
  } else {
    n = (int)(local - (int64_t)J.nn * K); m = 0;
    tile = J.tile0 + (n / 64) * J.tm;
    idx = 64 * 64 + n % 64;
  }
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < kDfSplit; q++) s += partials[((int64_t)tile * kDfSplit + q) * kDfTileFloats + idx];
  float *dst;
  if (jj < kDfLayers) dst = is_w ? (out.w[jj] ? out.w[jj] + (int64_t)n * K + m : nullptr) : (out.b[jj] ? out.b[jj] + n : nullptr);
  else if (n < 3) dst = is_w ? (out.warp_w ? out.warp_w + n * K + m : nullptr) : (out.warp_b ? out.warp_b + n : nullptr);
  else if (n < 7) dst = is_w ? (out.rot_w ? out.rot_w + (n - 3) * K + m : nullptr) : (out.rot_b ? out.rot_b + n - 3 : nullptr);
  else dst = is_w ? (out.scale_w ? out.scale_w + (n - 7) * K + m : nullptr) : (out.scale_b ? out.scale_b + n - 7 : nullptr);
  if (dst) *dst = accumulate ? *dst + s : s;
}

static DfNet df_net(const bds_deform_net *n) {
  DfNet d;
  for (int i = 0; i < kDfLayers; i++) { d.w[i] = n->w[i]; d.b[i] = n->b[i]; }
  d.warp_w = n->warp_w; d.warp_b = n->warp_b;
  d.rot_w = n->rot_w; d.rot_b = n->rot_b;
  d.scale_w = n->scale_w; d.scale_b = n->scale_b;
  return d;
}

static bool df_net_ok(const bds_deform_net *n) {
  if (!n || !n->warp_w || !n->warp_b || !n->rot_w != !n->rot_b || !n->scale_w != !n->scale_b) return false;
  for (int i = 0; i < kDfLayers; i++)
    if (!n->w[i] || !n->b[i] || !aligned16(n->w[i])) return false;
  if (!aligned16(n->warp_w) || (n->rot_w && !aligned16(n->rot_w)) || (n->scale_w && !aligned16(n->scale_w))) return false;
  return true;
}

static int64_t df_chunk(int64_t N) { return N < kDfChunk ? cdiv(N, kDfP) * kDfP : kDfChunk; }

template <int E>
static DfJobs df_jobs(const DfStash<E> &st, int64_t C) {
  using S = DfShape<E>;
  DfJobs J;
  int tile = 0;
  int64_t e = 0;
  for (int i = 0; i < kDfJobs; i++) {
    DfJob &j = J.j[i];
    j.dz = i < kDfLayers ? st.dz + (int64_t)i * C * kDfW : st.g;
    j.ldz = i < kDfLayers ? kDfW : kDfGS;
    j.nn = i < kDfLayers ? kDfW : 10;
    j.in2 = nullptr; j.ld2 = kDfW; j.k2 = 0;
    if (i == 0 || i == kDfSkip) { j.in1 = st.emb; j.ld1 = S::K0P; j.k1 = S::K0; }
    else { j.in1 = st.a + (int64_t)(i - 1) * C * kDfW; j.ld1 = kDfW; j.k1 = kDfW; }
    if (i == kDfSkip) { j.in2 = st.a + (int64_t)(kDfSkip - 1) * C * kDfW; j.k2 = kDfW; }
    if (i == kDfLayers) { j.in1 = st.a + (int64_t)(kDfLayers - 1) * C * kDfW; j.ld1 = kDfW; j.k1 = kDfW; }
    j.tm = (j.k1 + j.k2 + 63) / 64;
    j.tile0 = tile;
    tile += (j.nn + 63) / 64 * j.tm;
    j.e0 = e;
    e += (int64_t)j.nn * (j.k1 + j.k2) + j.nn;
  }
  J.tiles = tile;
  J.entries = e;
  return J;
}

template <int E>
static size_t df_temp_bytes(int64_t N) {
  const int64_t C = df_chunk(N);
  const DfStash<E> st(nullptr, C);
  const DfJobs J = df_jobs<E>(st, C);
  return (DfStash<E>::floats(C) + (size_t)J.tiles * kDfSplit * kDfTileFloats) * sizeof(float);
}

template <int E>
static int df_launch_bwd(int64_t N, const float *x, const float *t, const float *cond, const DfNet &net, const float *v_xyz,
                         const float *v_rot, const float *v_scale, float *v_x, float *v_t, float *v_cond, const DfGrad &grad, bool want_w,
                         int accumulate, float *ws, hipStream_t st) {
  const int64_t C = df_chunk(N);
  const DfStash<E> sh(ws, C);
  const DfJobs J = df_jobs<E>(sh, C);
  float *partials = ws + DfStash<E>::floats(C);
  for (int64_t p0 = 0; p0 < N; p0 += C) {
    const int64_t p1 = p0 + C < N ? p0 + C : N, rows = cdiv(p1 - p0, kDfP) * kDfP;
    hipLaunchKernelGGL(deform_bwd_data_kernel<E>, dim3((unsigned)(rows / kDfP)), dim3(kDfBlock), 0, st, N, p0, p1, C, x, t, cond, net, v_xyz,
                       v_rot, v_scale, v_x, v_t, v_cond, ws);
    BDS_LAUNCH_CHECK();
    if (!want_w) continue;
    hipLaunchKernelGGL(deform_wgrad_kernel, dim3((unsigned)J.tiles, kDfSplit), dim3(kDfBlock), 0, st, J, rows, partials);
    BDS_LAUNCH_CHECK();
    hipLaunchKernelGGL(deform_wreduce_kernel, dim3((unsigned)cdiv(J.entries, 256)), dim3(256), 0, st, J, grad,
                       (accumulate || p0 > 0) ? 1 : 0, (const float *)partials);
    BDS_LAUNCH_CHECK();
  }
  return BDS_OK;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_deform_supported(int D, int W, int x_multires, int t_multires, int input_ch, int embed_dim) {
  return D == kDfLayers && W == kDfW && x_multires == kDfMultires && t_multires == kDfMultires && input_ch == 3 &&
         (embed_dim == 0 || embed_dim == 16);
}

extern "C" size_t bds_deform_bwd_temp_bytes(int64_t N, int embed_dim) {
  if (N <= 0 || (embed_dim != 0 && embed_dim != 16)) return 0;
  return embed_dim ? df_temp_bytes<16>(N) : df_temp_bytes<0>(N);
}

extern "C" int bds_deform_fwd(int64_t N, int embed_dim, const float *x, const float *t, const float *cond, const bds_deform_net *net,
                              float *d_xyz, float *rotation, float *scaling, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && (embed_dim == 0 || embed_dim == 16));
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(x && t && (embed_dim == 0 || cond) && df_net_ok(net) && d_xyz);
  BDS_REQUIRE((!rotation || net->rot_w) && (!scaling || net->scale_w));
  const DfNet dn = df_net(net);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)cdiv(N, kDfP));
  if (embed_dim) hipLaunchKernelGGL(deform_fwd_kernel<16>, grid, dim3(kDfBlock), 0, st, N, x, t, cond, dn, d_xyz, rotation, scaling);
  else hipLaunchKernelGGL(deform_fwd_kernel<0>, grid, dim3(kDfBlock), 0, st, N, x, t, cond, dn, d_xyz, rotation, scaling);
  BDS_LAUNCH_CHECK();
  return BDS_OK;
}

extern "C" int bds_deform_bwd(int64_t N, int embed_dim, const float *x, const float *t, const float *cond, const bds_deform_net *net,
                              const float *v_xyz, const float *v_rotation, const float *v_scaling, float *v_x, float *v_t, float *v_cond,
                              const bds_deform_net_grad *grad, int accumulate, void *temp, size_t temp_bytes, bds_stream_t stream) {
  BDS_REQUIRE(N >= 0 && (embed_dim == 0 || embed_dim == 16));
  if (N == 0) return BDS_OK;
  BDS_REQUIRE(x && t && (embed_dim == 0 || cond) && df_net_ok(net) && (!v_cond || embed_dim));
  BDS_REQUIRE(temp && temp_bytes >= bds_deform_bwd_temp_bytes(N, embed_dim) && aligned16(temp));
  const DfNet dn = df_net(net);
  DfGrad g = {};
  bool want_w = false;
  if (grad) {
    for (int i = 0; i < kDfLayers; i++) { g.w[i] = grad->w[i]; g.b[i] = grad->b[i]; want_w = want_w || g.w[i] || g.b[i]; }
    g.warp_w = grad->warp_w; g.warp_b = grad->warp_b;
    g.rot_w = net->rot_w ? grad->rot_w : nullptr; g.rot_b = net->rot_w ? grad->rot_b : nullptr;
    g.scale_w = net->scale_w ? grad->scale_w : nullptr; g.scale_b = net->scale_w ? grad->scale_b : nullptr;
    want_w = want_w || g.warp_w || g.warp_b || g.rot_w || g.rot_b || g.scale_w || g.scale_b;
  }
  hipStream_t st = as_stream(stream);
  float *ws = static_cast<float *>(temp);
  if (embed_dim) return df_launch_bwd<16>(N, x, t, cond, dn, v_xyz, v_rotation, v_scaling, v_x, v_t, v_cond, g, want_w, accumulate, ws, st);
  return df_launch_bwd<0>(N, x, t, cond, dn, v_xyz, v_rotation, v_scaling, v_x, v_t, v_cond, g, want_w, accumulate, ws, st);
}
