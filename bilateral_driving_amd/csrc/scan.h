// Workgroup prefix sums and ranks shared by the compaction kernels ("count per workgroup -> exclusive offsets -> emit").  Device only.
// Everything here sums integers, so the results do not depend on the order of the additions.  Every function with an LDS argument
// holds barriers: ALL threads of the workgroup call it, none returns early in front of it.
#pragma once
#include "bds_common.h"

namespace bds {

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// returns the exclusive prefix of `v` within the block and the block total; lds_w (one word per wave) is free again on return.
// WAVES: the block's waves where the caller knows them at compile time, 0: read from blockDim.x
template <int WAVES = 0, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T &total, T *lds_w) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
  const int nw = WAVES ? WAVES : blockDim.x / kWave;
  T inc = wave_incl_scan(v);
  if (lane == kWave - 1) lds_w[wv] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int w = 0; w < nw; w++) {
    T s = lds_w[w];
    if (w < wv) base += s;
    tot += s;
  }
  total = tot;
  __syncthreads();
  return base + inc - v;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t ballot) {      // set bits below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// C predicates per thread, bit c of `bits`.  block_count: thread c < C returns the number of the workgroup's threads with bit c set.
// block_rank: rank[c] = the threads in front of this one with bit c set, for c < channels.  lds_w holds C words per wave and is NOT
// free on return: a barrier goes in front of its next use.
template <int C>
__device__ __forceinline__ void block_ballots(uint32_t bits, uint32_t *rank, uint32_t *lds_w) {
#pragma unroll
  for (int c = 0; c < C; c++) {
    const uint64_t b = __ballot((bits >> c) & 1u);
    rank[c] = lane_rank(b);
    if ((threadIdx.x & (kWave - 1)) == 0) lds_w[(threadIdx.x / kWave) * C + c] = (uint32_t)__popcll(b);
  }
  __syncthreads();
}
template <int C, int WAVES>
__device__ __forceinline__ uint32_t block_count(uint32_t bits, uint32_t *lds_w) {
  uint32_t rank[C], s = 0;
  block_ballots<C>(bits, rank, lds_w);
  if (threadIdx.x < C)
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += lds_w[w * C + threadIdx.x];
  return s;
}
template <int C>
__device__ __forceinline__ void block_rank(uint32_t bits, uint32_t *rank, uint32_t *lds_w, int channels = C) {
  block_ballots<C>(bits, rank, lds_w);
#pragma unroll
  for (int c = 0; c < C; c++)
    if (c < channels)
      for (int w = 0; w < (int)(threadIdx.x / kWave); w++) rank[c] += lds_w[w * C + c];
}

// One workgroup of THREADS: the table data[n][C] -> the exclusive prefix sums of its C columns, in place; total[c] = column c's sum,
// in every thread.  Thread t owns the contiguous rows [t seg, (t + 1) seg), seg = ceil(n / THREADS); lds_w as block_excl_scan's.
template <int THREADS, int C = 1, typename T>
__device__ __forceinline__ void workgroup_scan_in_place(T *data, int64_t n, T *total, T *lds_w) {
  const int64_t seg = (n + THREADS - 1) / THREADS;
  const int64_t lo = threadIdx.x * seg < n ? threadIdx.x * seg : n, hi = lo + seg < n ? lo + seg : n;
  T run[C];
#pragma unroll
  for (int c = 0; c < C; c++) run[c] = 0;
  for (int64_t i = lo; i < hi; i++)
#pragma unroll
    for (int c = 0; c < C; c++) run[c] += data[i * C + c];
#pragma unroll
  for (int c = 0; c < C; c++) run[c] = block_excl_scan<THREADS / kWave>(run[c], total[c], lds_w);
  for (int64_t i = lo; i < hi; i++)
#pragma unroll
    for (int c = 0; c < C; c++) {
      const T v = data[i * C + c];
      data[i * C + c] = run[c];
      run[c] += v;
    }
}

}  // namespace bds
