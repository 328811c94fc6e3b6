// TEST-ONLY host shim of the K-nearest self-search's per-element math (csrc/knn_math.h, the functions the kernels of csrc/knn.hip
// run) on the CPU, so that tests/test_knn_cpu.py can compare the cell addressing, the ring walk with its termination test, the
// K-best insertion and the scale epilogue with the float64 restatement without a GPU.  Not part of libbds.so, never loaded by the
// product.  hm_knn_run follows the kernels' stages (bounds, the two trims of the box, grid, sort by cell, rings, brute force for the
// unresolved); inside a cell it visits the points in reverse row order, where the kernels' order is whatever the atomics gave: the
// (d2, index) order of the list makes the result the same.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../bilateral_driving_amd/csrc/knn_math.h"

using namespace bds;

extern "C" float hm_knn_pair(const float *a, const float *b) { return knn_pair(a[0], a[1], a[2], b[0], b[1], b[2]); }
extern "C" unsigned hm_knn_ordered(float v) { return knn_ordered(v); }
extern "C" float hm_knn_from_ordered(unsigned u) { return knn_from_ordered(u); }

// grid_out: {edge, inv, slack, lo x y z} (hm_knn_run adds the box's hi x y z); dims_out: 3 ints
extern "C" void hm_knn_grid(const float *lo, const float *hi, long long N, float *grid_out, int *dims_out) {
  KnnGrid g;
  knn_choose_grid(lo, hi, N, &g);
  grid_out[0] = g.edge;
  grid_out[1] = g.inv;
  grid_out[2] = g.slack;
  for (int a = 0; a < 3; a++) {
    grid_out[3 + a] = g.lo[a];
    dims_out[a] = g.dim[a];
  }
}

// feeds `n` candidates (d2[i], ids[i]) to a K-list in the given order; out_d / out_i receive the list
template <int K>
static void insert_all(const float *d2, const int *ids, int n, float *out_d, int *out_i) {
  KnnBest<K> b;
  knn_clear<K>(b);
  for (int i = 0; i < n; i++) knn_insert<K>(b, d2[i], ids[i]);
  for (int k = 0; k < K; k++) {
    out_d[k] = b.d[k];
    out_i[k] = b.i[k];
  }
}

template <int K>
static void run(long long N, const float *x, int ring_max, float *dist, int *idx, int *ring, int *cells, float *log_scales, float clamp_lo,
                float clamp_hi, float *grid_out, int *dims_out) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (long long i = 0; i < N; i++)
    for (int a = 0; a < 3; a++) {
      lo[a] = fminf(lo[a], x[3 * i + a]);
      hi[a] = fmaxf(hi[a], x[3 * i + a]);
    }
  for (int a = 0; a < 3; a++) {      // (through the encoding the bounds kernel's atomics use)
    lo[a] = knn_from_ordered(knn_ordered(lo[a]));
    hi[a] = knn_from_ordered(knn_ordered(hi[a]));
  }
  for (int pass = 0; pass < 2; pass++) {      // the two trimming passes: the box loses at most N / 128 points beyond each face
    std::vector<unsigned> hist(3 * kKnnBins, 0u);
    for (int a = 0; a < 3; a++) {
      const float scale = knn_bin_scale(lo[a], hi[a]);
      for (long long i = 0; i < N; i++) hist[a * kKnnBins + knn_bin(x[3 * i + a], lo[a], scale)]++;
    }
    for (int a = 0; a < 3; a++) knn_trim_axis(&hist[a * kKnnBins], N, lo[a], hi[a], &lo[a], &hi[a]);
  }
  KnnGrid g;
  knn_choose_grid(lo, hi, N, &g);
  hm_knn_grid(lo, hi, N, grid_out, dims_out);
  for (int a = 0; a < 3; a++) grid_out[6 + a] = hi[a];
  const long long ncell = (long long)g.dim[0] * g.dim[1] * g.dim[2];
  std::vector<long long> off(ncell + 1, 0), cell(N);
  for (long long i = 0; i < N; i++) {
    int c[3];
    knn_cell(g, x[3 * i], x[3 * i + 1], x[3 * i + 2], c);
    for (int a = 0; a < 3; a++) cells[3 * i + a] = c[a];
    cell[i] = knn_cell_id(g, c);
    off[cell[i] + 1]++;
  }
  for (long long c = 0; c < ncell; c++) off[c + 1] += off[c];
  std::vector<long long> order(N), fill(off.begin(), off.end() - 1);
  for (long long i = N - 1; i >= 0; i--) order[fill[cell[i]]++] = i;
  for (long long i = 0; i < N; i++) {
    const float qx = x[3 * i], qy = x[3 * i + 1], qz = x[3 * i + 2];
    const int *c = &cells[3 * i];
    const float ql[3] = {qx - g.lo[0], qy - g.lo[1], qz - g.lo[2]};
    KnnBest<K> b;
    knn_clear<K>(b);
    auto scan = [&](long long s, long long e) {
      for (long long t = s; t < e; t++) {
        const long long p = order[t];
        if (p != i) knn_insert<K>(b, knn_pair(qx, qy, qz, x[3 * p], x[3 * p + 1], x[3 * p + 2]), (int)p);
      }
    };
    int resolved = -1;
    for (int r = 0; r <= ring_max && resolved < 0; r++) {
      for (int z = std::max(c[2] - r, 0); z <= std::min(c[2] + r, g.dim[2] - 1); z++)
        for (int y = std::max(c[1] - r, 0); y <= std::min(c[1] + r, g.dim[1] - 1); y++) {
          const long long row = ((long long)z * g.dim[1] + y) * g.dim[0];
          const bool shell = std::abs(z - c[2]) == r || std::abs(y - c[1]) == r;
          if (shell) {
            scan(off[row + std::max(c[0] - r, 0)], off[row + std::min(c[0] + r, g.dim[0] - 1) + 1]);
          } else {
            if (c[0] - r >= 0) scan(off[row + c[0] - r], off[row + c[0] - r + 1]);
            if (c[0] + r <= g.dim[0] - 1) scan(off[row + c[0] + r], off[row + c[0] + r + 1]);
          }
        }
      if (knn_resolved(b.d[K - 1], knn_ring_margin2(g, ql, c, r))) resolved = r;
    }
    if (resolved < 0) {      // the fallback: every point
      knn_clear<K>(b);
      scan(0, N);
    }
    ring[i] = resolved;
    float d[K];
    for (int k = 0; k < K; k++) {
      d[k] = sqrtf(b.d[k]);
      dist[i * K + k] = d[k];
      idx[i * K + k] = b.i[k];
    }
    log_scales[i] = knn_log_scale<K>(d, clamp_lo, clamp_hi);
  }
}

#define HM_KNN_DISPATCH(FN, ...) \
  switch (K) {                   \
    case 1: FN<1>(__VA_ARGS__); break; \
    case 2: FN<2>(__VA_ARGS__); break; \
    case 3: FN<3>(__VA_ARGS__); break; \
    case 4: FN<4>(__VA_ARGS__); break; \
    case 5: FN<5>(__VA_ARGS__); break; \
    case 6: FN<6>(__VA_ARGS__); break; \
    case 7: FN<7>(__VA_ARGS__); break; \
    case 8: FN<8>(__VA_ARGS__); break; \
    default: return -1;          \
  }

extern "C" int hm_knn_insert_all(int K, const float *d2, const int *ids, int n, float *out_d, int *out_i) {
  HM_KNN_DISPATCH(insert_all, d2, ids, n, out_d, out_i)
  return 0;
}

// x [N,3]; dist, idx [N,K]; ring [N]: the ring that resolved the query, -1 = the brute-force fallback; cells [N,3]; log_scales [N]
extern "C" int hm_knn_run(long long N, const float *x, int K, int ring_max, float *dist, int *idx, int *ring, int *cells, float *log_scales,
                          float clamp_lo, float clamp_hi, float *grid_out, int *dims_out) {
  HM_KNN_DISPATCH(run, N, x, ring_max, dist, idx, ring, cells, log_scales, clamp_lo, clamp_hi, grid_out, dims_out)
  return 0;
}
