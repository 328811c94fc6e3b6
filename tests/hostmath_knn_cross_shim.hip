// TEST-ONLY host shim of the batched cross search's per-element math (csrc/knn_math.h: knn_pair, knn_pair_l1, knn_insert_shift on
// KnnBest<Kc>, knn_blend_weight -- the functions the kernel of csrc/knn_cross.hip runs) on the CPU, so that
// tests/test_knn_points_cpu.py can compare them with the numpy restatement without a GPU.  Not part of libbds.so, never loaded by
// the product.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/knn_math.h"

using namespace bds;

extern "C" float hm_knn_cross_pair(int norm, const float *a, const float *b) {
  return norm == 2 ? knn_pair(a[0], a[1], a[2], b[0], b[1], b[2]) : knn_pair_l1(a[0], a[1], a[2], b[0], b[1], b[2]);
}

extern "C" float hm_knn_cross_weight(float d2, float lo, float hi) { return knn_blend_weight(d2, lo, hi); }

// One query q against the rows order[0..n) of the cloud p2 [.,3], visited in that order: the list of capacity Kc as the kernel keeps
// it (shift = 1) or as knn_insert would (shift = 0); out_d / out_i receive all Kc entries (an empty slot: +inf, 0x7fffffff).
template <int Kc>
static void query(int norm, int shift, const float *q, const float *p2, const int *order, int n, float *out_d, int *out_i) {
  KnnBest<Kc> b;
  knn_clear<Kc>(b);
  for (int t = 0; t < n; t++) {
    const int r = order[t];
    const float d = hm_knn_cross_pair(norm, q, p2 + 3 * r);
    if (shift)
      knn_insert_shift<Kc>(b, d, r);
    else
      knn_insert<Kc>(b, d, r);
  }
  for (int k = 0; k < Kc; k++) {
    out_d[k] = b.d[k];
    out_i[k] = b.i[k];
  }
}

extern "C" int hm_knn_cross_query(int Kc, int norm, int shift, const float *q, const float *p2, const int *order, int n, float *out_d,
                                  int *out_i) {
  switch (Kc) {
    case 4: query<4>(norm, shift, q, p2, order, n, out_d, out_i); return 0;
    case 8: query<8>(norm, shift, q, p2, order, n, out_d, out_i); return 0;
    case 16: query<16>(norm, shift, q, p2, order, n, out_d, out_i); return 0;
    case 32: query<32>(norm, shift, q, p2, order, n, out_d, out_i); return 0;
    default: return -1;
  }
}
