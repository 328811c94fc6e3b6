// TEST-ONLY host shim of the evaluation geometry metrics' per-element math (csrc/geometry_math.h, the functions the kernels of
// csrc/geometry.hip run) on the CPU, so that tests/test_geometry_cpu.py can compare the unprojection, the trim counts, the rank select
// and a whole frame with the float64 restatement without a GPU.  Not part of libbds.so, never loaded by the product.  The frame
// follows the kernels' stages (flags, ordered compaction, pair loop, select, row); its double sums run serially, where the kernels
// add per-lane partial sums in a fixed tree.
#include <stdint.h>

#include <vector>

#include "../bilateral_driving_amd/csrc/geometry_math.h"

using namespace bds;

extern "C" void hm_geo_unproject(int u, int v, float z, const float *K, const float *c2w, float *out) { geo_unproject(u, v, z, K, c2w, out); }
extern "C" long long hm_geo_trim_count(long long n, int which) { return geo_trim_count(n, which); }
extern "C" unsigned hm_geo_flags(float pred, float gt, int ego, int sky, int dynamic, int human, int vehicle) {
  return geo_flags(geo_valid(pred, gt, ego != 0), sky != 0, dynamic != 0, human != 0, vehicle != 0);
}
extern "C" float hm_geo_pair(int norm, const float *a, const float *b) {
  return norm == 1 ? geo_pair<1>(a[0], a[1], a[2], b[0], b[1], b[2]) : geo_pair<2>(a[0], a[1], a[2], b[0], b[1], b[2]);
}

// out = {sum, sum of squares, k, threshold} over the k smallest of n non-negative floats (k >= 1): four 8-bit radix steps, then the sums
extern "C" void hm_geo_select(const float *vals, long long n, long long k, double *out) {
  unsigned prefix = 0u, mask = 0u;
  unsigned long long rank = (unsigned long long)(k - 1);
  for (int shift = 24; shift >= 0; shift -= 8) {
    unsigned hist[256] = {0};
    for (long long i = 0; i < n; i++) {
      const unsigned b = geo_bits(vals[i]);
      if ((b & mask) == prefix) hist[(b >> shift) & 255u]++;
    }
    prefix |= geo_select_digit(hist, &rank) << shift;
    mask |= 255u << shift;
  }
  double s = 0.0, s2 = 0.0;
  unsigned long long c = 0;
  for (long long i = 0; i < n; i++) {
    if (geo_bits(vals[i]) < prefix) {
      s += (double)vals[i];
      s2 += (double)vals[i] * (double)vals[i];
      c++;
    }
  }
  const float t = geo_from_bits(prefix);
  geo_trimmed(s, s2, c, (unsigned long long)k, t, &out[0], &out[1]);
  out[2] = (double)k;
  out[3] = (double)t;
}

static void nearest(const std::vector<float> &q, const std::vector<float> &t, const std::vector<long long> &ids, std::vector<float> &best) {
  best.assign(ids.size(), INFINITY);
  for (size_t i = 0; i < ids.size(); i++)
    for (size_t j = 0; j < ids.size(); j++) {
      const float *a = &q[3 * ids[i]], *b = &t[3 * ids[j]];
      best[i] = fminf(best[i], geo_pair<2>(a[0], a[1], a[2], b[0], b[1], b[2]));
    }
}

// masks: one byte per pixel or NULL; row: 32 doubles in the layout of BDS_GEOMETRY_METRICS_ROW; dist_pred / dist_gt: [H*W]; returns n
extern "C" long long hm_geo_frame(int H, int W, const float *pred, const float *gt, const uint8_t *ego, const uint8_t *m0, const uint8_t *m1,
                                  const uint8_t *m2, const uint8_t *m3, const float *K, const float *c2w, double *row, float *dist_pred,
                                  float *dist_gt) {
  std::vector<float> P, G, err;
  std::vector<long long> all, cls[kGeoClasses];
  auto bit = [](const uint8_t *m, long long i) { return m != nullptr && m[i] != 0; };
  for (int v = 0; v < H; v++)
    for (int u = 0; u < W; u++) {
      const long long pix = (long long)v * W + u;
      const unsigned fl = geo_flags(geo_valid(pred[pix], gt[pix], bit(ego, pix)), bit(m0, pix), bit(m1, pix), bit(m2, pix), bit(m3, pix));
      if (!(fl & 1u)) continue;
      float p[3], g[3];
      geo_unproject(u, v, pred[pix], K, c2w, p);
      geo_unproject(u, v, gt[pix], K, c2w, g);
      const long long j = (long long)all.size();
      all.push_back(j);
      for (int k = 0; k < 3; k++) {
        P.push_back(p[k]);
        G.push_back(g[k]);
      }
      err.push_back(fabsf(pred[pix] - gt[pix]));
      for (int c = 0; c < kGeoClasses; c++)
        if ((fl >> (c + 1)) & 1u) cls[c].push_back(j);
    }
  const long long n = (long long)all.size();
  std::vector<float> dp, dg;
  nearest(P, G, all, dp);
  nearest(G, P, all, dg);
  for (long long i = 0; i < n; i++) {
    dist_pred[i] = dp[i];
    dist_gt[i] = dg[i];
  }
  const double nan = (double)NAN;
  const float *arrays[3] = {dp.data(), dg.data(), err.data()};
  for (int s = 0; s < 1 + kGeoTrims; s++) {
    const long long k = s == 0 ? n : geo_trim_count(n, s - 1);
    double m[3] = {nan, nan, nan}, sq = nan;
    for (int a = 0; a < 3 && k > 0; a++) {
      double o[4];
      if (s == 0) {      // every value lies below the threshold
        o[0] = o[1] = 0.0;
        for (long long i = 0; i < n; i++) {
          o[0] += (double)arrays[a][i];
          o[1] += (double)arrays[a][i] * (double)arrays[a][i];
        }
      } else {
        hm_geo_select(arrays[a], n, k, o);
      }
      m[a] = o[0] / (double)k;
      if (a == 2) sq = sqrt(o[1] / (double)k);
    }
    row[s] = m[0] + m[1];
    row[4 + s] = sq;
    row[20 + s] = m[0];
    row[24 + s] = m[1];
    row[28 + s] = m[2];
  }
  row[8] = nan;
  if (n > 0) {
    double o[4];
    hm_geo_select(err.data(), n, (n - 1) / 2 + 1, o);
    row[8] = o[3] * o[3];
  }
  row[14] = (double)n;
  for (int c = 0; c < kGeoClasses; c++) {
    std::vector<float> a, b;
    nearest(P, G, cls[c], a);
    nearest(G, P, cls[c], b);
    double sa = 0.0, sb = 0.0;
    for (size_t i = 0; i < a.size(); i++) {
      sa += (double)a[i];
      sb += (double)b[i];
    }
    const double m = (double)cls[c].size();
    row[9 + c] = m > 0.0 ? sa / m + sb / m : nan;
    row[15 + c] = m;
  }
  return n;
}
