// Per-element math of the exact K-nearest self-search that initialises a scene's scales (models/gaussians/basics.py:208-224
// k_nearest_sklearn, called by vanilla.py:79-105 and nodes/rigid.py:113-120), used by csrc/knn.hip and by the host shim
// tests/hostmath_knn_shim.hip.
//   box        the grid's box is the cloud's box with at most N / 128 points trimmed beyond each face, found in two passes of a
//              1024-bin histogram per axis (the second over the first's result): a cloud with a heavy tail -- a street's lidar sweeps
//              plus sky points kilometres away -- would otherwise spend its cells on empty space.  Points beyond the box fall into
//              the border cells; exactness does not depend on the box (see `ring`)
//   grid       a uniform grid over that box: about one cell per point, never more than max(1, 2 N) cells, at least one cell
//              per axis (an axis of zero extent, or one thinner than the edge, gets one)
//   cell       clamp(floor((p - lo) * inv_edge), 0, dim - 1) per axis, x fastest in the linear id: a border cell also holds
//              whatever lies beyond it
//   pair       the squared distance from the coordinate DIFFERENCES, each product and each sum rounded on its own (no fused
//              multiply-add: (dx*dx + dy*dy) + dz*dz is what numpy and torch give for the same expression, bit for bit)
//   K best     K (d2, index) pairs in registers, ordered lexicographically; the index decides ties, so the list does not depend on
//              the order in which the candidates arrive
//   ring       after the cube of cells within Chebyshev radius r of the query's cell, the query is resolved when its K-th d2 is at
//              most the squared distance to the nearest face of the cube that is not a face of the grid, taken conservatively
//   scale      log(clamp(mean of the K distances, lo, hi))
#pragma once
#include "gs_math.h"

namespace bds {

constexpr int kKnnMaxK = 8;
constexpr int kKnnStatsWords = 32;      // include/bds.h BDS_KNN_STATS_WORDS
constexpr int kKnnBins = 1024;          // per axis, of the histograms that trim the box
constexpr int kKnnTrimShift = 7;        // at most N >> 7 points beyond each face of the box
// The margin of the termination test is shortened by a slack and by this factor before it is squared.  The slack, 2^-19 of the
// larger of the box's largest extent and the query's largest local coordinate, covers the roundings between a point and its cell:
// t = fl(fl(p - lo) * inv) with inv = fl(1 / edge) places a point whose cell is >= m at p - lo >= m * edge * (1 - 2^-22) and one whose
// cell is < m at p - lo < m * edge * (1 + 2^-22) (m * edge is at most the box's extent, wherever p lies); the query's local coordinate
// carries 2^-24 of itself, the face m * edge 2^-24 of the extent, their difference one more.  The factor covers the rounding of the
// pair distance itself (about 4 * 2^-24 relative) and of the square, so that every point outside the cube has a COMPUTED d2 strictly
// above a resolved query's K-th.  None of this assumes that the points lie inside the box.
constexpr float kKnnMarginScale = 0.9999f;
constexpr float kKnnSlackOfExtent = 1.0f / 524288.0f;

struct KnnGrid {
  float lo[3];
  float edge, inv, slack;
  int dim[3];
};

BDS_HD float knn_pair(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// the L1 twin of knn_pair for the cross search (csrc/knn_cross.hip, norm = 1): (|dx| + |dy|) + |dz|, each sum rounded on its own
BDS_HD float knn_pair_l1(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (fabsf(dx) + fabsf(dy)) + fabsf(dz);
}

// the cross search's blend epilogue: the inverse of the clamped distance of a neighbour at squared distance d2
BDS_HD float knn_blend_weight(float d2, float clamp_lo, float clamp_hi) { return 1.0f / fminf(fmaxf(sqrtf(d2), clamp_lo), clamp_hi); }

constexpr int kKnnEmptyRow = 0x7fffffff;      // the row knn_clear leaves in a slot no candidate has taken

BDS_HD bool knn_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

template <int K>
struct KnnBest {
  float d[K];
  int i[K];
};

template <int K>
BDS_HD void knn_clear(KnnBest<K> &b) {
#pragma unroll
  for (int s = 0; s < K; s++) {
    b.d[s] = INFINITY;
    b.i[s] = 0x7fffffff;
  }
}

// the list stays ascending: the newcomer replaces the last entry, then one pass of compare-exchanges carries it to its place
template <int K>
BDS_HD void knn_insert(KnnBest<K> &b, float d, int i) {
  if (!knn_less(d, i, b.d[K - 1], b.i[K - 1])) return;
  b.d[K - 1] = d;
  b.i[K - 1] = i;
#pragma unroll
  for (int s = K - 1; s > 0; s--) {
    const bool up = knn_less(b.d[s], b.i[s], b.d[s - 1], b.i[s - 1]);
    const float d0 = b.d[s - 1], d1 = b.d[s];
    const int i0 = b.i[s - 1], i1 = b.i[s];
    b.d[s - 1] = up ? d1 : d0;
    b.d[s] = up ? d0 : d1;
    b.i[s - 1] = up ? i1 : i0;
    b.i[s] = up ? i0 : i1;
  }
}

// knn_insert's result by shifting, for the long lists of the cross search: entry s takes entry s - 1 where the newcomer goes below
// that one, the newcomer itself where it goes below entry s only.  Walking down from the last entry, each step reads entry s - 1
// before anything has overwritten it, so the list is updated in place: two flags live at a time, no second copy of the list.
// knn_less without the short circuit: three compares and two mask operations, no branch per entry
BDS_HD bool knn_less_flat(float da, int ia, float db, int ib) { return (da < db) | ((da == db) & (ia < ib)); }

template <int K>
BDS_HD void knn_insert_shift(KnnBest<K> &b, float d, int i) {
  bool below = knn_less_flat(d, i, b.d[K - 1], b.i[K - 1]);
  if (!below) return;
#pragma unroll
  for (int s = K - 1; s > 0; s--) {
    const bool above = knn_less_flat(d, i, b.d[s - 1], b.i[s - 1]);
    b.d[s] = above ? b.d[s - 1] : (below ? d : b.d[s]);
    b.i[s] = above ? b.i[s - 1] : (below ? i : b.i[s]);
    below = above;
  }
  b.d[0] = below ? d : b.d[0];
  b.i[0] = below ? i : b.i[0];
}

BDS_HD int knn_cell_axis(float p, float lo, float inv, int dim) {
  const float t = floorf((p - lo) * inv);
  return (int)fminf(fmaxf(t, 0.0f), (float)(dim - 1));      // (a NaN, which the entry's callers exclude, would give cell 0)
}

BDS_HD void knn_cell(const KnnGrid &g, float x, float y, float z, int c[3]) {
  c[0] = knn_cell_axis(x, g.lo[0], g.inv, g.dim[0]);
  c[1] = knn_cell_axis(y, g.lo[1], g.inv, g.dim[1]);
  c[2] = knn_cell_axis(z, g.lo[2], g.inv, g.dim[2]);
}

// histogram bin of a coordinate over [lo, lo + kKnnBins / scale]; scale 0 (an axis without extent): bin 0
BDS_HD float knn_bin_scale(float lo, float hi) {
  const float ext = hi - lo;
  return (ext > 0.0f && ext < INFINITY) ? (float)kKnnBins / ext : 0.0f;
}
BDS_HD int knn_bin(float v, float lo, float scale) {
  const float t = floorf((v - lo) * scale);
  return (int)fminf(fmaxf(t, 0.0f), (float)(kKnnBins - 1));
}

// hist: one axis' kKnnBins counts over [lo, hi] (points beyond are counted in the end bins).  Whole bins are dropped from either end
// while the points in them stay within the budget of N >> kKnnTrimShift.
BDS_HD void knn_trim_axis(const unsigned *hist, long long N, float lo, float hi, float *lo_out, float *hi_out) {
  *lo_out = lo;
  *hi_out = hi;
  const float w = (hi - lo) / (float)kKnnBins;
  if (!(w > 0.0f) || !(w < INFINITY)) return;
  const unsigned long long budget = (unsigned long long)(N > 0 ? N : 0) >> kKnnTrimShift;
  unsigned long long cum = 0;
  int b0 = 0, b1 = kKnnBins - 1;
  while (b0 < kKnnBins - 1 && cum + hist[b0] <= budget) cum += hist[b0++];
  cum = 0;
  while (b1 > b0 && cum + hist[b1] <= budget) cum += hist[b1--];
  if (b0 > 0) *lo_out = fminf(lo + (float)b0 * w, hi);
  if (b1 < kKnnBins - 1) *hi_out = fmaxf(fminf(lo + (float)(b1 + 1) * w, hi), *lo_out);
}

BDS_HD long long knn_cell_id(const KnnGrid &g, const int c[3]) { return ((long long)c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0]; }

// The grid of a cloud of N points over the box [lo, hi].  Only axes at least one edge long are divided: the edge comes from their
// extents' product and N, an axis thinner than it is dropped and the edge taken again (at most three times).  Rounding the dimensions
// up can exceed the cap of max(1, 2 N) cells, so the edge then grows by a tenth at a time (the dimensions are at most twice
// extent / edge each, so nine steps suffice; the loop is bounded and ends in one cell).
BDS_HD void knn_choose_grid(const float lo[3], const float hi[3], long long N, KnnGrid *g) {
  float ext[3], maxext = 0.0f;
  bool on[3];
  for (int a = 0; a < 3; a++) {
    g->lo[a] = lo[a];
    g->dim[a] = 1;
    ext[a] = hi[a] - lo[a];
    on[a] = ext[a] > 0.0f;
    maxext = fmaxf(maxext, ext[a]);
  }
  g->edge = 1.0f;
  g->inv = 0.0f;
  g->slack = 0.0f;
  if (!(maxext > 0.0f) || !(maxext < INFINITY)) return;      // one point repeated, or an extent beyond float32: one cell
  const double cap = N > 0 ? 2.0 * (double)N : 1.0;
  double e = 0.0;
  for (int pass = 0; pass < 3; pass++) {
    double vol = 1.0;
    int d = 0;
    for (int a = 0; a < 3; a++)
      if (on[a]) {
        vol *= (double)ext[a];
        d++;
      }
    const double per = vol / (double)(N > 0 ? N : 1);
    e = d == 3 ? cbrt(per) : (d == 2 ? sqrt(per) : per);
    bool dropped = false;
    for (int a = 0; a < 3; a++)
      if (on[a] && (double)ext[a] < e) {
        on[a] = false;
        dropped = true;
      }
    if (!dropped) break;
  }
  if (!on[0] && !on[1] && !on[2]) return;      // (cannot happen: the longest axis is never thinner than the edge)
  for (int step = 0; step < 64; step++) {
    const float edge = (float)e;
    if (!(edge > 0.0f) || !(edge < INFINITY)) return;
    const float inv = 1.0f / edge;
    if (!(inv > 0.0f) || !(inv < INFINITY)) return;
    double cells = 1.0;
    int dim[3];
    bool fits = true;
    for (int a = 0; a < 3; a++) {
      const double n = on[a] ? floor((double)ext[a] / (double)edge) + 1.0 : 1.0;
      if (n > 1073741824.0) fits = false;
      dim[a] = fits ? (int)n : 1;
      cells *= n;
    }
    if (fits && cells <= cap) {
      g->edge = edge;
      g->inv = inv;
      g->slack = maxext * kKnnSlackOfExtent;
      for (int a = 0; a < 3; a++) g->dim[a] = dim[a];
      return;
    }
    e *= 1.1;
  }
}

// The squared radius around the query (local coordinates ql = q - lo, cell c) inside which every point lies in the cube of cells
// within Chebyshev radius r: +inf when the cube covers the grid, negative when the conservative margin is not positive (never
// resolved at this ring).  A face of the cube that is a face of the grid bounds nothing: the border cells hold what lies beyond.
BDS_HD float knn_ring_margin2(const KnnGrid &g, const float ql[3], const int c[3], int r) {
  float m = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int lo_c = c[a] - r, hi_c = c[a] + r;
    if (lo_c > 0) m = fminf(m, ql[a] - (float)lo_c * g.edge);
    if (hi_c < g.dim[a] - 1) m = fminf(m, (float)(hi_c + 1) * g.edge - ql[a]);
  }
  if (m == INFINITY) return INFINITY;
  const float far = fmaxf(fmaxf(fabsf(ql[0]), fabsf(ql[1])), fabsf(ql[2])) * kKnnSlackOfExtent;
  m = (m - fmaxf(g.slack, far)) * kKnnMarginScale;
  return m > 0.0f ? m * m : -1.0f;
}

BDS_HD bool knn_resolved(float kth_d2, float margin2) { return margin2 == INFINITY || kth_d2 <= margin2; }

// dist: K ascending distances (not squared)
template <int K>
BDS_HD float knn_log_scale(const float *dist, float clamp_lo, float clamp_hi) {
  float s = dist[0];
#pragma unroll
  for (int k = 1; k < K; k++) s += dist[k];
  const float mean = s / (float)K;
  return logf(fminf(fmaxf(mean, clamp_lo), clamp_hi));
}

// order-preserving map of a finite float onto uint32 (for integer atomic min / max) and back
BDS_HD unsigned knn_ordered(float v) {
  union { float f; unsigned u; } c;
  c.f = v;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
BDS_HD float knn_from_ordered(unsigned u) {
  union { float f; unsigned u; } c;
  c.u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return c.f;
}

}  // namespace bds
