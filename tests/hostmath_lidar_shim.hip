// TEST-ONLY host shim of the lidar scene preparation's per-element math (csrc/lidar_math.h, the functions the kernels of
// csrc/lidar.hip run) on the CPU, so that tests/test_lidar_cpu.py can compare the projection with its winner rule, the visibility, the
// box test and the downsampler with the float64 restatement and the reference's recorded results without a GPU.  Not part of
// libbds.so, never loaded by the product.  The loops follow the kernels' passes; where the kernels take an atomic max the shim takes
// the max in row order, which gives the same map.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/lidar_math.h"

using namespace bds;

extern "C" int hm_lidar_project(const float *M, const float *p, int W, int H, int *px, int *py, float *depth) {
  return lidar_project(M, p[0], p[1], p[2], W, H, px, py, depth) ? 1 : 0;
}

// the three passes of bds_lidar_project (same arguments, host arrays)
extern "C" void hm_lidar_views(int V, int W, int H, long long N, const float *points, const float *mats, const long long *ranges,
                               const float *images, int *winner, float *depth, int *pix, unsigned char *visible, float *colors) {
  for (long long p = 0; p < (long long)V * H * W; p++) winner[p] = -1;
  for (long long i = 0; i < N; i++) {
    int last = -1;
    for (int v = 0; v < V; v++) {
      long long b = ranges[2 * v], e = ranges[2 * v + 1];
      b = b < 0 ? 0 : (b > N ? N : b);
      e = e < 0 ? 0 : (e > N ? N : e);
      if (i < b || i >= e) continue;
      int px, py;
      float d;
      if (!lidar_project(mats + 12 * v, points[3 * i], points[3 * i + 1], points[3 * i + 2], W, H, &px, &py, &d)) continue;
      const int q = (v * H + py) * W + px;
      if (winner[q] < (int)i) winner[q] = (int)i;
      last = q;
    }
    pix[i] = last;
    if (last >= 0) {
      visible[i] = 1;
      if (images && colors)
        for (int c = 0; c < 3; c++) colors[3 * i + c] = images[3 * (long long)last + c];
    }
  }
  for (long long p = 0; p < (long long)V * H * W; p++) {
    const int w = winner[p];
    const int v = (int)(p / ((long long)H * W));
    depth[p] = w >= 0 ? lidar_row(mats + 12 * v + 8, points[3 * (long long)w], points[3 * (long long)w + 1], points[3 * (long long)w + 2]) : 0.0f;
  }
}

extern "C" void hm_lidar_visible(long long N, const float *points, int V, const float *mats, const int *sizes, unsigned char *visible) {
  for (long long i = 0; i < N; i++) {
    bool seen = false;
    for (int v = 0; v < V && !seen; v++) {
      int px, py;
      float d;
      seen = lidar_project(mats + 12 * v, points[3 * i], points[3 * i + 1], points[3 * i + 2], sizes[2 * v], sizes[2 * v + 1], &px, &py, &d);
    }
    visible[i] = seen ? 1 : 0;
  }
}

// mask form and emit form at once: inside [N]; records in (row, box) order, at most `capacity` written; returns their number
extern "C" long long hm_lidar_boxes(long long N, const float *points, int B, const float *w2o, const float *half, const long long *ranges,
                                    const int *ids, unsigned char *inside, long long capacity, int *rec_ids, float *rec_xyz) {
  long long at = 0;
  for (long long i = 0; i < N; i++) {
    inside[i] = 0;
    for (int b = 0; b < B; b++) {
      if (ranges && (i < ranges[2 * b] || i >= ranges[2 * b + 1])) continue;
      float o[3];
      if (!lidar_in_box(w2o + 12 * b, half + 3 * b, points[3 * i], points[3 * i + 1], points[3 * i + 2], o)) continue;
      inside[i] = 1;
      if (at < capacity) {
        rec_ids[3 * at] = ids[2 * b];
        rec_ids[3 * at + 1] = ids[2 * b + 1];
        rec_ids[3 * at + 2] = (int)i;
        for (int c = 0; c < 3; c++) rec_xyz[3 * at + c] = o[c];
      }
      at++;
    }
  }
  return at;
}

extern "C" void hm_lidar_window(int i, int in, int out, int *start, int *end) {
  *start = lidar_window_start(i, in, out);
  *end = lidar_window_end(i, in, out);
}

extern "C" void hm_lidar_downsample(int H, int W, int Ho, int Wo, const float *in, float *out) {
  for (int i = 0; i < Ho; i++)
    for (int j = 0; j < Wo; j++) out[i * Wo + j] = lidar_downsample_cell(in, H, W, Ho, Wo, i, j);
}
