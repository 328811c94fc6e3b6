// TEST-ONLY host shim of the pseudo-lidar generation's per-element math (csrc/pseudo_lidar_math.h, the functions the kernels of
// csrc/pseudo_lidar.hip run) on the CPU, so that tests/test_pseudo_lidar_cpu.py can compare the binning with its winner rule and the
// emission with the float64 restatement and the reference's recorded results without a GPU.  Not part of libbds.so, never loaded by
// the product.  The loops follow the kernels' passes; where the bin kernel takes an atomic max the shim takes the max in index order,
// which gives the same map.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/pseudo_lidar_math.h"

using namespace bds;

extern "C" int hm_pl_pixel(const float *cam, const double *beams, int H, int W, int mode, int u, int v, float d, float *p) {
  return pl_pixel_cell(cam, beams, H, W, mode, u, v, d, p);
}

extern "C" int hm_pl_point(const double *beams, int crop, int H, int W, int mode, const float *p) {
  return pl_point_cell(beams, crop, H, W, mode, p);
}

// the emit pass of one camera: the occupied cells of the kept rows in cell order
template <typename F>
static int emit(const int *winner, int H, int W, int slice, int *source, F &&write) {
  int at = 0;
  for (int cell = 0; cell < H * W; cell++) {
    if ((cell / W) % slice != 0 || winner[cell] < 0) continue;
    write(at, winner[cell]);
    if (source) source[at] = winner[cell];
    at++;
  }
  return at;
}

// bds_pseudo_lidar_from_depth (same arguments, host arrays)
extern "C" void hm_pl_from_depth(int C, int Hi, int Wi, const float *depth, const float *cams, const double *beams, int H, int W,
                                 int slice, int mode, int *winner, float *points, int *counts, int *source) {
  const int cap = ((H + slice - 1) / slice) * W, N = Hi * Wi;
  for (int c = 0; c < C; c++) {
    const float *cam = cams + c * kPlCamFloats, *dm = depth + (long long)c * N;
    int *win = winner + (long long)c * H * W;
    for (int k = 0; k < H * W; k++) win[k] = -1;
    for (int i = 0; i < N; i++) {
      float p[3];
      const int cell = pl_pixel_cell(cam, beams, H, W, mode, i % Wi, i / Wi, dm[i], p);
      if (cell >= 0 && win[cell] < i) win[cell] = i;
    }
    float *out = points + (long long)c * cap * 3;
    counts[c] = emit(win, H, W, slice, source ? source + (long long)c * cap : nullptr, [&](int at, int i) {
      float pc[3];
      pl_unproject(cam, i % Wi, i / Wi, dm[i], beams[kPlMaxDepth], pc);
      pl_to_lidar(cam, pc, out + 3 * at);
    });
  }
}

// bds_pseudo_lidar_from_points
extern "C" void hm_pl_from_points(long long N, const float *cloud, const double *beams, int crop, int H, int W, int slice, int mode,
                                  int *winner, float *points, int *counts, int *source) {
  for (int k = 0; k < H * W; k++) winner[k] = -1;
  for (long long i = 0; i < N; i++) {
    const int cell = pl_point_cell(beams, crop, H, W, mode, cloud + 4 * i);
    if (cell >= 0 && winner[cell] < (int)i) winner[cell] = (int)i;
  }
  counts[0] = emit(winner, H, W, slice, source, [&](int at, int i) {
    for (int k = 0; k < 4; k++) points[4 * at + k] = cloud[4 * (long long)i + k];
  });
}
