// TEST-ONLY host shim of the lens undistortion (csrc/undistort_math.h, the functions the kernel of csrc/undistort.hip runs) on the
// CPU, so that tests/test_undistort_cpu.py can compare the map, the taps and whole frames with the numpy restatement
// (tests/undistort_ref64.py) and with known answers without a GPU.  Not part of libbds.so, never loaded by the product.  The loop
// of hm_ud_frames follows the kernel: one pixel at a time, the map once for all channels.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/undistort_math.h"
#include "../include/bds.h"

using namespace bds;

// the map of one frame: u, v [H,W]
extern "C" void hm_ud_map(const double *cam, int H, int W, double *u, double *v) {
  for (int i = 0; i < H; i++)
    for (int j = 0; j < W; j++) ud_map(cam, i, j, u + (long long)i * W + j, v + (long long)i * W + j);
}

// n positions -> taps [n,6]: sx, sy, w00, w01, w10, w11
extern "C" void hm_ud_taps(long long n, const double *u, const double *v, int32_t *taps) {
  for (long long k = 0; k < n; k++) {
    const UdTaps t = ud_taps(u[k], v[k]);
    int32_t *o = taps + 6 * k;
    o[0] = t.sx, o[1] = t.sy, o[2] = t.w00, o[3] = t.w01, o[4] = t.w10, o[5] = t.w11;
  }
}

template <int C>
static void frames(int F, int H, int W, const uint8_t *src, const double *cams, int kind, void *out) {
  for (long long f = 0; f < F; f++)
    for (int i = 0; i < H; i++)
      for (int j = 0; j < W; j++) {
        double u, v;
        ud_map(cams + kUdCamDoubles * f, i, j, &u, &v);
        const UdTaps t = ud_taps(u, v);
        const bool outside = ud_outside(t, H, W);
        const long long o = ((f * H + i) * W + j) * C;
        int32_t value[C] = {};
        if (!outside) ud_sample<C>(t, src + f * H * W * C, H, W, value);
        for (int ch = 0; ch < C; ch++) {
          if (kind == BDS_UNDISTORT_UINT8)
            static_cast<uint8_t *>(out)[o + ch] = (uint8_t)value[ch];
          else
            static_cast<float *>(out)[o + ch] = kind == BDS_UNDISTORT_UNIT ? ud_unit(value[ch]) : ud_mask(value[ch]);
        }
      }
}

// ud_unit of the values 0..255
extern "C" void hm_ud_unit_table(float *out) {
  for (int v = 0; v < 256; v++) out[v] = ud_unit(v);
}

// bds_undistort on host arrays
extern "C" void hm_ud_frames(int F, int H, int W, int C, const uint8_t *src, const double *cams, int kind, void *out) {
  if (C == 3)
    frames<3>(F, H, W, src, cams, kind, out);
  else
    frames<1>(F, H, W, src, cams, kind, out);
}
