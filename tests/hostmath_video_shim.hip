// TEST-ONLY host shim of the video frames' pixel formulas (csrc/video_math.h, the functions the kernel of csrc/video.hip runs) on the CPU,
// so that tests/test_video_cpu.py can compare them with the numpy restatement and the reference's recorded results without a GPU.  Not
// part of libbds.so, never loaded by the product.
#include <stdint.h>

#include "../bilateral_driving_amd/csrc/video_math.h"

using namespace bds;

extern "C" void hm_vf_to8b(int64_t n, const float *x, uint8_t *out) {
  for (int64_t i = 0; i < n; i++) out[i] = vf_to8b(x[i]);
}

// depth, weight [n] -> index [n] (kVfBad = -1: black)
extern "C" void hm_vf_depth_index(int64_t n, const float *depth, const float *weight, int32_t *index) {
  for (int64_t i = 0; i < n; i++) index[i] = vf_depth_index(depth[i], weight[i]);
}

// index [n] -> rgb [n,3]
extern "C" void hm_vf_turbo(int64_t n, const int32_t *index, uint8_t *rgb) {
  for (int64_t i = 0; i < n; i++) {
    const uint32_t c = vf_turbo(index[i]);
    rgb[3 * i] = (uint8_t)c, rgb[3 * i + 1] = (uint8_t)(c >> 8), rgb[3 * i + 2] = (uint8_t)(c >> 16);
  }
}

// rgb [n,3], op [n] -> out [n,3], before the quantiser
extern "C" void hm_vf_over_green(int64_t n, const float *rgb, const float *op, float *out) {
  for (int64_t i = 0; i < n; i++)
    for (int ch = 0; ch < 3; ch++) out[3 * i + ch] = vf_over_green(rgb[3 * i + ch], op[i], ch);
}

extern "C" void hm_vf_lidar_shows_depth(int64_t n, const float *depth, uint8_t *out) {
  for (int64_t i = 0; i < n; i++) out[i] = vf_lidar_shows_depth(depth[i]) ? 1 : 0;
}

// {min(lo, hi), |hi - lo|, the green background's three channels}
extern "C" void hm_vf_constants(float *out) {
  out[0] = kVfCurveMin, out[1] = kVfCurveSpan, out[2] = kVfGreen[0], out[3] = kVfGreen[1], out[4] = kVfGreen[2];
}
