// Lens undistortion of a camera's frame stack on the device (include/bds.h: bds_undistort): what CameraData.load_images,
// load_egocar_mask, load_dynamic_masks and load_sky_masks (datasets/base/pixel_source.py:235-375) do frame by frame on the host with
// cv2.undistort, with the ``/ 255`` of the image stack or the ``> 0`` of the masks fused into the store.
//
// One thread per output pixel: the map is computed once in double (csrc/undistort_math.h, about 30 FP64 operations, and two
// divisions only where the new matrix is not affine) and serves all channels.  A workgroup is 64 x 4 pixels, one wave per row segment,
// so a wave's 2 x 65 taps fall into two (under distortion a few more) source rows and the four waves share the rows between them
// through L1; blockIdx.z is the frame: its 18 doubles are wave-uniform loads.  No LDS, no atomics: bit-identical run to run.  The byte
// roof is each source byte once from HBM plus the bytes written; measured, a 198 x 640 x 960 x 3 stack to float32 runs at 30 % of it
// (the twelve one-byte gathers per pixel, not the arithmetic or the stores, set the time).  Frames, and an
// output pixel's position, are indexed in 64 bits; a byte's offset inside its frame fits 32.
#include "bds_common.h"
#include "undistort_math.h"

namespace bds {

constexpr int kUdBlockW = 64, kUdBlockH = 4;
constexpr int kUdMaxGridZ = 65535;

template <int C>
struct __attribute__((packed, aligned(4))) UdPixel {
  float v[C];
};

template <int C, int KIND>
__global__ __launch_bounds__(kUdBlockW *kUdBlockH) void undistort_kernel(int H, int W, const uint8_t *__restrict__ src,
                                                                         const double *__restrict__ cams, void *__restrict__ out) {
  const int j = blockIdx.x * kUdBlockW + threadIdx.x, i = blockIdx.y * kUdBlockH + threadIdx.y;
  if (j >= W || i >= H) return;
  const int64_t f = blockIdx.z;
  const uint8_t *frame = src + f * H * W * C;
  double u, v;
  ud_map(cams + kUdCamDoubles * f, i, j, &u, &v);
  const UdTaps t = ud_taps(u, v);
  const bool outside = ud_outside(t, H, W);
  const int64_t o = ((f * H + i) * W + j) * C;
  int32_t value[C] = {};
  if (!outside) ud_sample<C>(t, frame, H, W, value);
  if (KIND == BDS_UNDISTORT_UINT8) {
#pragma unroll
    for (int ch = 0; ch < C; ch++) static_cast<uint8_t *>(out)[o + ch] = (uint8_t)value[ch];
  } else {
    // a pixel's floats leave in one store: a wave writes 64 C consecutive dwords
    UdPixel<C> px;
#pragma unroll
    for (int ch = 0; ch < C; ch++) px.v[ch] = KIND == BDS_UNDISTORT_UNIT ? ud_unit(value[ch]) : ud_mask(value[ch]);
    *reinterpret_cast<UdPixel<C> *>(static_cast<float *>(out) + o) = px;
  }
}

template <int C, int KIND>
static void undistort_launch(int F, int H, int W, const uint8_t *src, const double *cams, void *out, hipStream_t stream) {
  const dim3 grid((unsigned)cdiv(W, kUdBlockW), (unsigned)cdiv(H, kUdBlockH), (unsigned)F);
  hipLaunchKernelGGL((undistort_kernel<C, KIND>), grid, dim3(kUdBlockW, kUdBlockH), 0, stream, H, W, src, cams, out);
}

}  // namespace bds

using namespace bds;

extern "C" int bds_undistort(int F, int H, int W, int C, const uint8_t *src, const double *cams, int out_kind, void *out,
                             bds_stream_t stream) {
  BDS_REQUIRE(src != nullptr && cams != nullptr && out != nullptr);
  BDS_REQUIRE(F >= 1 && H >= 1 && W >= 1 && H <= kUdMaxExtent && W <= kUdMaxExtent);
  BDS_REQUIRE(C == 1 || C == 3);
  BDS_REQUIRE(out_kind == BDS_UNDISTORT_UINT8 || out_kind == BDS_UNDISTORT_UNIT || out_kind == BDS_UNDISTORT_MASK);
  BDS_REQUIRE((reinterpret_cast<uintptr_t>(cams) & 7u) == 0);
  const size_t out_item = out_kind == BDS_UNDISTORT_UINT8 ? 1 : 4;
  BDS_REQUIRE((reinterpret_cast<uintptr_t>(out) & (out_item - 1)) == 0);
  const int64_t frame = (int64_t)H * W * C;
  for (int f0 = 0; f0 < F; f0 += kUdMaxGridZ) {      // (frames are the grid's third dimension)
    const int n = F - f0 < kUdMaxGridZ ? F - f0 : kUdMaxGridZ;
    const uint8_t *s = src + f0 * frame;
    const double *c = cams + (int64_t)f0 * kUdCamDoubles;
    void *o = static_cast<uint8_t *>(out) + f0 * frame * (int64_t)out_item;
    const hipStream_t st = as_stream(stream);
    if (C == 3) {
      if (out_kind == BDS_UNDISTORT_UINT8) undistort_launch<3, BDS_UNDISTORT_UINT8>(n, H, W, s, c, o, st);
      else if (out_kind == BDS_UNDISTORT_UNIT) undistort_launch<3, BDS_UNDISTORT_UNIT>(n, H, W, s, c, o, st);
      else undistort_launch<3, BDS_UNDISTORT_MASK>(n, H, W, s, c, o, st);
    } else {
      if (out_kind == BDS_UNDISTORT_UINT8) undistort_launch<1, BDS_UNDISTORT_UINT8>(n, H, W, s, c, o, st);
      else if (out_kind == BDS_UNDISTORT_UNIT) undistort_launch<1, BDS_UNDISTORT_UNIT>(n, H, W, s, c, o, st);
      else undistort_launch<1, BDS_UNDISTORT_MASK>(n, H, W, s, c, o, st);
    }
    BDS_LAUNCH_CHECK();
  }
  return BDS_OK;
}
