// The finished uint8 frame of an evaluation video (save_concatenated_videos / save_seperate_videos, models/video_utils.py:703-857, with
// the dataset layouts, to8b and depth_visualizer of utils/visualization.py) in one launch: where the reference colours every depth map,
// tiles the cameras into a zeroed float32 canvas, concatenates the keys and quantises, all in numpy on host copies of the renders, the
// kernel writes the canvas [Hc,Wc,3] uint8 from the device tensors.  The per-pixel formulas live in video_math.h.
//   table   the frame is a list of panels: a kind, up to two sources, the first source row shown and a rectangle of the canvas.  The
//           table travels BY VALUE as a kernel argument (at most 64 panels, 3 KB): the pointers change every frame, so nothing is
//           uploaded or allocated and a captured stream outlives nothing.  The panel loop is wave-uniform: every field sits in SGPRs.
//   pixels  the canvas is a flat byte array from a 4-byte aligned base; a row is 3 Wc bytes, rarely a multiple of 4.  A lane takes
//           four consecutive flat pixels -- 12 bytes, three dword stores -- which may straddle a row end or a panel edge: each pixel
//           finds its panels on its own, walking the table in order, so where panels overlap the LATER one wins as the reference's
//           successive assignments do.  A pixel in no panel is 0 (the reference's canvas is zeroed): every byte is written, no memset
//           precedes the launch.  A quad that the launch's pixel range [first, end) cuts -- the Hc Wc % 4 tail, the edge of a band --
//           writes its own pixels byte by byte.
//   bands   more than 64 panels: one launch per band of rows that at most 64 panels touch (disjoint byte ranges).
// No atomics and no read-back: bit-identical run to run.
#include <algorithm>
#include <vector>

#include "bds_common.h"
#include "video_math.h"

namespace bds {

constexpr int kVfBlock = 256, kVfQuad = 4;

struct VfPanel {      // 48 bytes
  const void *src0, *src1;
  int32_t kind, flags, src_w, src_row0, dst_y, dst_x, dst_h, dst_w;
};
struct VfTable {
  int32_t n, pad;
  VfPanel p[BDS_VIDEO_MAX_PANELS];
};
static_assert(sizeof(VfTable) + 32 <= 4096, "the table and the other arguments fit the kernel argument segment");

__device__ __forceinline__ float vf_scalar(const void *src, bool bytes, int64_t i) {
  return bytes ? (float)static_cast<const uint8_t *>(src)[i] : static_cast<const float *>(src)[i];
}

// the colour (r | g << 8 | b << 16) of source pixel i = row * src_w + column of one panel; kind and flags are wave-uniform
__device__ __forceinline__ uint32_t vf_panel_pixel(const VfPanel &p, int64_t i) {
  const float *rgb = static_cast<const float *>(p.src0) + 3 * i;
  switch (p.kind) {
    case BDS_VIDEO_RGB:
      return vf_pack(vf_to8b(rgb[0]), vf_to8b(rgb[1]), vf_to8b(rgb[2]));
    case BDS_VIDEO_GRAY: {
      const uint32_t v = vf_to8b(vf_scalar(p.src0, (p.flags & BDS_VIDEO_SRC0_BYTES) != 0, i));
      return v * 0x010101u;
    }
    case BDS_VIDEO_DEPTH: {
      const float w = p.src1 != nullptr ? vf_scalar(p.src1, (p.flags & BDS_VIDEO_SRC1_BYTES) != 0, i) : 1.0f;
      return vf_turbo(vf_depth_index(static_cast<const float *>(p.src0)[i], w));
    }
    case BDS_VIDEO_OVER_GREEN: {
      const float op = static_cast<const float *>(p.src1)[i];
      return vf_pack(vf_to8b(vf_over_green(rgb[0], op, 0)), vf_to8b(vf_over_green(rgb[1], op, 1)), vf_to8b(vf_over_green(rgb[2], op, 2)));
    }
    default: {      // BDS_VIDEO_LIDAR_ON_IMAGE
      const float d = static_cast<const float *>(p.src1)[i];
      if (vf_lidar_shows_depth(d)) return vf_turbo(vf_depth_index(d, 1.0f));
      return vf_pack(vf_to8b(rgb[0]), vf_to8b(rgb[1]), vf_to8b(rgb[2]));
    }
  }
}

// grid: cdiv(cdiv(end, 4) - first / 4, 256) workgroups; pixels [first, end) of the flat canvas, 0 <= first < end <= Hc Wc < 2^31 / 3
__global__ __launch_bounds__(kVfBlock) void video_frame_kernel(const VfTable tab, int Wc, int first, int end, uint8_t *__restrict__ canvas) {
  const int64_t q = (int64_t)(first / kVfQuad) + (int64_t)blockIdx.x * kVfBlock + threadIdx.x;
  const int64_t px0 = q * kVfQuad;
  if (px0 >= end) return;
  int y[kVfQuad], x[kVfQuad];
  uint32_t c[kVfQuad] = {0u, 0u, 0u, 0u};
  y[0] = (int)px0 / Wc;      // (px0 < end < 2^31 / 3)
  x[0] = (int)px0 - y[0] * Wc;
#pragma unroll
  for (int k = 1; k < kVfQuad; k++) {
    const bool wrap = x[k - 1] + 1 == Wc;
    x[k] = wrap ? 0 : x[k - 1] + 1;
    y[k] = y[k - 1] + (wrap ? 1 : 0);
  }
  bool valid[kVfQuad];
#pragma unroll
  for (int k = 0; k < kVfQuad; k++) valid[k] = px0 + k >= first && px0 + k < end;

  for (int j = 0; j < tab.n; j++) {
    const VfPanel &p = tab.p[j];
#pragma unroll
    for (int k = 0; k < kVfQuad; k++) {
      const int ry = y[k] - p.dst_y, rx = x[k] - p.dst_x;
      if (valid[k] && ry >= 0 && ry < p.dst_h && rx >= 0 && rx < p.dst_w)
        c[k] = vf_panel_pixel(p, (int64_t)(ry + p.src_row0) * p.src_w + rx);
    }
  }

  if (valid[0] && valid[kVfQuad - 1]) {      // twelve bytes r g b r | g b r g | b r g b from a 4-byte boundary
    uint32_t *out = reinterpret_cast<uint32_t *>(canvas) + 3 * q;
    out[0] = c[0] | (c[1] << 24);
    out[1] = (c[1] >> 8) | (c[2] << 16);
    out[2] = (c[2] >> 16) | (c[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < kVfQuad; k++) {
      if (valid[k]) {
        uint8_t *out = canvas + 3 * (px0 + k);
        out[0] = (uint8_t)c[k], out[1] = (uint8_t)(c[k] >> 8), out[2] = (uint8_t)(c[k] >> 16);
      }
    }
  }
}

static bool vf_panel_ok(const bds_video_panel &p, int Hc, int Wc) {
  if (p.kind < BDS_VIDEO_RGB || p.kind > BDS_VIDEO_LIDAR_ON_IMAGE) return false;
  const bool gray = p.kind == BDS_VIDEO_GRAY, depth = p.kind == BDS_VIDEO_DEPTH;
  const int allowed = gray ? BDS_VIDEO_SRC0_BYTES : (depth ? BDS_VIDEO_SRC1_BYTES : 0);
  if ((p.flags & ~allowed) != 0 || p.reserved != 0) return false;
  if (p.src0 == nullptr || (p.src1 == nullptr && (p.kind == BDS_VIDEO_OVER_GREEN || p.kind == BDS_VIDEO_LIDAR_ON_IMAGE))) return false;
  if (gray && p.src1 != nullptr) return false;
  if (!(p.flags & BDS_VIDEO_SRC0_BYTES) && (reinterpret_cast<uintptr_t>(p.src0) & 3u) != 0) return false;
  if (!(p.flags & BDS_VIDEO_SRC1_BYTES) && (reinterpret_cast<uintptr_t>(p.src1) & 3u) != 0) return false;
  if (p.src_h < 0 || p.src_w < 0 || (int64_t)p.src_h * p.src_w * 3 > INT32_MAX) return false;
  if (p.dst_y < 0 || p.dst_x < 0 || p.dst_h < 0 || p.dst_w < 0 || p.src_row0 < 0) return false;
  if ((int64_t)p.dst_y + p.dst_h > Hc || (int64_t)p.dst_x + p.dst_w > Wc) return false;
  return (int64_t)p.src_row0 + p.dst_h <= p.src_h && p.dst_w <= p.src_w;
}

}  // namespace bds

using namespace bds;

extern "C" int bds_video_frame(int n_panels, const bds_video_panel *panels, int Hc, int Wc, uint8_t *canvas, bds_stream_t stream) {
  BDS_REQUIRE(n_panels >= 0 && Hc >= 0 && Wc >= 0 && (int64_t)Hc * Wc * 3 <= INT32_MAX);
  BDS_REQUIRE(n_panels == 0 || panels != nullptr);
  for (int j = 0; j < n_panels; j++) BDS_REQUIRE(vf_panel_ok(panels[j], Hc, Wc));
  if (Hc == 0 || Wc == 0) return BDS_OK;
  BDS_REQUIRE(canvas != nullptr && (reinterpret_cast<uintptr_t>(canvas) & 3u) == 0);

  // the rows at which the set of panels changes; between two neighbours it is constant
  std::vector<int> shown, edges = {0, Hc};
  for (int j = 0; j < n_panels; j++) {
    if (panels[j].dst_h == 0 || panels[j].dst_w == 0) continue;
    shown.push_back(j);
    edges.push_back(panels[j].dst_y);
    edges.push_back(panels[j].dst_y + panels[j].dst_h);
  }
  std::sort(edges.begin(), edges.end());
  edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
  auto touching = [&](int r0, int r1) {
    int n = 0;
    for (int j : shown) n += panels[j].dst_y < r1 && panels[j].dst_y + panels[j].dst_h > r0;
    return n;
  };
  // bands: as many neighbouring intervals as share at most BDS_VIDEO_MAX_PANELS panels
  std::vector<int> cuts = {0};
  for (size_t e = 1; e < edges.size(); e++) {
    if (touching(edges[e - 1], edges[e]) > BDS_VIDEO_MAX_PANELS) return BDS_ECAPACITY;
    if (touching(cuts.back(), edges[e]) > BDS_VIDEO_MAX_PANELS) cuts.push_back(edges[e - 1]);
  }
  cuts.push_back(Hc);

  hipStream_t st = as_stream(stream);
  for (size_t b = 0; b + 1 < cuts.size(); b++) {
    const int r0 = cuts[b], r1 = cuts[b + 1];
    if (r0 == r1) continue;
    VfTable tab;
    tab.n = 0, tab.pad = 0;
    for (int j : shown) {
      const bds_video_panel &p = panels[j];
      if (!(p.dst_y < r1 && p.dst_y + p.dst_h > r0)) continue;
      tab.p[tab.n++] = VfPanel{p.src0, p.src1, p.kind, p.flags, p.src_w, p.src_row0, p.dst_y, p.dst_x, p.dst_h, p.dst_w};
    }
    const int first = r0 * Wc, end = r1 * Wc;
    const int64_t quads = cdiv(end, kVfQuad) - first / kVfQuad;
    hipLaunchKernelGGL(video_frame_kernel, dim3((unsigned)cdiv(quads, kVfBlock)), dim3(kVfBlock), 0, st, tab, Wc, first, end, canvas);
    BDS_LAUNCH_CHECK();
  }
  return BDS_OK;
}
