// Segment lookup of the scene view (csrc/scene_view.hip): the rows of several Gaussian classes lie one behind the other in ONE global
// row range (models/trainers/base.py:355-366 concatenates the classes per key), and a list-driven kernel has to find, for a global
// row id, the class it belongs to.  __host__ __device__ so that tests/ can run the exact device formula on the host through a
// hipcc-built shim (tests/hostmath_scene_shim.hip); the product only calls it from kernels and from the host entries' set-up.
#pragma once
#include <stdint.h>

#include "gs_math.h"

namespace bds {

constexpr int kSceneMaxSegments = 8;

// start[i] = first global row of segment i (start[0] = 0, ascending); entries at and beyond the number of segments hold INT32_MAX,
// which no row id reaches (ids are int32 and smaller than the row total, itself at most INT32_MAX).
struct SceneStarts {
  int32_t start[kSceneMaxSegments];
};

// Segment of global row g: the number of starts (beyond the first) that g has reached -- seven compares and adds, no branch, no
// table walk.  Total: every int32 g gets an answer in [0, kSceneMaxSegments).  A zero-row segment is never the answer for a row in
// [0, total): its start equals the next segment's, so whoever reaches it reaches that one too (and a trailing one starts at the
// total, which no row reaches).  g < 0 gives 0; the caller bounds the LOCAL row (g - start) by the segment's row count.
BDS_HD int scene_segment(const SceneStarts &t, int32_t g) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < kSceneMaxSegments; i++) s += g >= t.start[i] ? 1 : 0;
  return s;
}

// Host side: the starts of n_seg segments of rows[i] rows each.  False when the shape is not one the lookup serves (more than
// kSceneMaxSegments segments, a negative count, a total beyond int32).  total (optional) receives the row total.
static inline bool scene_starts_fill(int n_seg, const int64_t *rows, SceneStarts &t, int64_t *total) {
  if (n_seg < 1 || n_seg > kSceneMaxSegments || rows == nullptr) return false;
  int64_t at = 0;
  for (int i = 0; i < kSceneMaxSegments; i++) {
    if (i < n_seg) {
      if (rows[i] < 0) return false;
      t.start[i] = (int32_t)at;
      at += rows[i];
      if (at > (int64_t)INT32_MAX) return false;
    } else {
      t.start[i] = INT32_MAX;
    }
  }
  if (total) *total = at;
  return true;
}

}  // namespace bds
