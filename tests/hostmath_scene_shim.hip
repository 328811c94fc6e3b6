// TEST-ONLY host shim of the scene view's segment lookup (csrc/scene_math.h: the compare chain the kernels of csrc/scene_view.hip run
// per list rank, and the host set-up of its starts) on the CPU, so that tests/test_lazy_scene_cpu.py can compare it with
// numpy.searchsorted without a GPU.  Not part of libbds.so, never loaded by the product.
#include "../bilateral_driving_amd/csrc/scene_math.h"

using namespace bds;

// starts_out [8] receives the table; seg_out [n_ids] the segment of every id.  Returns 0, or -1 when the set-up refuses the shape.
extern "C" int hm_scene_segments(int n_seg, const int64_t *rows, int64_t n_ids, const int32_t *ids, int32_t *starts_out, int32_t *seg_out,
                                 int64_t *total_out) {
  SceneStarts t;
  if (!scene_starts_fill(n_seg, rows, t, total_out)) return -1;
  for (int i = 0; i < kSceneMaxSegments; i++) starts_out[i] = t.start[i];
  for (int64_t i = 0; i < n_ids; i++) seg_out[i] = scene_segment(t, ids[i]);
  return 0;
}
