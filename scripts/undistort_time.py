#!/usr/bin/env python3
"""Times the undistortion of one camera's image stack at Waymo's load size (640 x 960, 198 frames, configs/datasets/waymo) in two
forms on the same GPU:

  (a) undistort   bilateral_driving_amd.undistort.undistort_images(stack, K, dist, out="unit") on a uint8 stack that is already on the
                  device: the per-frame table formed on the host and uploaded, the float32 result allocated, one launch of
                  ``bds_undistort`` with the ``/ 255`` fused.  ``entry`` is that launch alone into a preallocated result.
  (b) grid_sample the same map applied by ``torch.nn.functional.grid_sample(mode="bilinear", padding_mode="zeros",
                  align_corners=True)`` on float32.  ``grid_sample`` times the call alone: the float32 [F,3,H,W] input and the
                  [F,H,W,2] grid are made beforehand and not counted.  ``with_convert`` adds what a caller holding the uint8 stack
                  must also run: the conversion, the ``/ 255`` and the two permutes.

A and B alternate; each sample is one call between two device events after a warm-up; the medians are reported.  The two forms are
compared on their outputs first ((a) blends on the 1/32-pixel grid with 15-bit weights and rounds to 8 bits before the division, (b)
interpolates in float32: they differ by up to about one 8-bit level).

    python scripts/undistort_time.py [--out profiles/undistort_time.json] [--reps 15] [--frames 198]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/undistort_time.py --kernel-only 50"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import undistort      # noqa: E402

H, W = 640, 960
K = np.array([[1030.0, 0.0, 481.3], [0.0, 1030.0, 322.9], [0.0, 0.0, 1.0]])      # Waymo's front camera, scaled to the load size
DIST = np.array([0.045, -0.35, 0.0012, -0.0006, 0.0])
HBM_SPEC_TBS, HBM_STREAM_TBS = 8.0, 6.2


def source_grid(frames, dev):
    """[F,H,W,2] float32 for grid_sample from the float64 map of include/bds.h, formed with framework ops on the device."""
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2, k3 = DIST
    ir = np.linalg.inv(K).reshape(9)
    i, j = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    _x, _y, _w = j * ir[0] + i * ir[1] + ir[2], j * ir[3] + i * ir[4] + ir[5], j * ir[6] + i * ir[7] + ir[8]
    x, y = _x / _w, _y / _w
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    u = fx * (x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)) + u0
    v = fy * (y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)) + v0
    grid = torch.stack([2 * u / (W - 1) - 1, 2 * v / (H - 1) - 1], dim=-1).float()
    return grid[None].expand(frames, H, W, 2).contiguous()


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_time.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=198)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N", help="launch bds_undistort N times and exit: the program to run under a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("undistort_time.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    n = a.frames
    g = torch.Generator().manual_seed(0)
    stack = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    L, lib = undistort.L, undistort.L.lib()
    cams = torch.from_numpy(undistort.camera_table(K, DIST, None, n)).to(dev)
    result = torch.empty(n, H, W, 3, dtype=torch.float32, device=dev)

    def entry():
        L.check(lib.bds_undistort(n, H, W, 3, L.ptr(stack), L.ptr(cams), undistort.KINDS["unit"], L.ptr(result), L.stream()), "bds_undistort")
    if a.kernel_only:
        for _ in range(a.kernel_only):
            entry()
        torch.cuda.synchronize()
        return
    grid = source_grid(n, dev)
    as_float = (stack.float() / 255).permute(0, 3, 1, 2).contiguous()
    forms = {
        "a_undistort_images": lambda: undistort.undistort_images(stack, K, DIST, out="unit"),
        "a_entry_alone": entry,
        "b_grid_sample": lambda: F.grid_sample(as_float, grid, mode="bilinear", padding_mode="zeros", align_corners=True),
        "b_with_convert": lambda: F.grid_sample((stack.float() / 255).permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros",
                                                align_corners=True).permute(0, 2, 3, 1).contiguous(),
    }
    ours = forms["a_undistort_images"]()
    theirs = forms["b_with_convert"]()
    diff = (ours - theirs).abs()
    agreement = {"max_abs_difference_in_8bit_levels": float(diff.max()) * 255, "mean_abs_difference_in_8bit_levels": float(diff.mean()) * 255}
    del ours, theirs, diff
    for fn in forms.values():      # warm-up
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in forms}
    for _ in range(a.reps):      # the forms alternate
        for k, fn in forms.items():
            samples[k].append(event_ms(fn))
    moved = n * H * W * 3 * (1 + 4)      # each source byte once, each float32 written once
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "image": [H, W, 3], "reps": a.reps,
           "clock": "device events around one call, ms; the forms alternate; median of reps after one warm-up",
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()},
           "agreement_a_vs_b": agreement,
           "bytes_moved_algorithmic": moved,
           "entry_alone_TB_per_s": moved / (statistics.median(samples["a_entry_alone"]) * 1e-3) / 1e12,
           "hbm_TB_per_s": {"specified": HBM_SPEC_TBS, "streaming_stores_measured": HBM_STREAM_TBS}}
    res["entry_alone_share_of_streaming_rate"] = res["entry_alone_TB_per_s"] / HBM_STREAM_TBS
    res["speedup_entry_vs_grid_sample"] = res["ms"]["b_grid_sample"]["median"] / res["ms"]["a_entry_alone"]["median"]
    res["speedup_wrapper_vs_with_convert"] = res["ms"]["b_with_convert"]["median"] / res["ms"]["a_undistort_images"]["median"]
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
