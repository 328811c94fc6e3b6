#!/usr/bin/env python3
"""Time the initial scales of a scene (bilateral_driving_amd/init.py init_scales: the exact 3-nearest self-search with its fused
epilogue) on (a) the bench's lidar-initialised street scene (harness.lidar_scene: road, facades and clutter in a 120 m corridor plus a
tenth of the points at up to 2 km) and (b) a uniform cloud of 2 M points in a 100 m cube.  Warm-up calls, then the median of repeated
timed calls (HIP events around one call, a synchronise behind each).  Also reads the search's stats (grid, unresolved queries).
importable, the reference's own search (models/gaussians/basics.py:208-224: NearestNeighbors(k + 1, "auto", "euclidean") on the host,
the copy to the host included) is timed once on the same clouds and the distances are compared.

    python scripts/knn_init_time.py --out profiles/knn_init_time.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import harness, init  # noqa: E402


def clouds(lidar_points, uniform_points):
    for n in lidar_points:
        yield f"lidar_scene_{n}", harness.lidar_scene(n, seed=0, device="cpu")["means"].float().contiguous()
    for n in uniform_points:
        yield f"uniform_{n}", torch.rand(n, 3, generator=torch.Generator().manual_seed(0)) * 100.0


def timed(fn, warmup, repeats):
    ms = []
    for i in range(warmup + repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(e))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def sklearn_search(x_dev, k):
    from sklearn.neighbors import NearestNeighbors
    t0 = time.perf_counter()
    x = x_dev.cpu().numpy()
    distances, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
    out = distances[:, 1:].astype(np.float32)
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lidar-points", type=int, nargs="*", default=[1_000_000, 2_000_000])
    ap.add_argument("--uniform-points", type=int, nargs="*", default=[2_000_000])
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_init_time.py measures on the GPU; none found")
    try:
        import sklearn
        have_sklearn = not a.no_sklearn
    except ImportError:
        have_sklearn = False
    res = {"device": torch.cuda.get_device_name(0), "k": 3, "warmup": a.warmup, "repeats": a.repeats,
           "sklearn": sklearn.__version__ if have_sklearn else None, "clouds": []}
    for name, x in clouds(a.lidar_points, a.uniform_points):
        x = x.cuda()
        N = x.shape[0]
        dist, stats = init.k_nearest(x, 3, return_indices=False, return_stats=True)
        row = {"cloud": name, "points": N, "cell_edge": stats["cell_edge"], "dims": stats["dims"], "cells": stats["cells"],
               "grid_box": [stats["lo"], stats["hi"]], "cloud_box": [stats["cloud_lo"], stats["cloud_hi"]],
               "unresolved": stats["unresolved"], "unresolved_share": stats["unresolved"] / N,
               "fallback_pairs": float(stats["unresolved"]) * N,
               "init_scales_ms": timed(lambda: init.init_scales(x, 3, 3), a.warmup, a.repeats),
               "k_nearest_ms": timed(lambda: init.k_nearest(x, 3), a.warmup, a.repeats)}
        if have_sklearn:
            want, ms = sklearn_search(x, 3)
            got = dist.cpu().numpy()
            nz = want > 0
            row.update({"sklearn_ms": ms, "sklearn_over_init_scales": ms / row["init_scales_ms"]["median"],
                        "worst_relative_difference_from_sklearn": float(np.max(np.abs(got[nz] - want[nz]) / want[nz])),
                        "zeros_agree": bool(np.all(got[~nz] == 0))})
        res["clouds"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
