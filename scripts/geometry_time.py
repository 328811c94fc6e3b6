#!/usr/bin/env python3
"""Time the geometry scoring of one 1920x1280 evaluation frame (bilateral_driving_amd/geometry.py) at about 4e4 and about 1.5e5 valid
lidar points, in two forms: (a) the fused op (geometry_metrics: six launches, no host wait); (b) the same expression as framework ops
on the same GPU in the same process -- boolean indexing for the clouds, chunked ``torch.cdist(...).min`` both ways, ``torch.sort`` for
the trims, the five class subsets likewise.  cdist runs with compute_mode="donot_use_mm_for_euclid_dist": its default form expands
|x|^2 + |y|^2 - 2 x.y on the matrix cores and was measured 0.09 m^2 off at coordinates of 300 m, which is the size of the metric itself.
Its chunks are kept below 2^23 distances per call: above about 2^24 the difference form returned wrong minima on the ROCm build this
was measured with (0.05 - 0.6 m^2 off at 1e4 - 3e4 targets with 2048-row chunks, exact with 256-row chunks).  Warm-up, then the
median of repeated timed calls (HIP events), a and b alternating.  Prints the pair rate of the fused op (whole-frame and class pairs,
both directions), and that rate x 8 flop as a share of the 157 TF FP32 vector peak.

    python scripts/geometry_time.py --out profiles/geometry_time.json"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import geometry  # noqa: E402

H, W = 1280, 1920
PEAK_FP32_VECTOR = 157.3e12
FLOP_PER_PAIR = 8        # three subtractions, a multiply, two fused multiply-adds (two flop each), a minimum
CHUNK_DISTANCES = 1 << 23


def make(n, seed=0):
    g = np.random.default_rng(seed)
    hits = g.choice(H * W, n, replace=False)
    gt = np.zeros(H * W, np.float32)
    gt[hits] = g.uniform(2.0, 70.0, n)
    pred = g.uniform(1.0, 75.0, H * W).astype(np.float32)
    pred[hits] = gt[hits] * (1 + g.normal(0, 0.02, n))
    rows = np.arange(H * W) // W
    dyn = g.uniform(0, 1, H * W) < 0.25
    human = dyn & (g.uniform(0, 1, H * W) < 0.2)
    masks = {"sky_masks": ~dyn & (rows < H // 8), "dynamic_masks": dyn, "human_masks": human, "vehicle_masks": dyn & ~human}
    K = np.array([[2000.0, 0, W / 2 - 0.5], [0, 2000.0, H / 2 - 0.5], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (350.0, -120.0, 2.0)
    t = lambda a: torch.as_tensor(a).cuda()
    return t(pred.reshape(H, W)), t(gt.reshape(H, W)), t(K), t(c2w), {k: t(v.reshape(H, W)) for k, v in masks.items()}


def side_a(pred, gt, K, c2w, masks):
    return geometry.geometry_metrics(pred, gt, K, c2w, masks)


def _unproject(depth, K, c2w, mask):
    v, u = torch.where(mask)
    z = depth[v, u]
    cam = torch.stack(((u.float() - K[0, 2]) * z / K[0, 0], (v.float() - K[1, 2]) * z / K[1, 1], z, torch.ones_like(z)), 1)
    return (c2w @ cam.T).T[:, :3].contiguous()


def _nearest(x, y):
    out = torch.empty(len(x), device=x.device)
    chunk = max(1, CHUNK_DISTANCES // max(len(y), 1))
    for i in range(0, len(x), chunk):
        out[i:i + chunk] = torch.cdist(x[i:i + chunk], y, compute_mode="donot_use_mm_for_euclid_dist").min(1).values.square()
    return out


def _trimmed(sorted_vals, q):
    return sorted_vals[:int(sorted_vals.numel() * q)].mean()


def side_b(pred, gt, K, c2w, masks):
    """Framework ops: device scalars under the same names as side_a (boolean indexing waits on the host for its counts)."""
    valid = (gt > 0.01) & (gt < 80.0) & (pred > 0.0001) & (pred < 80.0)
    P, G = _unproject(pred, K, c2w, valid), _unproject(gt, K, c2w, valid)
    sp, sg = torch.sort(_nearest(P, G)).values, torch.sort(_nearest(G, P)).values
    err = torch.sort((pred[valid] - gt[valid]).abs()).values
    out = {"chamfer": sp.mean() + sg.mean(), "depth_err": err.square().mean().sqrt(), "depth_err_median_squared": err.square().median()}
    for tag, q in (("_99", 0.99), ("_97", 0.97), ("_95", 0.95)):
        out[f"chamfer{tag}"] = _trimmed(sp, q) + _trimmed(sg, q)
        out[f"depth_err_rmse{tag}"] = err[:int(err.numel() * q)].square().mean().sqrt()
    inside = {c: masks[k] for c, k in zip(geometry.CLASSES, geometry.MASK_KEYS)}
    inside["background"] = ~(inside["sky"] | inside["dynamic"] | inside["human"] | inside["vehicle"])
    for c, m in inside.items():
        sel = m[valid]
        out[f"chamfer_{c}"] = _nearest(P[sel], G[sel]).mean() + _nearest(G[sel], P[sel]).mean()
    return out


def timed(fns, args, warmup, repeats):
    ms = [[] for _ in fns]
    for i in range(warmup + repeats):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            fn(*args)
            e.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[j].append(s.elapsed_time(e))
    return [{"median": statistics.median(m), "min": min(m), "max": max(m)} for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--points", type=int, nargs="+", default=[40000, 150000])
    ap.add_argument("--no-framework", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "warmup": a.warmup, "repeats": a.repeats, "frames": []}
    for n in a.points:
        args = make(n)
        ra = side_a(*args)
        counts = [float(ra["valid"])] + [float(ra[f"{c}_valid"]) for c in geometry.CLASSES]
        pairs = 2.0 * sum(c * c for c in counts)
        fns = (side_a,) if a.no_framework else (side_a, side_b)
        t = timed(fns, args, a.warmup, a.repeats)
        rate = pairs / (t[0]["median"] * 1e-3)
        frame = {"valid": counts[0], "class_points": dict(zip(geometry.CLASSES, counts[1:])), "pairs": pairs, "fused_ms": t[0],
                 "pairs_per_s": rate, "share_of_fp32_vector_peak": rate * FLOP_PER_PAIR / PEAK_FP32_VECTOR}
        if not a.no_framework:
            rb = side_b(*args)
            frame.update({"framework_ms": t[1], "fused_over_framework": t[0]["median"] / t[1]["median"],
                          "fused_vs_framework_abs_diff": {k: abs(float(ra[k]) - float(rb[k])) for k in rb}})
        res["frames"].append(frame)
        print(json.dumps(frame), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
