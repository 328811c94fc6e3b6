#!/usr/bin/env python3
"""Times the pseudo-lidar generation of one frame (bilateral_driving_amd/pseudo_lidar.py: six 1920x1080 depth maps to 32 x 256 beams
each) against the same computation written as framework ops on the same GPU -- this script's own restatement of the reference's steps
(a boolean compaction, two 4 x N products, the angles in float64, the winner by an amax scatter of the pixel index, a gather), not
reference text.  Device events around each form, the median of REPS runs after one warm-up.

    python scripts/pseudo_lidar_time.py [--out profiles/pseudo_lidar_time.json] [--reps 5]

Also timed, the C entry alone into preallocated outputs (no table upload, no allocation), on the street's maps and on all-zero maps:
with no valid pixel the bin kernel only reads the depth, so the difference between the two is what the unprojection, the FP64 angles
(two sqrt, two divisions, two asin per live pixel) and the atomics cost together."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import pseudo_lidar as PL      # noqa: E402

CAMS, HI, WI, H, W = 6, 1080, 1920, 32, 256


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def scene(dev):
    """Six cameras around the lidar, 60 degrees apart, 1.6 m above a ground plane, walls 8 m to both sides of each view, 2 % noise."""
    g = torch.Generator().manual_seed(0)
    fx = 1000.0
    K = torch.tensor([[fx, fx, WI / 2, HI / 2]] * CAMS)
    v, u = torch.meshgrid(torch.arange(HI, dtype=torch.float32), torch.arange(WI, dtype=torch.float32), indexing="ij")
    ground = torch.where(v > HI / 2, 1.6 * fx / (v - HI / 2).clamp(min=1e-3), torch.full_like(v, 1e9))
    walls = 8.0 * fx / (u - WI / 2).abs().clamp(min=1e-3)
    base = torch.minimum(ground, walls)
    depths = torch.stack([base * (0.98 + 0.04 * torch.rand(HI, WI, generator=g)) for _ in range(CAMS)])
    depths[depths > 150] = 0.0
    l2w = torch.eye(4)
    l2w[:3, 3] = torch.tensor([212.0, -148.0, 3.0])
    c2w = []
    for c in range(CAMS):
        yaw = c * math.pi / 3
        fwd, left = np.array([math.cos(yaw), math.sin(yaw), 0.0]), np.array([-math.sin(yaw), math.cos(yaw), 0.0])
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = -left, [0, 0, -1.0], fwd, [0.5 * math.cos(yaw), 0.5 * math.sin(yaw), -0.2]
        c2w.append(l2w.double() @ torch.from_numpy(m))
    return depths.to(dev), K, torch.stack(c2w).float(), l2w


def framework(depths, K, c2w, l2w):
    """One frame as framework ops.  -> list of [M_c,3] (float64, as the reference returns)."""
    dev = depths.device
    dphi, dtheta = math.radians(90.0 / W), (math.radians(10.0) - math.radians(-30.0)) / H
    out = []
    v, u = torch.meshgrid(torch.arange(HI, dtype=torch.float32, device=dev), torch.arange(WI, dtype=torch.float32, device=dev), indexing="ij")
    w2l = torch.inverse(l2w).to(dev)
    for c in range(depths.shape[0]):
        d = depths[c]
        ok = (d > 0) & (d < 80.0)
        pix = torch.nonzero(ok.reshape(-1))[:, 0]
        uu, vv, dd = u[ok], v[ok], d[ok]
        cam = torch.stack([(uu - K[c, 2]) * dd / K[c, 0], (vv - K[c, 3]) * dd / K[c, 1], dd, torch.ones_like(dd)])
        world = c2w[c].to(dev) @ cam
        p = (w2l @ world)[:3].T.double()
        keep = (p[:, 0] < 80) & (p[:, 0] >= 0) & (p[:, 1] < 50) & (p[:, 1] >= -50) & (p[:, 2] < 3) & (p[:, 2] >= -2.5)
        p, pix = p[keep], pix[keep]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        dist, r = torch.sqrt(x * x + y * y + z * z), torch.sqrt(x * x + y * y)
        dist, r = torch.where(dist == 0, 1e-6, dist), torch.where(r == 0, 1e-6, r)
        col = ((math.radians(45.0) - torch.asin(y / r)) / dphi).long().clamp(0, W - 1)
        theta = torch.asin(z / dist)
        fov = (theta >= math.radians(-30.0)) & (theta <= math.radians(10.0))
        row = ((theta - math.radians(-30.0)) / dtheta).long().clamp(0, H - 1)
        cell = (row * W + col)[fov]
        order = torch.arange(len(pix), device=dev)[fov]
        winner = torch.full((H * W,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, cell, order, "amax")
        out.append(p[winner[winner >= 0]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pseudo_lidar_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    depths, K, c2w, l2w = scene(dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "cameras": CAMS, "image": [HI, WI], "beams": [H, W], "ms": {}}
    pts, counts = PL.depth_to_lidar(depths, K, c2w, l2w, H, W)
    theirs = framework(depths, K, c2w, l2w)
    n = counts.cpu().tolist()
    res["emitted"] = n
    res["framework_emitted"] = [len(t) for t in theirs]
    res["live_fraction"] = float(((depths > 0) & (depths < 80)).float().mean())
    res["ms"]["depth_to_lidar"] = timed(lambda: PL.depth_to_lidar(depths, K, c2w, l2w, H, W), a.reps)
    res["ms"]["framework"] = timed(lambda: framework(depths, K, c2w, l2w), a.reps)
    L, lib = PL.L, PL.L.lib()
    cams = PL.camera_table(K, c2w, l2w).to(dev)
    beams = torch.from_numpy(PL.beam_table(H, W)).to(dev)
    winner = torch.empty(CAMS, H, W, dtype=torch.int32, device=dev)
    points = torch.empty(CAMS, H * W, 3, device=dev)
    cnt = torch.zeros(CAMS, dtype=torch.int32, device=dev)

    def entry(maps):
        L.check(lib.bds_pseudo_lidar_from_depth(CAMS, HI, WI, L.ptr(maps), L.ptr(cams), L.ptr(beams), H, W, 1, PL.VERTICAL, L.ptr(winner),
                                                L.ptr(points), L.ptr(cnt), None, L.stream()), "bds_pseudo_lidar_from_depth")
    zeros = torch.zeros_like(depths)
    res["ms"]["entry_only"] = timed(lambda: entry(depths), a.reps)
    res["ms"]["entry_only_no_valid_pixel"] = timed(lambda: entry(zeros), a.reps)
    res["bytes_read"] = CAMS * HI * WI * 4
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
