#!/usr/bin/env python3
"""Times the lidar scene preparation's ops (bilateral_driving_amd/lidar.py) against the same operations written as framework ops on the
same GPU -- this script's own restatement of the reference's loops (one iteration per frame, or per frame and instance, with a
torch.inverse each), not reference text.  Device events around each op, the median of REPS runs after one warm-up.

    python scripts/lidar_prep_time.py [--out profiles/lidar_prep_time.json] [--reps 5]

Sizes: 1.2 M points in 200 sweeps; six cameras of 200 frames at 1920x1080 (six launch sequences on one stream; the cameras share one
image stack here, 5 GB, and each call allocates its own maps as the wrapper does -- the kernels of one camera are also timed alone,
into preallocated maps, for the bandwidth figure);
check_pts_visibility over 6 x 200 views; F x I = 200 x 100 boxes of which about a third are active; the downsampler at 1080p x 0.5 and
x 0.25."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import lidar as LD      # noqa: E402

N_PTS, SWEEPS, W, H, CAMS, INST = 1_200_000, 200, 1920, 1080, 6, 100


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
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand(N_PTS, 3, generator=g) * torch.tensor([120.0, 80.0, 8.0]) - torch.tensor([40.0, 40.0, 1.0])).to(dev)
    per = N_PTS // SWEEPS
    ranges = torch.stack([torch.arange(SWEEPS) * per, (torch.arange(SWEEPS) + 1) * per], 1).to(dev)
    K4 = torch.tensor([[1100.0, 0, W / 2, 0], [0, 1100.0, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    mats = []
    for f in range(SWEEPS):      # an OpenCV camera looking along +x, moving forward
        c2w = torch.tensor([[0.0, 0, 1, 0.3 * f], [-1, 0, 0, 0], [0, -1, 0, 1.5], [0, 0, 0, 1]])
        mats.append(K4 @ c2w.inverse())
    mats = torch.stack(mats).to(dev)
    poses = torch.eye(4).repeat(SWEEPS, INST, 1, 1)
    yaw = torch.rand(SWEEPS, INST, generator=g) * 6.28
    poses[..., 0, 0], poses[..., 0, 1], poses[..., 1, 0], poses[..., 1, 1] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos()
    poses[..., :3, 3] = torch.rand(SWEEPS, INST, 3, generator=g) * torch.tensor([120.0, 80.0, 2.0]) - torch.tensor([40.0, 40.0, 0.0])
    sizes = torch.rand(INST, 3, generator=g) * torch.tensor([2.0, 1.0, 0.6]) + torch.tensor([3.5, 1.6, 1.4])
    active = torch.rand(SWEEPS, INST, generator=g) < 1 / 3
    return pts, ranges, mats, poses, sizes, active


def fw_project(pts, ranges, mats, images, visible, colors):
    """The reference's loop as framework ops: per frame a projection, a mask, an index_put_ with duplicate indices and a gather."""
    maps = []
    rows = torch.arange(len(pts), device=pts.device)
    for f, (b, e) in enumerate(ranges):
        p = (mats[f, :3, :3] @ pts[b:e].T + mats[f, :3, 3:4]).T
        depth = p[:, 2]
        uv = p[:, :2] / (depth.unsqueeze(-1) + 1e-6)
        ok = (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H) & (depth > 0)
        uv = uv[ok]
        m = torch.zeros(H, W, device=pts.device)
        m[uv[:, 1].long(), uv[:, 0].long()] = depth[ok]
        maps.append(m)
        idx = rows[b:e][ok]
        visible[idx] = True
        colors[idx] = images[f][uv[:, 1].long(), uv[:, 0].long()]
    return torch.stack(maps)


def fw_visible(pts, mats, views):
    out = torch.zeros(len(pts), dtype=torch.bool, device=pts.device)
    for v in range(views):
        M = mats[v % len(mats)]
        p = (M[:3, :3] @ pts.T + M[:3, 3:4]).T
        depth = p[:, 2]
        uv = p[:, :2] / (depth.unsqueeze(-1) + 1e-6)
        out = out | ((uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H) & (depth > 0))
    return out


def fw_box(p, o2w, size):
    w2o = torch.inverse(o2w)
    o = torch.cat([p, torch.ones_like(p[:, :1])], 1) @ w2o.T
    return o, ((o[:, 0] > -size[0] / 2) & (o[:, 0] < size[0] / 2) & (o[:, 1] > -size[1] / 2) & (o[:, 1] < size[1] / 2)
               & (o[:, 2] > -size[2] / 2) & (o[:, 2] < size[2] / 2))


def fw_filter(pts, poses, sizes, active_list):
    inside = torch.zeros(len(pts), dtype=torch.bool, device=pts.device)
    for f, i in active_list:
        inside = inside | fw_box(pts, poses[f, i], sizes[i])[1]
    return inside


def fw_init_objects(pts, ranges, poses, sizes, active_list):
    out = {}
    for f, i in active_list:
        b, e = ranges[f]
        o, m = fw_box(pts[b:e], poses[f, i], sizes[i])
        out.setdefault(i, []).append(o[m, :3])
    return {i: torch.cat(v) for i, v in out.items()}


def fw_downsample(m, s):
    avg = torch.nn.functional.interpolate(m[None, None], scale_factor=s, mode="area")[0, 0]
    hit = torch.nn.functional.interpolate((m > 1e-3).float()[None, None], scale_factor=s, mode="area")[0, 0]
    out = torch.zeros_like(avg)
    out[hit > 0] = avg[hit > 0] / hit[hit > 0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_prep_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    pts, ranges, mats, poses, sizes, active = scene(dev)
    images = torch.rand(SWEEPS, H, W, 3, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "points": N_PTS, "sweeps": SWEEPS, "image": [H, W], "ms": {}, "bytes": {}}

    def both(name, ours, theirs, nbytes=None):
        res["ms"][name] = {"hip": timed(ours, a.reps), "framework": timed(theirs, a.reps)}
        if nbytes:
            res["bytes"][name] = nbytes
        print(name, res["ms"][name], flush=True)

    vis, col = torch.zeros(N_PTS, dtype=torch.uint8, device=dev), torch.zeros(N_PTS, 3, device=dev)
    visb = torch.zeros(N_PTS, dtype=torch.bool, device=dev)
    rl = ranges.cpu().tolist()
    def ours_project():
        for _ in range(CAMS):
            LD.project_points(pts, mats, ranges, W, H, images, vis, col, _checked=True)

    def fw_project_all():
        for _ in range(CAMS):
            fw_project(pts, rl, mats, images, visb, col)
    both("project_six_cameras_200_frames", ours_project, fw_project_all,
         # winner: memset + read; depth: write; points: 3 reads of 12 B; pix 4, visible 1, colours 12 + 12 gathered
         CAMS * (SWEEPS * H * W * 12 + N_PTS * (36 + 4 + 1 + 24)))
    lib, L = LD.L.lib(), LD.L
    depth, winner = torch.empty(SWEEPS, H, W, device=dev), torch.empty(SWEEPS, H, W, dtype=torch.int32, device=dev)
    pix, m3 = torch.empty(N_PTS, dtype=torch.int32, device=dev), mats[:, :3, :].contiguous()
    res["ms"]["project_six_cameras_200_frames"]["hip_kernels_only_one_camera"] = timed(lambda: L.check(lib.bds_lidar_project(
        SWEEPS, W, H, N_PTS, L.ptr(pts), L.ptr(m3), L.ptr(ranges), L.ptr(images), L.ptr(winner), L.ptr(depth), L.ptr(pix), L.ptr(vis),
        L.ptr(col), L.stream()), "project"), a.reps)
    res["bytes"]["project_one_camera_kernels"] = SWEEPS * H * W * 12 + N_PTS * (36 + 4 + 1 + 24)
    del depth, winner
    views = CAMS * SWEEPS
    all_mats, all_sizes = mats.repeat(CAMS, 1, 1), torch.tensor([[W, H]] * views, dtype=torch.int32)
    both("check_pts_visibility_1200_views", lambda: LD.visible_from(pts, all_mats, all_sizes), lambda: fw_visible(pts, mats, views),
         N_PTS * 13)
    active_list = [(int(f), int(i)) for f, i in torch.nonzero(active)]
    dposes, dsizes = poses.to(dev), sizes.to(dev)
    res["active_boxes"] = len(active_list)
    both("filter_pts_in_boxes", lambda: LD.points_in_boxes(pts, poses, sizes, active), lambda: fw_filter(pts, dposes, dsizes, active_list),
         N_PTS * 13)
    both("get_init_objects_records", lambda: LD.points_in_boxes(pts, poses, sizes, active, ranges, emit=True),
         lambda: fw_init_objects(pts, rl, dposes, dsizes, active_list), N_PTS * (12 * 2 + 4 * 2))
    # the device part of the two box forms alone (the tables formed and uploaded once)
    w2o, half, ids = [t.to(dev) for t in LD.box_tables(poses, sizes, active)]
    inside = torch.zeros(N_PTS, dtype=torch.uint8, device=dev)
    res["ms"]["filter_pts_in_boxes"]["hip_kernel_only"] = timed(lambda: L.check(lib.bds_lidar_points_in_boxes(
        N_PTS, L.ptr(pts), len(w2o), L.ptr(w2o), L.ptr(half), None, LD.BOX_CHUNK, L.ptr(inside), L.stream()), "mask"), a.reps)
    m = torch.where(torch.rand(H, W, device=dev) < 0.05, torch.rand(H, W, device=dev) * 80, torch.zeros(H, W, device=dev))
    for s in (0.5, 0.25):
        both(f"downsample_1080p_x{s}", lambda: LD.downsample_sparse_depth(m, s), lambda: fw_downsample(m, s),
             H * W * 4 + int(H * s) * int(W * s) * 4)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
