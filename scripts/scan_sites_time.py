#!/usr/bin/env python3
"""Times the C entries whose kernels share csrc/scan.h, each alone and into preallocated buffers: bds_refine_plan, bds_pvg_fwd,
bds_lidar_points_in_boxes_count + _emit, bds_depth_unproject, bds_knn_self and bds_union_slots at 10^6 rows (the unprojection: one
1080p frame).  Device events around CALLS calls after a warm-up; the median of REPS such windows, in microseconds per call, as one
JSON line.  BDS_LIB selects the library (an A/B variant built by build.py --variant).

    python scripts/scan_sites_time.py [--calls 50] [--reps 5]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import _lib as L      # noqa: E402
from bilateral_driving_amd import lidar as LD      # noqa: E402

N, H, W, K = 1_000_000, 1080, 1920, 16


def timed(fn, calls, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        us.append(s.elapsed_time(e) * 1000.0 / calls)
    return statistics.median(us)


def sites():
    lib, st = L.lib(), L.stream()
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g, device="cuda")
    e = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="cuda")
    u8 = lambda n: e(max(int(n), 16), dtype=torch.uint8)
    out = {}

    ls, lg, xs, vc, m2 = r(N, 3) * 7.5 - 4.5, r(N) * 9 - 6.5, r(N) * 0.004, torch.floor(r(N) * 6) + 1, r(N) * 0.2
    flags, ranks, totals = e(N, dtype=torch.uint8), e(N, 4, dtype=torch.int32), e(5, dtype=torch.int64)
    nb = int(lib.bds_refine_plan_temp_bytes(N))
    temp = u8(nb)
    out["bds_refine_plan"] = lambda: L.check(lib.bds_refine_plan(
        N, L.ptr(xs), L.ptr(vc), L.ptr(m2), L.ptr(ls), L.ptr(lg), None, 1, 0.0003, 0.06, 1, 0.05, 1, 0.005, 1, 15.0, 1, 0.15, L.ptr(flags),
        L.ptr(ranks), L.ptr(totals), L.ptr(temp), nb, st), "bds_refine_plan")

    m, v, ta, be = (r(N, 3) - 0.5) * 40, (r(N, 3) - 0.5) * 4, r(N) * 0.78, torch.log(0.03 * (0.4 / 0.03) ** r(N))
    lo, sc, q, dc, rest, cam = r(N) * 4 - 2, r(N, 3) * 4 - 4, r(N, 4) - 0.5, r(N, 3) - 0.5, (r(N, K - 1, 3) - 0.5) * 0.5, r(3)
    o = [e(N, w) for w in (3, 1, 3, 3, 4, 3)]
    mask = e(N, dtype=torch.bool)
    pb = int(lib.bds_pvg_temp_bytes(N))
    ptemp = u8(pb)
    out["bds_pvg_fwd"] = lambda: L.check(lib.bds_pvg_fwd(
        N, K, 3, 0.417, -0.017, 1, 0.2, L.ptr(m), L.ptr(v), L.ptr(ta), L.ptr(be), L.ptr(lo), L.ptr(sc), L.ptr(q), L.ptr(dc), L.ptr(rest),
        L.ptr(cam), *[L.ptr(t) for t in o], L.ptr(mask), L.ptr(ptemp), pb, st), "bds_pvg_fwd")

    pts = (r(N, 3) - 0.5) * 20
    B = 8
    poses = torch.eye(4).repeat(1, B, 1, 1)
    yaw = torch.arange(B) * 0.7
    poses[0, :, 0, 0], poses[0, :, 0, 1], poses[0, :, 1, 0], poses[0, :, 1, 1] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos()
    poses[0, :, :3, 3] = torch.stack([torch.cos(yaw * 3), torch.sin(yaw * 2), 0.2 * yaw - 2], 1) * 3
    w2o, half, ids = (t.cuda() for t in LD.box_tables(poses, torch.full((B, 3), 6.0), torch.ones(1, B, dtype=torch.bool)))
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    lws = u8(lib.bds_lidar_boxes_workspace_bytes(N))
    count = lambda: L.check(lib.bds_lidar_points_in_boxes_count(N, L.ptr(pts), B, L.ptr(w2o), L.ptr(half), None, LD.BOX_CHUNK, L.ptr(total),
                                                                L.ptr(lws), lws.numel(), st), "bds_lidar_points_in_boxes_count")
    count()
    M = int(total.item())
    rec_ids, rec_xyz = e(M, 3, dtype=torch.int32), e(M, 3)

    def boxes():
        count()
        L.check(lib.bds_lidar_points_in_boxes_emit(N, L.ptr(pts), B, L.ptr(w2o), L.ptr(half), None, L.ptr(ids), LD.BOX_CHUNK, L.ptr(lws),
                                                   lws.numel(), M, L.ptr(rec_ids), L.ptr(rec_xyz), st), "bds_lidar_points_in_boxes_emit")
    out["bds_lidar_points_in_boxes_count+emit"] = boxes

    depth, valid = r(H, W) * 78 + 0.5, (r(H, W) < 0.5).to(torch.uint8)
    Km = torch.tensor([[0.8 * W, 0, 0.5 * W], [0, 0.8 * W, 0.5 * H], [0, 0, 1]], device="cuda")
    c2w = torch.eye(4, device="cuda")
    cloud, n_out = e(H * W, 3), torch.zeros(1, dtype=torch.int64, device="cuda")
    gws = u8(lib.bds_geometry_metrics_workspace_bytes(H, W))
    out["bds_depth_unproject"] = lambda: L.check(lib.bds_depth_unproject(
        H, W, L.ptr(depth), L.ptr(valid), 0, L.ptr(Km), L.ptr(c2w), L.ptr(cloud), L.ptr(n_out), L.ptr(gws), gws.numel(), st),
        "bds_depth_unproject")

    x = r(N, 3) * 50
    dist, idx = e(N, 3), e(N, 3, dtype=torch.int32)
    kws = u8(lib.bds_knn_workspace_bytes(N))
    out["bds_knn_self"] = lambda: L.check(lib.bds_knn_self(N, L.ptr(x), 3, L.ptr(dist), L.ptr(idx), None, 0, 0.0, math.inf, L.ptr(kws),
                                                          kws.numel(), st), "bds_knn_self")

    um = (r(N) < 0.15).to(torch.uint8)
    cap = 200_000
    row_map, uids = e(N, dtype=torch.int32), e(cap, dtype=torch.int32)
    bufs = [e(*s) for s in ((cap, 3), (cap, 4), (cap, 3), (cap,), (cap, K, 3))]
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    uws = u8(lib.bds_union_slots_workspace_bytes(N))
    out["bds_union_slots"] = lambda: L.check(lib.bds_union_slots(N, L.ptr(um), cap, K, L.ptr(row_map), L.ptr(uids), *[L.ptr(b) for b in bufs],
                                                                 L.ptr(uws), uws.numel(), L.ptr(cnt), None, st), "bds_union_slots")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need the MI355X"
    res = {name: round(timed(fn, a.calls, a.reps), 2) for name, fn in sites().items()}
    print(json.dumps({"lib": os.path.basename(L.LIB_PATH), "us_per_call": res}))


if __name__ == "__main__":
    main()
