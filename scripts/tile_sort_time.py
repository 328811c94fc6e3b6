#!/usr/bin/env python3
"""Times the tile stage's two C entries, bds_isect_prepare (compaction, depth sort of the visible entries, counting) and
bds_isect_build (emission, tile sort, offsets), each alone and into preallocated buffers, on the projection outputs of the first view of
bench.py's headline workload (2M Gaussians in Morton order, first camera of the six-camera ring, 1920x1080, culled lists): 64-px list
tiles in the four settings of the size hooks (options 4 and 6: short sort, packed entries), and 16-px list tiles (13-bit tile key: two
passes) in the default setting.  Device events around CALLS calls after a warm-up; the median of REPS such windows, in microseconds
per call, as one JSON line.  BDS_LIB selects the library (an A/B variant built by build.build(out=...)).

    python scripts/tile_sort_time.py [--calls 30] [--reps 5] [--gaussians 2000000]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import _lib as L      # noqa: E402
from bilateral_driving_amd import gs_ops as ops      # noqa: E402
from bilateral_driving_amd import harness as Hn      # noqa: E402

W, H = 1920, 1080


def timed(fn, calls, reps):
    for _ in range(5):
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


def view_inputs(N):
    dev = "cuda:0"
    cam = Hn.ring_cameras(W, H, yaws_deg=Hn.SIX_CAM_YAWS, device=dev)[0]
    p = Hn.synthetic_scene(N, seed=0, device=dev)
    perm = Hn.spatial_order(p["means"])
    p = {k: v[perm].contiguous() for k, v in p.items()}
    radii, means2d, depths, conics, _ = ops.fully_fused_projection(p["means"], p["quats"], torch.exp(p["log_scales"]), cam.viewmat[None],
                                                                   cam.K[None], W, H, eps2d=0.3, near_plane=0.1, far_plane=1e10)
    opac = torch.sigmoid(p["opacity_logits"])[None].contiguous()
    return [t.detach().contiguous() for t in (means2d, radii, depths, conics, opac)]


def entries(inputs, ts):
    """The two calls of gs_ops.isect_tiles for list tiles of ``ts`` px, with every buffer allocated up front."""
    means2d, radii, depths, conics, opac = inputs
    lib, st = L.lib(), L.stream()
    Cn, N = radii.shape
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    e = lambda *s, dtype: torch.empty(*s, dtype=dtype, device="cuda")
    tpg = e(Cn, N, dtype=torch.int32)
    wsb = lib.bds_isect_prepare_workspace_bytes(Cn, N)
    ws = e(max(wsb, 16), dtype=torch.uint8)
    counts = (C.c_int64 * 2)()

    def prepare():
        L.check(lib.bds_isect_prepare(Cn, N, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(conics), L.ptr(opac), ts, tw, th, L.ptr(tpg),
                                      L.ptr(ws), wsb, -1, -1, counts, None, 0, st), "bds_isect_prepare")
    prepare()
    M, n_vis = counts
    fids, offs = e(M, dtype=torch.int32), e(Cn, th, tw, dtype=torch.int32)
    ws2b = lib.bds_isect_build_workspace_bytes(Cn, N, M)
    ws2 = e(max(ws2b, 16), dtype=torch.uint8)

    def build():
        L.check(lib.bds_isect_build(Cn, N, M, n_vis, L.ptr(means2d), L.ptr(radii), L.ptr(depths), L.ptr(conics), L.ptr(opac), ts, tw, th,
                                    L.ptr(ws), wsb, L.ptr(ws2), ws2b, None, L.ptr(fids), L.ptr(offs), None, 0, 0, st), "bds_isect_build")
    return prepare, build, int(M), int(n_vis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the timings need the MI355X"
    inputs = view_inputs(a.gaussians)
    res, sizes = {}, {}
    try:
        for ts, regimes in ((64, ((1, 1), (0, 1), (1, 0), (0, 0))), (16, ((1, 1),))):
            for short, packed in regimes:
                L.set_option(L.OPT_SHORT_SORT, short); L.set_option(L.OPT_PACKED, packed)
                prepare, build, M, n_vis = entries(inputs, ts)
                tag = f"tile{ts}_short{short}_packed{packed}"
                sizes[f"tile{ts}"] = dict(pairs=M, visible=n_vis)
                res[f"bds_isect_prepare/{tag}"] = round(timed(prepare, a.calls, a.reps), 2)
                prepare()      # (the build reads what the last prepare left in the workspace)
                res[f"bds_isect_build/{tag}"] = round(timed(build, a.calls, a.reps), 2)
    finally:
        L.set_option(L.OPT_SHORT_SORT, 1); L.set_option(L.OPT_PACKED, 1)
    print(json.dumps({"lib": os.path.basename(L.LIB_PATH), "sizes": sizes, "us_per_call": res}))


if __name__ == "__main__":
    main()
