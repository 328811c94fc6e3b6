#!/usr/bin/env python3
"""Time of the fused pose transform of the node classes (csrc/nodes.hip through ``nodes.pose_transform``) against the same expression
as framework ops (``nodes.framework_transform``: normalise, quat_to_rotmat, the [N,3,3] gather, bmm, quat_mult, the fv mask), forward
only and forward + backward (gradients of the point tensors and of the instance quaternions / translations, as the trainer needs).

    python scripts/node_pose_time.py [--out profiles/node_pose_time.json] [--sizes 5000,50000,200000,1000000] [--instances 8,64,256]
    python scripts/node_pose_time.py --profile N      (a few fused forward + backward calls, for rocprofv3 --kernel-trace --stats)

Ids are in random order.  Device events around each call after a warm-up, A and B alternated over the repeats; the median is
reported (ms).  The fused side passes a flag word, so it reads nothing back (the bad-id check rides on get_gaussians' one read)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import nodes  # noqa: E402

F = 40


def make(N, I, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = dict(means=torch.randn(N, 3, generator=g) * 2, quats=torch.randn(N, 4, generator=g), logits=torch.randn(N, 1, generator=g),
             instances_quats=torch.randn(F, I, 4, generator=g), instances_trans=torch.randn(F, I, 3, generator=g))
    d = {k: v.cuda().requires_grad_(True) for k, v in d.items()}
    d["point_ids"] = torch.randint(0, I, (N, 1), generator=g).cuda()
    d["instances_fv"] = (torch.rand(F, I, generator=g) > 0.2).cuda()
    return d


def call(d, fused, flags):
    args = (d["means"], d["quats"], d["logits"], d["point_ids"], d["instances_quats"], d["instances_trans"], d["instances_fv"], 7)
    if fused:
        return nodes.pose_transform(*args, flags=flags)
    return nodes.framework_transform(*args)


def step(d, fused, backward, flags, ws):
    for k in ("means", "quats", "logits", "instances_quats", "instances_trans"):
        d[k].grad = None
    if not backward:
        with torch.no_grad():
            call(d, fused, flags)
        return
    wm, wq, op = call(d, fused, flags)
    ((wm * ws[0]).sum() + (wq * ws[1]).sum() + (op * ws[2]).sum()).backward()


def timed(fn, reps):
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/node_pose_time.json")
    ap.add_argument("--sizes", default="5000,50000,200000,1000000")
    ap.add_argument("--instances", default="8,64,256")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    L.lib()
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    if a.profile:
        d = make(a.profile, 64)
        ws = [torch.randn(a.profile, c, device="cuda") for c in (3, 4, 1)]
        for _ in range(5):
            step(d, True, True, flags, ws)
            step(d, False, True, flags, ws)
        torch.cuda.synchronize()
        return
    rows = []
    for N in [int(x) for x in a.sizes.split(",")]:
        for I in [int(x) for x in a.instances.split(",")]:
            d = make(N, I)
            ws = [torch.randn(N, c, device="cuda") for c in (3, 4, 1)]
            for backward in (False, True):
                for _ in range(5):
                    step(d, True, backward, flags, ws)
                    step(d, False, backward, flags, ws)
                torch.cuda.synchronize()
                tf, tr = [], []
                for _ in range(a.reps):
                    tf += timed(lambda: step(d, True, backward, flags, ws), 1)
                    tr += timed(lambda: step(d, False, backward, flags, ws), 1)
                mf, mr = statistics.median(tf), statistics.median(tr)
                row = dict(N=N, I=I, mode="fwd+bwd" if backward else "fwd", fused_ms=round(mf, 4), framework_ms=round(mr, 4),
                           speedup=round(mr / mf, 2), fused_min_ms=round(min(tf), 4), framework_min_ms=round(min(tr), 4))
                print(json.dumps(row), flush=True)
                rows.append(row)
            del d, ws
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), frames=F, reps=a.reps, rows=rows,
               note="median of device-event times around one call (ms); ids in random order; the backward includes the loss's "
                    "own reductions on both sides")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
