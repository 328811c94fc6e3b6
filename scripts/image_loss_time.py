#!/usr/bin/env python3
"""Time of the image loss of one 1920 x 1080 view, forward + backward, in three forms on the same inputs in one process:
  (a) framework   the reference's expressions as framework ops (tests/image_loss_ref64.framework_terms)
  (b) two_nodes   losses.pixel_loss + losses.reg_losses: the same kernels as (c) called as two nodes, each with the other's terms off (the
                  two names are option sets of image_terms; before that fold they had kernels of their own, which the 0.198 ms of
                  profiles/image_loss_time.json is of)
  (c) image_terms the one node
with the option set all three can form (bce, l1 depth without normalize / inverse, every regulariser, an egocar mask).  Median of
device events over --iters runs after --warmup, in the rounds c b a c b a c (A / B / A: every b and a lies between two rounds of c).

    python scripts/image_loss_time.py [--out profiles/image_loss_time.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_loss_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    args = ap.parse_args()
    from bilateral_driving_amd import losses
    from tests import image_loss_ref64 as R
    d = {k: v.cuda() for k, v in R.make(args.height, args.width, 1).items()}
    o = R.options()
    w_reg = torch.tensor(R.W6[3:], device="cuda")
    v = torch.tensor(R.V6, device="cuda")

    def two_nodes(rgb, pixels, opacity, depth, **kw):
        pix = losses.pixel_loss(rgb, opacity, depth, pixels, kw["sky_masks"], kw["lidar_depth"], kw["egocar_masks"], *R.W6[:3], "l1", 80.0)
        return torch.cat([pix, losses.reg_losses(pixels, opacity, depth, rgb, kw["dyn_opacity"], kw["egocar_masks"], 0.2) * w_reg])

    def step(fn):
        pos, kw = R.call_args(d, o)
        leaves = [pos[k].detach().requires_grad_(True) for k in (0, 2, 3)]
        (fn(leaves[0], pos[1], leaves[1], leaves[2], **kw) * v).sum().backward()

    def time(fn):
        for _ in range(args.warmup):
            step(fn)
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(fn)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    forms = {"framework": R.framework_terms, "two_nodes": two_nodes, "image_terms": losses.image_terms}
    rounds = [(name, time(forms[name])) for name in ("image_terms", "two_nodes", "framework") * 2 + ("image_terms",)]
    out = dict(height=args.height, width=args.width, iters=args.iters, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               rounds_ms=[dict(form=n, median_ms=round(t, 4)) for n, t in rounds],
               note="forward + backward of one view, host launch overhead included; image_terms is timed first, between and last")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
