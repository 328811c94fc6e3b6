#!/usr/bin/env python3
"""Time the scoring of one 1080p evaluation frame with four masks (bilateral_driving_amd/metrics.py) in three forms:
(a) the fused op (image_metrics: two launches, no host wait); (b) the same expression as framework ops on the same GPU in the same
process -- index-built symmetric padding, avg_pool2d for the five moments, boolean indexing for the masks, as the reference's lines
(models/video_utils.py:273-361) would read if they stayed on the device; (c) the host restatement with scipy on the CPU
(tests/metrics_ref64.py), once.  Warm-up, then the median of repeated timed regions of several calls each (HIP events), a and b
alternating.  Also records, over the test shapes and image kinds, the worst ratio of the kernel's error to the tests' bound.

    python scripts/eval_metrics_time.py --out profiles/eval_metrics_time.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/eval_metrics_time.py --profile       (kernel table of the fused op)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import metrics  # noqa: E402
from tests import metrics_ref64 as R  # noqa: E402

H, W = 1080, 1920
PREFIX = {"sky_masks": "occupied", "dynamic_masks": "masked", "human_masks": "human", "vehicle_masks": "vehicle"}


def make(seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    masks = {k: torch.rand(H, W, generator=g) < p for k, p in (("sky_masks", 0.3), ("dynamic_masks", 0.2), ("human_masks", 0.02),
                                                                ("vehicle_masks", 0.1))}
    return pred, gt, masks


def side_a(pred, gt, masks):
    return metrics.image_metrics(pred, gt, {PREFIX[k]: v for k, v in masks.items()}, invert=("occupied",))


_INDEX = {}


def _reflect_index(n, dev):
    """Index tensor of scipy's mode="reflect" padding; built once per (n, device), outside the timed regions (the first call is in the
    untimed comparison run of main)."""
    if (n, dev) not in _INDEX:
        i = torch.arange(-R.PAD, n + R.PAD, device=dev)
        _INDEX[n, dev] = torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))
    return _INDEX[n, dev]


def framework_psnr(a, b):
    return -10 * torch.log10(F.mse_loss(a, b))


def side_b(pred, gt, masks):
    """Framework ops: returns device scalars under the same names as side_a (the masked entries wait on the host for their counts and
    index lists, as boolean indexing does)."""
    iy, ix = _reflect_index(H, pred.device), _reflect_index(W, pred.device)
    x, y = (t.permute(2, 0, 1)[:, iy][:, :, ix][None] for t in (pred, gt))          # [1,3,H+6,W+6], mode="reflect" of scipy
    ux, uy, uxx, uyy, uxy = (F.avg_pool2d(t, R.WIN, 1) for t in (x, y, x * x, y * y, x * y))
    cov = R.WIN * R.WIN / (R.WIN * R.WIN - 1.0)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    S = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4) / ((ux ** 2 + uy ** 2 + 1e-4) * (vx + vy + 9e-4)))[0].permute(1, 2, 0)   # [H,W,3]
    out = {"psnr": framework_psnr(pred, gt), "ssim": S[R.PAD:-R.PAD, R.PAD:-R.PAD].mean((0, 1)).mean()}
    for key, m in masks.items():
        m = ~m if key == "sky_masks" else m
        if m.sum() > 0:
            out[f"{PREFIX[key]}_psnr"] = framework_psnr(pred[m], gt[m])
            out[f"{PREFIX[key]}_ssim"] = S[m].mean()
    return out


def timed(fns, args, warmup, repeats, calls):
    """Median / min / max milliseconds PER CALL of each fn, the fns alternating region by region."""
    ms = [[] for _ in fns]
    for i in range(warmup + repeats):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(calls):
                fn(*args)
            e.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[j].append(s.elapsed_time(e) / calls)
    return [{"median": statistics.median(m), "min": min(m), "max": max(m)} for m in ms]


def accuracy():
    """Worst ratio of the kernel's error to the tests' bound (twice the float32 restatement's own error against float64, plus 1e-6)
    over the test shapes and image kinds, for the map and for the ten scalars."""
    worst = {"map": (0.0, None), "scalars": (0.0, None)}
    for Hs, Ws in R.SHAPES:
        for kind in R.KINDS:
            pred, gt, masks, r64, r32 = R.case(Hs, Ws, kind)
            got = metrics.image_metrics(torch.as_tensor(pred).cuda(), torch.as_tensor(gt).cuda(),
                                        {PREFIX[k]: torch.as_tensor(v).cuda() for k, v in masks.items()}, return_map=True,
                                        invert=("occupied",))
            bound, _ = R.bound(r64, r32, "ssim_map")
            ratio = float(np.abs(got["ssim_map"].cpu().numpy().astype(np.float64) - r64["ssim_map"]).max()) / bound
            worst["map"] = max(worst["map"], (ratio, f"{Hs}x{Ws} {kind}"), key=lambda t: t[0])
            for k in r64:
                if k != "ssim_map":
                    ratio = abs(float(got[k]) - r64[k]) / R.bound(r64, r32, k)[0]
                    worst["scalars"] = max(worst["scalars"], (ratio, f"{Hs}x{Ws} {kind} {k}"), key=lambda t: t[0])
    return {k: {"worst_ratio_to_bound": v[0], "case": v[1]} for k, v in worst.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed region")
    ap.add_argument("--profile", action="store_true", help="a few fused calls at 1080p for a kernel trace")
    a = ap.parse_args()
    pred_c, gt_c, masks_c = make()
    pred, gt, masks = pred_c.cuda(), gt_c.cuda(), {k: v.cuda() for k, v in masks_c.items()}
    if a.profile:
        for _ in range(20):
            side_a(pred, gt, masks)
        torch.cuda.synchronize()
        return
    ra, rb = side_a(pred, gt, masks), side_b(pred, gt, masks)
    diff = {k: abs(float(ra[k]) - float(rb[k])) for k in rb}
    ta, tb = timed((side_a, side_b), (pred, gt, masks), a.warmup, a.repeats, a.calls)
    t0 = time.perf_counter()
    rc = R.reference_frame(pred_c.numpy(), gt_c.numpy(), {k: v.numpy() for k, v in masks_c.items()}, np.float32)
    tc = (time.perf_counter() - t0) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "H": H, "W": W, "masks": len(masks), "warmup": a.warmup, "repeats": a.repeats,
           "calls_per_region": a.calls, "fused_ms": ta, "framework_ms": tb, "fused_over_framework": ta["median"] / tb["median"],
           "host_scipy_ms_once": tc, "host_note": "the restatement forms the map once; the reference forms it up to five times",
           "algorithmic_bytes": {"metrics_tile_kernel": H * W * (24 + 4), "metrics_reduce_kernel": ((H + 15) // 16) * ((W + 15) // 16) * 128},
           "fused_vs_framework_abs_diff": diff, "fused_vs_host_float32_abs_diff": {k: abs(float(ra[k]) - rc[k]) for k in rb},
           "accuracy": accuracy()}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
