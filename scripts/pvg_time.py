#!/usr/bin/env python3
"""Time the periodic-vibration Gaussians' fused time transform (bilateral_driving_amd/pvg.py) against the framework form on the same
GPU in the same process: A = framework_transform (SH through the fused SH op, as the reference calls gsplat's) + the five mask gathers
+ the reference-style NaN / Inf scan (ten reductions, each with a host wait); B = time_transform + the flag test.  Forward alone and
forward + backward of a weighted sum; warm-up, then the median of the repeats (HIP events around each call).

    python scripts/pvg_time.py --out profiles/pvg_time.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/pvg_time.py --profile        (kernel table: N = 10^6, degree 3)

Each case also records the algorithmic bytes of the fused launches for its N, M and K (see `algorithmic_bytes`)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import gs_ops, pvg  # noqa: E402

T, SCALE = 0.2, 0.78
CASES = ((100_000, 16), (1_000_000, 16), (3_000_000, 16), (1_000_000, 1))      # (N, K): SH degree 3, and the sigmoid form
KEYS = ("_means", "_opacities", "_rgbs", "_scales", "_quats")


def make(N, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    p = [(r(N, 3) - 0.5) * 40, torch.randn(N, 3, generator=g), r(N, 1) * SCALE, torch.log(0.03 * (0.4 / 0.03) ** r(N, 1)),
         torch.randn(N, 1, generator=g) * 2, r(N, 3) * 4 - 4, torch.randn(N, 4, generator=g), r(N, 3) - 0.5,
         torch.randn(N, K - 1, 3, generator=g) * 0.2]
    return [x.cuda().requires_grad_(True) for x in p], torch.tensor([1.5, -2.0, 0.7]).cuda()


def side_a(p, cam, args):
    *dense, mask = pvg.framework_transform(*p, cam, *args, sh=gs_ops.spherical_harmonics)
    gs = {k: v[mask] for k, v in zip(KEYS, dense)}
    for k, v in gs.items():
        if torch.isnan(v).any():
            raise ValueError(k)
        if torch.isinf(v).any():
            raise ValueError(k)
    return list(gs.values())


def side_b(p, cam, args):
    info = {}
    *outs, _mask = pvg.time_transform(*p, cam, *args, info=info)
    if info["flags"]:
        raise ValueError(info["flags"])
    return outs


def timed(fn, p, cam, args, backward, warmup, repeats):
    ms = []
    for i in range(warmup + repeats):
        for x in p:
            x.grad = None
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        outs = fn(p, cam, args)
        if backward:
            sum((o * (j + 1)).sum() for j, o in enumerate(outs)).backward()
        e.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def algorithmic_bytes(N, M, K):
    """Bytes each fused launch has to move: count reads tau, beta and writes the mask byte for all N rows; write reads the mask byte of
    all N rows and, per kept row, the 36 B of time parameters (mean, velocity, tau, beta, logit), scale, quaternion and the SH row,
    and writes the 56 B compact row + 12 B of un-clamped colour; the backward reads per kept row the parameters it needs, 24 B of
    saved outputs and the 56 B gradient row, and writes all nine gradients for all N rows."""
    sh = 12 * K
    return {"pvg_count_kernel": N * 9, "pvg_write_kernel": N * 1 + M * (36 + 12 + 16 + sh + 56 + 12),
            "pvg_bwd_kernel": N * 1 + M * (12 + 12 + 12 + 16 + 24 + 56) + N * (12 + 12 + 12 + 12 + 16 + sh)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--profile", action="store_true", help="a few fused forward + backward calls at N = 10^6, degree 3, for a kernel trace")
    a = ap.parse_args()
    args = (0.417, -0.017, True, T)
    if a.profile:
        p, cam = make(1_000_000, 16)
        for _ in range(10):
            for x in p:
                x.grad = None
            sum(o.sum() for o in side_b(p, cam, args + (3,))).backward()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats, "cases": []}
    for N, K in CASES:
        p, cam = make(N, K)
        deg = 3 if K == 16 else 0
        M = int(side_b(p, cam, args + (deg,))[0].shape[0])
        case = {"N": N, "K": K, "degrees_to_use": deg, "M": M, "algorithmic_bytes": algorithmic_bytes(N, M, K)}
        for name, backward in (("fwd", False), ("fwd_bwd", True)):
            ta = timed(side_a, p, cam, args + (deg,), backward, a.warmup, a.repeats)
            tb = timed(side_b, p, cam, args + (deg,), backward, a.warmup, a.repeats)
            case[name] = {"framework_ms": {"median": ta[0], "min": ta[1], "max": ta[2]}, "fused_ms": {"median": tb[0], "min": tb[1], "max": tb[2]},
                          "speedup": ta[0] / tb[0]}
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
