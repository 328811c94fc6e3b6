"""Cost of rasterize_mode "antialiased" (render.antialiased, trainers/base.py:406): the captured training frame at the headline size
(2 M Gaussians, the six-camera 1920 x 1080 rig, bench.py's scene) as graph_view.FrameGraph replays it, classic against antialiased,
alternated in one process.

    python scripts/antialiased_time.py [--steps 20] [--rounds 5] [--mode both|classic|antialiased] [--out FILE.json]

Prints one JSON line: the median ms per frame of each mode over ``rounds`` regions of ``steps`` frames, and their difference.  Each
region captures its frame afresh (one FrameGraph alive at a time, as bench.py does); the modes alternate region by region.
``--mode`` with one mode only runs that frame (for a ``rocprofv3 --kernel-trace --stats`` run of its own)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(N, W, H, dev):
    from bilateral_driving_amd import harness as Hn
    cams = Hn.ring_cameras(W, H, yaws_deg=Hn.SIX_CAM_YAWS, device=dev)
    for cam in cams:
        cam.viewmat.requires_grad_(True)
    params = Hn.synthetic_scene(N, seed=0, device=dev)
    perm = Hn.spatial_order(params["means"])
    params = {k: v[perm].contiguous().requires_grad_(True) for k, v in params.items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(len(cams), levels=((2, 2, 1), (4, 4, 2), (8, 8, 4)), device=dev)]
    gen = torch.Generator().manual_seed(7)
    skies = [torch.rand(H, W, 3, generator=gen).to(dev).requires_grad_(True) for _ in cams]
    targets = [torch.rand(H, W, 3, generator=gen).to(dev) for _ in cams]
    return cams, params, grids, skies, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "classic", "antialiased"), default="both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    from bilateral_driving_amd.graph_view import FrameGraph
    dev = "cuda:0"
    modes = ("classic", "antialiased") if args.mode == "both" else (args.mode,)
    cams, params, grids, skies, targets = scene(args.gaussians, args.width, args.height, dev)
    times = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:     # alternated, ONE frame alive at a time (a FrameGraph binds the leaves' .grad to its own gradient buffer)
            frame = FrameGraph(params, cams, grids, skies, targets, factors=(4, 4, 2), img_indices=list(range(len(cams))),
                               antialiased=m == "antialiased")
            for _ in range(args.warmup):
                assert frame.step() is True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                frame.step()
            torch.cuda.synchronize()
            times[m].append((time.perf_counter() - t0) / args.steps * 1e3)
            assert frame.valid()
            del frame
    med = {m: sorted(t)[len(t) // 2] for m, t in times.items()}
    res = dict(gaussians=args.gaussians, width=args.width, height=args.height, views=len(cams), steps=args.steps, rounds=args.rounds,
               ms_per_frame={m: round(v, 4) for m, v in med.items()}, ms_per_frame_all={m: [round(x, 4) for x in t] for m, t in times.items()})
    if len(modes) == 2:
        d = med["antialiased"] - med["classic"]
        res.update(antialiased_minus_classic_ms=round(d, 4), antialiased_over_classic_pct=round(100.0 * d / med["classic"], 3))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
