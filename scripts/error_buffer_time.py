#!/usr/bin/env python3
"""Times the error-driven image sampler (bilateral_driving_amd/sampler.py) on the MI355X at 135 x 240 (the shipped 1080p / 8) and
1080 x 1920, each with B = 1 and B = 200 views, in three measurements:

  kernel_vs_framework   ``bds_error_maps`` over B device-resident views against the same expression as framework ops on the device
                        (clamp, subtract, abs, mean over the channels, the masked multiplication by 5, the scatter into the map buffer,
                        mean / amin / amax per view).  Device events around windows of back-to-back calls; outputs compared first.
  sweep_vs_host_path    the streaming form (B calls of one view each and the one read-back of the statistics) against the reference's
                        host path for the same B views: per view ``clamp`` and ``squeeze().cpu().numpy()`` of the render, the ground
                        truth and the dynamic opacity, then ``np.stack``, ``torch.from_numpy``, the expression on the host, ``.to(device)``
                        and the per-image mean.  The reference is not importable where this runs: the host path was WRITTEN FROM THE OP
                        SEQUENCE of render_images and update_image_error_maps, in this script's own structure.  Host clock around work
                        that ends in a synchronise.
  draw                  per training step, ``propose_training_image`` in the reference's form (gather, ``error_weight`` rebuilt on the
                        host and uploaded, multiply, ``torch.multinomial(...).item()``) against the table draw, for 6 cameras x 200
                        frames and ``start_enhance_weight`` 3.  Host clock, windows of 200 steps.

Every timed step runs in a child process of its own under ``timeout``; the first step that fails ends the run.  Each form is warmed up,
then timed in repeated windows; the median window is reported with the fastest and the slowest.

    python scripts/error_buffer_time.py [--out profiles/error_buffer_time.json]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((135, 240), (1080, 1920))
BATCHES = (1, 200)
CAMS, FRAMES, WEIGHT = 6, 200, 3
NUM_IMGS = CAMS * FRAMES
LIMITS = {"kernel_vs_framework": 150, "sweep_vs_host_path": 300, "draw": 120}      # seconds per step


def stats_of(ms, calls):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "windows": len(ms), "calls_per_window": calls}


def event_ms(torch, fn, reps, warm, calls):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / calls)
    return stats_of(ms, calls)


def wall_ms(torch, fn, reps, warm, calls):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return stats_of(ms, calls)


def views(torch, B, h, w):
    g = torch.Generator(device="cuda").manual_seed(B * 7 + h)
    pred = torch.rand(B, h, w, 3, device="cuda", generator=g) * 1.5 - 0.2
    gt = torch.rand(B, h, w, 3, device="cuda", generator=g)
    dyn = torch.rand(B, h, w, device="cuda", generator=g) * 0.2
    return pred, gt, dyn


def kernel_vs_framework(B, h, w):
    import torch
    from bilateral_driving_amd import sampler as S
    pred, gt, dyn = views(torch, B, h, w)
    slots = torch.randperm(B, device="cuda")
    ids = torch.randperm(B, device="cuda")
    maps_a, stats_a = torch.zeros(B, h, w, device="cuda"), torch.zeros(B, 3, device="cuda")
    maps_b, stats_b = torch.zeros(B, h, w, device="cuda"), torch.zeros(B, 3, device="cuda")
    box = {"ws": None}

    def kernel():
        box["ws"] = S.error_maps(pred, gt, dyn, maps_a, slots, stats_a, ids, box["ws"])

    def framework():
        e = torch.abs(gt - pred.clamp(0., 1.)).mean(dim=-1)
        e[dyn > 0.1] *= 5
        maps_b[slots] = e
        stats_b[ids] = torch.stack([e.mean(dim=(1, 2)), e.amin(dim=(1, 2)), e.amax(dim=(1, 2))], dim=1)
    kernel()
    framework()
    torch.cuda.synchronize()
    mean_gap = float(((stats_a[:, 0].double() - stats_b[:, 0].double()).abs() / stats_b[:, 0].double()).max())
    same = {"maps": "bit-equal" if torch.equal(maps_a, maps_b) else float((maps_a - maps_b).abs().max()),
            "min_max": "bit-equal" if torch.equal(stats_a[:, 1:], stats_b[:, 1:]) else float((stats_a[:, 1:] - stats_b[:, 1:]).abs().max()),
            "mean_largest_relative_difference": mean_gap}
    calls = 50 if B * h * w < 10 ** 7 else 5
    res = {"outputs_kernel_vs_framework": same, "bytes_moved": 32 * B * h * w}
    for _ in range(2):      # alternating, the later pass is reported
        res["kernel_ms"] = event_ms(torch, kernel, 20, 3, calls)
        res["framework_ms"] = event_ms(torch, framework, 20, 3, calls)
    res["TB_per_s_kernel"] = res["bytes_moved"] / (res["kernel_ms"]["median"] * 1e-3) / 1e12
    res["framework_over_kernel"] = res["framework_ms"]["median"] / res["kernel_ms"]["median"]
    return res


def sweep_vs_host_path(B, h, w):
    import numpy as np
    import torch
    from bilateral_driving_amd import sampler as S
    pred, gt, dyn = views(torch, B, h, w)
    per_view = [(pred[b], gt[b], dyn[b][..., None]) for b in range(B)]
    frame = [torch.full((1,), b, dtype=torch.int64, device="cuda") for b in range(B)]
    maps, stats = torch.zeros(B, h, w, device="cuda"), torch.zeros(B, 3, device="cuda")
    box = {"ws": None}

    def sweep():
        for b, (p, g, d) in enumerate(per_view):
            box["ws"] = S.error_maps(p[None], g[None], d.reshape(1, h, w), maps, frame[b], stats, frame[b], box["ws"])
        return stats.cpu()

    def host_path():
        rgbs, gts, dyns = [], [], []
        for p, g, d in per_view:                                   # render_images: one view at a time
            rgbs.append(p.clamp(0., 1.).squeeze().cpu().numpy())
            gts.append(g.squeeze().cpu().numpy())
            dyns.append(d.squeeze().cpu().numpy())
        g_, p_ = torch.from_numpy(np.stack(gts, axis=0)), torch.from_numpy(np.stack(rgbs, axis=0))      # update_image_error_maps
        e = torch.abs(g_ - p_).mean(dim=-1)
        e[torch.from_numpy(np.stack(dyns, axis=0)) > 0.1] *= 5
        e = e.to("cuda")
        return e, e.mean(dim=(1, 2))
    got = sweep()
    e, mean = host_path()
    torch.cuda.synchronize()
    same = {"maps": "bit-equal" if torch.equal(maps, e) else float((maps - e).abs().max()),
            "mean_largest_relative_difference": float(((got[:, 0].double() - mean.cpu().double()).abs() / mean.cpu().double()).max())}
    big = B * h * w >= 10 ** 7
    res = {"outputs_sweep_vs_host_path": same}
    for _ in range(1 if big else 2):
        res["sweep_ms"] = wall_ms(torch, sweep, 5 if big else 10, 1, 1 if B > 1 else 20)
        res["host_path_ms"] = wall_ms(torch, host_path, 3 if big else 10, 1, 1 if B > 1 else 20)
    res["host_path_over_sweep"] = res["host_path_ms"]["median"] / res["sweep_ms"]["median"]
    return res


def draw():
    import numpy as np
    import torch
    from bilateral_driving_amd import sampler as S
    num_imgs = NUM_IMGS

    class Sampler(dict):
        __getattr__ = dict.__getitem__

    class Source:
        num_cams, num_imgs, device, buffer_ratio, image_error_buffered = CAMS, NUM_IMGS, torch.device("cuda"), 1.0, True
        data_cfg = type("Cfg", (), {"sampler": Sampler(buffer_ratio=1.0, start_enhance_weight=WEIGHT)})()
    source = Source()
    source.image_error_buffer = (torch.rand(num_imgs, generator=torch.Generator().manual_seed(1)) * 0.1 + 0.01).cuda()
    cands = list(range(num_imgs))

    def reference_form():
        self, candidate_indices = source, cands
        if random.random() < self.buffer_ratio and self.image_error_buffered:
            image_mean_error = self.image_error_buffer[candidate_indices]
            start_enhance_weight = self.data_cfg.sampler.get('start_enhance_weight', 1)
            if start_enhance_weight > 1:
                frame_num = int(self.num_imgs / self.num_cams)
                error_weight = torch.cat((torch.linspace(start_enhance_weight, 1, int(frame_num * 0.1)), torch.ones(frame_num - int(frame_num * 0.1))))
                error_weight = error_weight[..., None].repeat(1, self.num_cams).reshape(-1)
                error_weight = error_weight[candidate_indices].to(self.device)
                image_mean_error = image_mean_error * error_weight
            return candidate_indices[torch.multinomial(image_mean_error, 1, replacement=False).item()]
        return random.choice(candidate_indices)

    def table_form():
        return S.propose_training_image(source, cands)
    # the two forms draw from one distribution: frequencies over 20000 draws each against the weights' shares
    table = S.draw_table(source, cands)
    share = table.weights / table.total
    n = 20000
    freq = {name: np.bincount([fn() for _ in range(n)], minlength=num_imgs) / n for name, fn in (("reference", reference_form), ("table", table_form))}
    res = {"candidates": num_imgs, "start_enhance_weight": WEIGHT,
           "total_variation_from_the_weights_20000_draws": {k: float(0.5 * np.abs(v - share).sum()) for k, v in freq.items()}}
    for _ in range(2):
        res["table_ms_per_step"] = wall_ms(torch, table_form, 20, 2, 200)
        res["reference_ms_per_step"] = wall_ms(torch, reference_form, 20, 2, 200)
    res["reference_over_table"] = res["reference_ms_per_step"]["median"] / res["table_ms_per_step"]["median"]
    return res


STEPS = {"kernel_vs_framework": kernel_vs_framework, "sweep_vs_host_path": sweep_vs_host_path, "draw": draw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_buffer_time.json"))
    ap.add_argument("--step")
    ap.add_argument("--shape", type=int, nargs=3, metavar=("B", "h", "w"))
    ap.add_argument("--result")
    a = ap.parse_args()
    if a.step:                       # a child: one timed step, its result to a file
        import torch
        assert torch.cuda.is_available(), "the timings need the MI355X"
        res = STEPS[a.step](*(a.shape or ()))
        res["device"] = torch.cuda.get_device_name(0)
        with open(a.result, "w") as f:
            json.dump(res, f)
        return
    out = {"clock": {"kernel_vs_framework": "device events around a window of back-to-back calls, ms per call",
                     "sweep_vs_host_path": "host clock around a window that ends in a synchronise, ms per B views",
                     "draw": "host clock, ms per training step"}}
    jobs = [(step, (B, h, w)) for step in ("kernel_vs_framework", "sweep_vs_host_path") for h, w in SIZES for B in BATCHES] + [("draw", None)]
    with tempfile.TemporaryDirectory() as tmp:
        for step, shape in jobs:
            path = os.path.join(tmp, "result.json")
            cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--result", path]
            if shape:
                cmd += ["--shape", *map(str, shape)]
            label = step if shape is None else f"{step} {shape[1]}x{shape[2]} B={shape[0]}"
            print(f"[time] {label}", flush=True)
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(f"{label} ended with status {rc}: nothing more is started")
            with open(path) as f:
                res = json.load(f)
            out["device"] = res.pop("device")
            if shape is None:
                out[step] = res
            else:
                out.setdefault(step, {})[f"{shape[1]}x{shape[2]}_B{shape[0]}"] = res
            print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
