#!/usr/bin/env python3
"""Times one evaluation video frame (bilateral_driving_amd/video.py) on the MI355X: 3 cameras of 1080 x 1920, keys ``rgbs``, ``depths``
and ``Dynamic_depths`` -- a 3 237 x 5 759 canvas of 9 panels -- in three ways:

  kernel      ``FrameComposer.frame``: one ``bds_video_frame`` launch over the device tensors.  Device events around windows of
              back-to-back calls.
  framework   the same expressions as framework ops on the same GPU: clamp, multiply, cast for the images; log, scale, clamp, multiply,
              index into the colour table for the depths; copies into a zeroed float32 canvas, the crop, ``torch.cat``, the quantiser.
              Device events likewise; the outputs are compared first (bit-equal outside the depth pixels, at most one table index inside).
  host_path   the reference's numpy path on this machine's host for the same frame: per view ``.cpu().numpy()`` of every array,
              ``-log``, the scaling and the colour-table lookup in float64, the layout's zeroed float32 canvas, the crop,
              ``np.concatenate`` and ``to8b``.  The reference is not importable where this runs: the path was WRITTEN FROM THE OP
              SEQUENCE of ``render``, ``visualize_cmap``, ``layout_waymo`` and ``save_concatenated_videos``, in this script's own
              structure, with matplotlib's ``turbo`` where that imports and a 256-entry float64 table lookup of the same cost otherwise.
              Host clock around work that ends with the frame on the host; the kernel's form is timed the same way (launch + ``.cpu()``).

For the kernel the algorithmic bytes (every source read once, 3 bytes per pixel written) and the share of the 6.3 TB/s that a float4
copy reaches on this chip are reported, and -- to say what bounds the launch -- the same canvas from images alone and from depths alone
(``per_kind``).  Each form is warmed up, then timed in repeated windows; the median
window is reported with the fastest and the slowest.

Every timed call reads another of ``--sets`` source sets (4 x 174 MB), so that no call finds its sources in the 256 MiB Infinity
Cache.  The event windows include the Python wrapper of each call; the kernel's own time comes from a run of its own under the
profiler, whose dispatches ``--parse-trace`` adds to the result:

    python scripts/video_time.py [--out profiles/video_time.json] [--height 1080 --width 1920]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o video -- python scripts/video_time.py --trace-run
    python scripts/video_time.py --parse-trace DIR [--out profiles/video_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMS = ["front_left_camera", "front_camera", "front_right_camera"]
KEYS = ["rgbs", "depths", "Dynamic_depths"]
# the frame, and the same canvas from images alone (12 + 3 bytes per pixel, no arithmetic to speak of) and from depths alone (8 + 3 bytes
# per pixel, one logf and one table lookup each)
VARIANTS = {"frame": KEYS, "rgbs_only": ["rgbs"] * 3, "depths_only": ["depths", "Dynamic_depths", "depths"]}
READ_PER_PIXEL = {"frame": 12 + 2 * 8, "rgbs_only": 3 * 12, "depths_only": 3 * 8}
COPY_TB_PER_S = 6.3
TRACE_WARM, TRACE_CALLS = 5, 50
KERNEL = "video_frame_kernel"


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


def wall_ms(torch, fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats_of(ms, 1)


def algorithmic_bytes(h, w):
    """Every source read once, 3 bytes per pixel of the cropped canvas written."""
    canvas = 3 * (3 * (h - 1)) * (3 * w - 1)
    return {name: h * w * len(CAMS) * read + canvas for name, read in READ_PER_PIXEL.items()}


def parse_trace(a):
    """The kernel's own times from a ``--trace-run`` under ``rocprofv3 --kernel-trace --output-format csv -d DIR``: per variant
    TRACE_WARM + TRACE_CALLS dispatches in VARIANTS' order, the first TRACE_WARM of each left out."""
    import csv
    import glob
    rows = [r for f in glob.glob(os.path.join(a.parse_trace, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
    spans = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if KERNEL in r["Kernel_Name"])
    per = TRACE_WARM + TRACE_CALLS
    assert len(spans) == per * len(VARIANTS), f"{len(spans)} dispatches of {KERNEL}, expected {per * len(VARIANTS)}"
    with open(a.out) as f:
        res = json.load(f)
    res["kernel_trace"] = {"clock": "rocprofv3 --kernel-trace: the dispatch's end minus its start, us", "calls": TRACE_CALLS}
    for k, name in enumerate(VARIANTS):
        us = [(e - s) / 1e3 for s, e in spans[k * per + TRACE_WARM:(k + 1) * per]]
        nbytes = algorithmic_bytes(a.height, a.width)[name]
        res["kernel_trace"][name] = {"us": {"median": statistics.median(us), "min": min(us), "max": max(us)}, "algorithmic_bytes": nbytes,
                                     "TB_per_s": nbytes / (statistics.median(us) * 1e-6) / 1e12,
                                     "share_of_float4_copy_rate": nbytes / (statistics.median(us) * 1e-6) / 1e12 / COPY_TB_PER_S}
    print(json.dumps(res["kernel_trace"]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_time.json"))
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--host-windows", type=int, default=3)
    ap.add_argument("--sets", type=int, default=4, help="source sets the calls rotate through: together beyond the 256 MiB Infinity Cache")
    ap.add_argument("--trace-run", action="store_true", help="only the launches, for a run under rocprofv3 --kernel-trace")
    ap.add_argument("--parse-trace", metavar="DIR", help="add the kernel times of such a run's *kernel_trace.csv under DIR to --out")
    a = ap.parse_args()
    if a.parse_trace:
        return parse_trace(a)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "the timings need the MI355X"
    from bilateral_driving_amd import video as V
    h, w = a.height, a.width
    g = torch.Generator(device="cuda").manual_seed(54)
    sets = []
    for _ in range(a.sets):
        one_set = {"cam_names": list(CAMS), "rgbs": [], "depths": [], "opacities": [], "Dynamic_depths": [], "Dynamic_opacities": []}
        for _ in CAMS:
            one_set["rgbs"].append(torch.rand(h, w, 3, device="cuda", generator=g) * 1.2 - 0.1)
            for k in ("depths", "Dynamic_depths"):
                one_set[k].append(torch.exp(torch.rand(h, w, device="cuda", generator=g) * 4.6 + 0.7))
            for k in ("opacities", "Dynamic_opacities"):
                one_set[k].append(torch.rand(h, w, device="cuda", generator=g))
        sets.append(one_set)
    rr = sets[0]                     # the set whose outputs are compared and that the host path shows
    turn = {"at": 0}

    def next_set():                  # every timed call reads another set: no call finds its sources in a cache
        turn["at"] += 1
        return sets[turn["at"] % len(sets)]
    composers = {name: V.FrameComposer("waymo", keys) for name, keys in VARIANTS.items()}

    def kernel():
        return composers["frame"].frame(next_set(), CAMS)
    if a.trace_run:
        for name in VARIANTS:
            for _ in range(TRACE_WARM + TRACE_CALLS):
                composers[name].frame(next_set(), CAMS)
            torch.cuda.synchronize()
        return

    # the colour table as the kernel holds it: the colours of exact table positions
    idx = torch.arange(256, device="cuda", dtype=torch.float32)
    s = (idx + 0.5) / 256
    lo, hi = -np.log(4.0 + 1e-6), -np.log(120 + 1e-6)
    depth_of = torch.exp(-(s.double() * abs(hi - lo) + min(lo, hi))).float() - 1e-6
    table8 = V.depth_visualizer(depth_of[None], None)[0]                       # [256,3] uint8
    table = table8.float() / 255 + 0.5 / 255                                   # a float table that quantises back to it

    def tile(frames):
        lh, lw = frames[1].shape[0], frames[1].shape[1]
        canvas = torch.zeros(lh, 5 * lw, 3, device="cuda")
        for c, f in enumerate(frames):
            canvas[:, (c + 1) * lw:(c + 2) * lw] = f
        return canvas[0:lh - 1, lw:4 * lw - 1]

    def colours(depth, opacity):
        v = -torch.log(depth + 1e-6)
        s_ = torch.nan_to_num(torch.clamp((v - float(np.float32(min(lo, hi)))) / float(np.float32(abs(hi - lo))), 0, 1)) * opacity
        return table[torch.clamp((s_ * 256).long(), 0, 255)]

    def framework(rr=None):
        rr = next_set() if rr is None else rr
        merged = [tile([f.clamp(0., 1.) for f in rr["rgbs"]])]
        for k, o in (("depths", "opacities"), ("Dynamic_depths", "Dynamic_opacities")):
            merged.append(tile([colours(d, op) for d, op in zip(rr[k], rr[o])]))
        return (255 * torch.clamp(torch.cat(merged, dim=0), 0, 1)).to(torch.uint8)

    try:
        import matplotlib
        cmap = matplotlib.colormaps["turbo"]
        cmap_name = "matplotlib turbo"
    except ImportError:
        lut = np.concatenate([table.double().cpu().numpy(), np.ones((256, 1))], axis=1)
        cmap_name = "256-entry float64 table lookup"

        def cmap(x):
            xa = np.array(x, copy=True)
            xa *= 256
            xa[xa < 0] = -1
            xa[xa == 256] = 255
            np.clip(xa, -1, 256, out=xa)
            return lut.take(np.clip(xa.astype(int), 0, 255), axis=0, mode="clip")

    def host_path():
        def get_numpy(x):
            return x.squeeze().cpu().numpy()
        lists = {k: [get_numpy(t.clamp(0., 1.) if k == "rgbs" else t) for t in rr[k]] for k in rr if k != "cam_names"}

        def visualize(value, weight):
            value = -np.log(value + 1e-6)
            value = np.nan_to_num(np.clip((value - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1))
            value *= weight
            return cmap(value)[..., :3]

        def layout(imgs):
            lh, lw = imgs[1].shape[0], imgs[1].shape[1]
            tiled = np.zeros((lh, 5 * lw, 3), dtype=np.float32)
            filled = np.zeros((lh, 5 * lw), dtype=np.uint8)
            for c, img in enumerate(imgs):
                tiled[:, (c + 1) * lw:(c + 2) * lw] = img
                filled[:, (c + 1) * lw:(c + 2) * lw] = 1
            ys, xs = np.where(filled)[0], np.where(filled)[1]
            return tiled[ys.min():ys.max(), xs.min():xs.max()]
        merged = [layout(lists["rgbs"])]
        for k, o in (("depths", "opacities"), ("Dynamic_depths", "Dynamic_opacities")):
            merged.append(layout([visualize(d, op) for d, op in zip(lists[k], lists[o])]))
        return (255 * np.clip(np.concatenate(merged, axis=0), 0, 1)).astype(np.uint8)

    def kernel_to_host():
        return composers["frame"].frame(rr, CAMS).cpu().numpy()

    got, ref = composers["frame"].frame(rr, CAMS), framework(rr)
    torch.cuda.synchronize()
    Hk = got.shape[0] // 3
    differ = (got != ref).any(dim=-1)
    step = (got[Hk:].int() - ref[Hk:].int()).abs().max()
    res = {"device": torch.cuda.get_device_name(0), "frame": list(got.shape), "panels": 9,
           "outputs_kernel_vs_framework": {"image_rows_bit_equal": bool(not differ[:Hk].any()), "depth_pixels_differing": int(differ[Hk:].sum()),
                                           "depth_pixels": int(differ[Hk:].numel()), "largest_channel_step": int(step)},
           "source_sets": len(sets),
           "clock": {"kernel_ms, framework_ms": "device events around a window of back-to-back calls (Python wrapper included), ms per frame",
                     "kernel_to_host_ms, host_path_ms": "host clock, the frame on the host at the end, ms per frame"},
           "host_colour_map": cmap_name}
    for _ in range(2):      # alternating, the later pass is reported
        res["kernel_ms"] = event_ms(torch, kernel, 20, 3, 100)
        res["framework_ms"] = event_ms(torch, framework, 10, 2, 3)
    res["kernel_to_host_ms"] = wall_ms(torch, kernel_to_host, 10, 2)
    res["host_path_ms"] = wall_ms(torch, host_path, a.host_windows, 1)
    res["algorithmic_bytes"] = algorithmic_bytes(h, w)["frame"]
    res["TB_per_s_kernel"] = res["algorithmic_bytes"] / (res["kernel_ms"]["median"] * 1e-3) / 1e12
    res["share_of_float4_copy_rate"] = res["TB_per_s_kernel"] / COPY_TB_PER_S
    # what bounds the launch: the same canvas from images alone and from depths alone
    res["per_kind"] = {}
    for name in ("rgbs_only", "depths_only"):
        ms = event_ms(torch, lambda: composers[name].frame(next_set(), CAMS), 20, 3, 100)
        nbytes = algorithmic_bytes(h, w)[name]
        res["per_kind"][name] = {"ms": ms, "algorithmic_bytes": nbytes, "TB_per_s": nbytes / (ms["median"] * 1e-3) / 1e12}
    res["framework_over_kernel"] = res["framework_ms"]["median"] / res["kernel_ms"]["median"]
    res["host_path_over_kernel_to_host"] = res["host_path_ms"]["median"] / res["kernel_to_host_ms"]["median"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
