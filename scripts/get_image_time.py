#!/usr/bin/env python3
"""Times one call of a view's input preparation at 1920 x 1080 in three forms, at the factors 1 and 0.5:

  (a) host       the reference's sequence of framework ops as it stands: int64 meshgrids and the four fills made on the host and
                 copied to the device, the rays as framework launches, F.interpolate for the image and the five masks, the area
                 resize of the depth.  The reference is not importable where this runs, so ``framework`` below was WRITTEN FROM THE
                 OP SEQUENCE of CameraData.get_image (which op, which dtype, created where), in this script's own structure;
  (b) device     the same expression with every tensor created on the device;
  (c) pixels     bilateral_driving_amd.pixels.get_image on a bare object.

Each form is warmed up, then timed in REPS windows of 50 back-to-back calls each, a host clock around the window and one device
synchronise at its end (form (a) has host work that device events would not see); the median window's time per call is reported.
Forms (b) and (c) are compared on their outputs before they are timed.

Also timed, with device events: ``bds_view_fields`` alone into preallocated outputs (the median of single launches, and of trains of
200), reported as bytes written (64 per pixel) over time against the HBM rates of the MI355X (8.0 TB/s specified, 6.0-6.3 TB/s
measured for plain streaming stores and copies).  The kernel's own time comes from a kernel trace, in a run of its own:

    python scripts/get_image_time.py [--out profiles/get_image_time.json] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/get_image_time.py --kernel-only 200"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bilateral_driving_amd import lidar, pixels      # noqa: E402

H, W = 1080, 1920
MASKS = ("sky_masks", "dynamic_masks", "human_masks", "vehicle_masks")
HBM_SPEC_TBS, HBM_STREAM_TBS = 8.0, 6.2
CALLS = 50      # calls per timed window: a window of (a) lasts 0.2 s, one of (c) 6 ms


class Camera:
    """What get_image reads of a CameraData: one frame's worth of tensors on the device, the per-frame scalars on the host."""

    def __init__(self, dev, factor):
        g = torch.Generator().manual_seed(0)
        self.images = torch.rand(1, H, W, 3, generator=g).to(dev)
        for k in MASKS:
            setattr(self, k, (torch.rand(1, H, W, generator=g) < 0.3).float().to(dev))
        self.egocar_mask = (torch.rand(H, W, generator=g) < 0.1).float().to(dev)
        self.lidar_depth_maps = (torch.rand(1, H, W, generator=g) * 60 * (torch.rand(1, H, W, generator=g) < 0.05)).to(dev)
        c2w = torch.eye(4)
        c2w[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
        c2w[:3, 3] = torch.tensor([212.0, -148.0, 3.0])
        self.cam_to_worlds = c2w[None].to(dev)
        self.intrinsics = torch.tensor([[[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1]]]).to(dev)
        self.normalized_time, self.unique_img_idx = torch.tensor([0.37]), torch.tensor([11])
        self.cam_id, self.cam_name, self.HEIGHT, self.WIDTH = 2, "front_camera", H, W
        self.downscale_factor, self.device = factor, dev


def _interp(t, s, mode, **kw):
    """F.interpolate of a [h,w] or [c,h,w] tensor by the factor ``s``."""
    t4 = t[None, None] if t.dim() == 2 else t[None]
    return F.interpolate(t4, scale_factor=s, mode=mode, **kw)[0]


def _resized_inputs(cam, frame, s):
    """The frame's image, masks and lidar map at the factor ``s``: one antialiased bicubic, five nearest and two area resizes."""
    rgb = cam.images[frame]
    planes = {k: getattr(cam, k)[frame] for k in MASKS}
    planes["egocar_mask"] = cam.egocar_mask
    depth = cam.lidar_depth_maps[frame]
    if s == 1.0:
        return rgb, planes, depth
    rgb = _interp(rgb.permute(2, 0, 1), s, "bicubic", antialias=True).permute(1, 2, 0)
    planes = {k: _interp(m, s, "nearest")[0] for k, m in planes.items()}
    mean, hits = _interp(depth, s, "area")[0], _interp((depth > 1e-3).float(), s, "area")[0]
    seen = hits > 0
    sparse = torch.zeros_like(mean)
    sparse[seen] = mean[seen] / hits[seen]
    return rgb, planes, sparse


def _pixel_grid(h, w, made, dev):
    """Flat int64 column and row numbers of an h x w image, made on ``made`` and moved to ``dev``."""
    cols, rows = torch.meshgrid(torch.arange(w, device=made), torch.arange(h, device=made), indexing="xy")
    return cols.flatten().to(dev), rows.flatten().to(dev)


def _rays(cols, rows, pose, K):
    """Pinhole rays through the pixel centres, rotated by the pose: a stack, a pad, a broadcast product with a sum, a norm, a division."""
    local = F.pad(torch.stack([(cols - K[0, 2] + 0.5) / K[0, 0], (rows - K[1, 2] + 0.5) / K[1, 1]], dim=-1), (0, 1), value=1.0)
    world = (local[:, None, :] * pose[None, :3, :3]).sum(dim=-1)
    length = torch.linalg.norm(world, dim=-1, keepdims=True)
    return torch.broadcast_to(pose[:3, -1], world.shape), world / (length + 1e-8), length


def framework(cam, frame, on_device):
    """One call as framework ops, written from the SEQUENCE of calls the reference makes -- which op, of which dtype, created where --
    so that launches, temporaries and copies match; the code is this script's own.  ``on_device``: grids and fills are created on
    the device instead of the host."""
    dev, s = cam.device, cam.downscale_factor
    made = dev if on_device else "cpu"
    rgb, planes, depth = _resized_inputs(cam, frame, s)
    h, w = (int(n) for n in rgb.shape[:2])
    cols, rows = _pixel_grid(h, w, made, dev)
    out = {"pixels": rgb, "lidar_depth_map": depth, **planes,
           "pixel_coords": torch.stack([rows / h, cols / w], dim=-1).float().reshape(h, w, 2)}
    for key, value, dtype in (("normed_time", float(cam.normalized_time[frame]), torch.float32), ("cam_id", cam.cam_id, torch.long),
                              ("img_idx", int(cam.unique_img_idx[frame]), torch.long), ("frame_idx", frame, torch.long)):
        out[key] = torch.full((h, w), value, dtype=dtype, device=made).to(dev)
    K = cam.intrinsics[frame] * s
    K[2, 2] = 1.0
    origins, viewdirs, length = _rays(cols, rows, cam.cam_to_worlds[frame], K)
    out.update(origins=origins.reshape(h, w, 3), viewdirs=viewdirs.reshape(h, w, 3), direction_norm=length.reshape(h, w, 1), intrinsics=K)
    return out


def wall_ms(fn, reps, warm=3, calls=CALLS):
    """ms per call: ``reps`` timed windows of ``calls`` back-to-back calls each, one synchronise at a window's end."""
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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "calls_per_window": calls}


def event_ms(fn, reps, warm=3, calls=1):
    """ms per call between two device events around ``calls`` back-to-back calls."""
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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "calls_per_window": calls}


def view_fields_entry(dev):
    """-> a function that launches bds_view_fields alone for one 1920 x 1080 view into preallocated outputs."""
    L, lib = pixels.L, pixels.L.lib()
    cam = Camera(dev, 1.0)
    c2w, K = cam.cam_to_worlds.contiguous(), cam.intrinsics.contiguous()
    ids, tm = torch.tensor([[11, 0, 2]], dtype=torch.int64, device=dev), torch.tensor([0.37], device=dev)
    f3, f3b, f1, f2, ft = (torch.empty(H, W, k, device=dev) for k in (3, 3, 1, 2, 1))
    i0, i1, i2 = (torch.empty(H, W, dtype=torch.int64, device=dev) for _ in range(3))
    ko = torch.empty(3, 3, device=dev)

    def entry():
        L.check(lib.bds_view_fields(1, H, W, L.ptr(c2w), L.ptr(K), 1, 1.0, L.ptr(tm), L.ptr(ids), L.ptr(f3), L.ptr(f3b), L.ptr(f1), L.ptr(f2),
                                    L.ptr(ft), L.ptr(i0), L.ptr(i1), L.ptr(i2), L.ptr(ko), L.stream()), "bds_view_fields")
    return entry


def compare(theirs, info, cams):
    """Forms (b) and (c) on the same inputs: bit-equal fields, and the largest difference of the others."""
    keys = {"sky_masks": "sky_masks", "dynamic_masks": "dynamic_masks", "human_masks": "human_masks", "vehicle_masks": "vehicle_masks",
            "egocar_mask": "egocar_masks"}
    mine = {**info, "cam_id": cams["cam_id"], "intrinsics": cams["intrinsics"]}
    res = {}
    for k, v in theirs.items():
        m = mine[keys.get(k, k)]
        assert tuple(m.shape) == tuple(v.shape), k
        res[k] = "bit-equal" if torch.equal(m, v.contiguous()) else float((m.double() - v.double()).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "get_image_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N",
                    help="launch bds_view_fields N times and exit: the program to run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("get_image_time.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    if a.kernel_only:
        entry = view_fields_entry(dev)
        for _ in range(a.kernel_only):
            entry()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "image": [H, W],
           "clock": f"host clock around {CALLS} calls and a synchronise, ms per call",
           "forms": {}, "outputs_b_vs_c": {}}
    for factor in (1.0, 0.5):
        cam = Camera(dev, factor)
        res["outputs_b_vs_c"][str(factor)] = compare(framework(cam, 0, True), *pixels.get_image(cam, 0))
        forms = {"a_host": lambda: framework(cam, 0, False), "b_device": lambda: framework(cam, 0, True), "c_pixels": lambda: pixels.get_image(cam, 0)}
        out = {k: None for k in forms}
        for _ in range(2):      # two rounds, the forms alternating; the later round is kept, the earlier shows the spread
            for k, fn in forms.items():
                r = wall_ms(fn, a.reps)
                out[k] = r if out[k] is None else {**r, "earlier_round_median": out[k]["median"]}
        res["forms"][str(factor)] = out
        if factor != 1.0:
            res["parts_ms_events"] = {
                "resize_image": event_ms(lambda: pixels.resize_image(cam.images[0], factor), a.reps, calls=CALLS),
                "resize_masks_5": event_ms(lambda: pixels.resize_masks([cam.egocar_mask] + [getattr(cam, k)[0] for k in MASKS], factor), a.reps, calls=CALLS),
                "lidar_downsample": event_ms(lambda: lidar.sparse_lidar_map_downsampler(cam.lidar_depth_maps[0], factor), a.reps, calls=CALLS),
                "torch_bicubic_aa": event_ms(lambda: F.interpolate(cam.images[0][None].permute(0, 3, 1, 2), scale_factor=factor, mode="bicubic",
                                                                   antialias=True), a.reps, calls=CALLS)}
    entry = view_fields_entry(dev)

    written = 64 * H * W + 36
    one, many = event_ms(entry, a.reps), event_ms(entry, a.reps, calls=200)
    per = many["median"]
    res["view_fields_alone"] = {"bytes_written": written, "single_launch_ms": one, "train_of_200_ms_per_launch": per,
                                "TB_per_s_single": written / (one["median"] * 1e-3) / 1e12, "TB_per_s_train": written / (per * 1e-3) / 1e12,
                                "share_of_streaming_rate_train": written / (per * 1e-3) / 1e12 / HBM_STREAM_TBS,
                                "share_of_specified_rate_train": written / (per * 1e-3) / 1e12 / HBM_SPEC_TBS,
                                "hbm_TB_per_s": {"specified": HBM_SPEC_TBS, "streaming_stores_measured": HBM_STREAM_TBS}}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
