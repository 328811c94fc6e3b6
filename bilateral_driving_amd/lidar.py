"""Lidar scene preparation on the device (csrc/lidar.hip through ``bds_lidar_project``, ``bds_lidar_visible``,
``bds_lidar_points_in_boxes*`` and ``bds_lidar_depth_downsample``): the sparse depth maps, the cloud's colours and visibility, the
instances' points in their box frames, the background seed without them, and the depth map's downsampler.

Reference: ``DrivingDataset`` (datasets/driving_dataset.py) makes all of this before step 0 -- ``project_lidar_pts_on_images``
(:644-727), ``get_init_objects`` (:280-416), ``filter_pts_in_boxes`` (:496-574), ``check_pts_visibility`` (:576-603) -- as Python loops
over frames x instances with a ``torch.inverse`` each, and ``sparse_lidar_map_downsampler`` (datasets/base/pixel_source.py:77-92) runs
in every step of the coarse-to-fine schedule.

* ``project_points(points, lidar2img, ranges, W, H, images=None)`` -> ``depth, winner, pix, visible, colors``.
* ``visible_from(points, lidar2img, sizes)`` -> bool [N].
* ``points_in_boxes(points, poses, sizes, active, frame_ranges=None, emit=False)``: the mask form (bool [N]) or the emit form (the
  records ordered by (instance, frame, row)).
* ``downsample_sparse_depth(depth_map, factor)``.
* the reference's methods under their names, taking the dataset as the first argument: ``project_lidar_pts_on_images``,
  ``get_init_objects``, ``filter_pts_in_boxes``, ``check_pts_visibility``, and ``sparse_lidar_map_downsampler``;
  ``install(DrivingDataset, pixel_source_module)`` sets them on the reference's class and module, ``uninstall`` puts the former back.

The winner rule.  Where several points of a sweep land in one pixel the reference writes them with ``index_put_`` on duplicate
indices: on the host the last write -- the highest row -- wins, on a GPU the result is unspecified.  Here the highest row wins,
always; the winner map is an output.  Two frames of a camera that take the same sweep colour a point from the later frame, a point
that several cameras see takes the last camera's colour, as the reference's loop order gives: one launch per camera on one stream,
and inside a launch a point keeps the last view that sees it (so frames that share a sweep need no launch of their own).

Deviations: the divisions of the downsampler are taken in the order torch takes them on the host (sum / kh / kw); the matrices
(``pad(K) @ inverse(c2w)``, ``inverse(o2w)``) are formed on the host in float32 -- per frame as the reference for the cameras, one
batched inverse over the ACTIVE boxes for the poses (an inactive box's pose is never inverted) -- and uploaded; a camera or pose
tensor that lives on the device is copied to the host for that (``get_init_objects`` also reads the poses' translations there for the
``only_moving`` filter).  A camera's images are passed as they lie when they are float32 on the device; otherwise the stack of a
camera's frames is converted and uploaded in one piece.

Read-backs: the error flag of the finiteness check (every entry point), the emit form's record total (``points_in_boxes(emit=True)``,
``get_init_objects``) and, in ``get_init_objects`` alone, the per-instance counts that it returns as Python ints.  Everything else is
enqueued on the current stream without a host wait.

``cam.undistort``: ``project_lidar_pts_on_images`` here refuses it (NotImplementedError); ``undistort.project_lidar_pts_on_images``
runs the same sequence with the optimal new camera matrix and is what ``undistort.install`` sets after ``lidar.install``.

Not covered: ``get_init_smpl_objects``, dataset file loading, novel-view
trajectories, ``seg_dynamic_instances_in_lidar_frame``."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam

VIEW_CHUNK = 64             # include/bds.h BDS_LIDAR_VIEW_CHUNK: views per LDS stage
BOX_CHUNK = 128             # include/bds.h BDS_LIDAR_BOX_CHUNK: boxes per LDS stage
MAX_ROWS = 2 ** 31 - 257    # include/bds.h: rows, pixels and records are 32-bit
RIGID_NODES, SMPL_NODES, DEFORMABLE_NODES = 0, 1, 2      # datasets/base/scene_dataset.py:16-19 ModelType


def _cloud(points: Tensor, what: str = "points", check: bool = True) -> Tensor:
    """[N,3] -> contiguous float32 on the device, every coordinate finite.  One read-back (the flag word of ``bds_nonfinite_flags``);
    ``check=False``: a cloud that this module has already checked."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what} must be [N,3], got {tuple(points.shape)}")
    if points.shape[0] > MAX_ROWS:
        raise ValueError(f"{what} holds {points.shape[0]} rows, more than {MAX_ROWS}")
    L.require_gpu(points)
    x = points.detach().float().contiguous()
    if check and x.numel():
        flags = torch.zeros(1, dtype=torch.int32, device=x.device)
        ptrs = (L.C.c_void_p * 1)(x.data_ptr())
        cnts = (L.C.c_int64 * 1)(x.numel())
        L.check(L.lib().bds_nonfinite_flags(1, ptrs, cnts, None, flags.data_ptr(), None, L.stream()), "bds_nonfinite_flags")
        if int(flags.item()):
            raise ValueError(f"{what} contains NaN or infinity")
    return x


def _mats(m: Tensor, device, what: str) -> Tensor:
    """[V,3,4] or [V,4,4] (the first three rows are taken) -> contiguous float32 [V,3,4] on ``device``."""
    if m.dim() != 3 or m.shape[1] not in (3, 4) or m.shape[2] != 4:
        raise ValueError(f"{what} must be [V,3,4] or [V,4,4], got {tuple(m.shape)}")
    return m.detach()[:, :3, :].float().to(device).contiguous()


@torch.no_grad()
def project_points(points: Tensor, lidar2img: Tensor, ranges: Tensor, W: int, H: int, images: Optional[Tensor] = None,
                   visible: Optional[Tensor] = None, colors: Optional[Tensor] = None, _checked: bool = False):
    """``points`` [N,3] on the device; ``lidar2img`` [V,3,4] (or [V,4,4]) of V views of ONE camera, ``pad(K) @ inverse(c2w)`` in
    float32; ``ranges`` [V,2] int64: the rows [begin, end) of the cloud that view v takes; ``images`` [V,H,W,3] float32 or None.
    Returns ``depth`` [V,H,W] float32 (0 where no point landed), ``winner`` [V,H,W] int32 (the highest valid row of the pixel, -1
    where none), ``pix`` [N] int32 (the linear index into [V,H,W] of the point's pixel in the last view that sees it, else -1),
    ``visible`` [N] bool and ``colors`` [N,3] (None without images): the image's pixel for every valid point, winner or not.
    ``visible`` (uint8 [N]) / ``colors`` (float32 [N,3]) given: updated in place -- a launch only sets the rows it sees, so successive
    cameras accumulate, the later one winning -- and returned as they are.  ValueError for a NaN / Inf coordinate; BdsError for a CPU
    tensor.  One read-back: the error flag."""
    W, H = int(W), int(H)
    x = _cloud(points, check=not _checked)
    N, dev = x.shape[0], x.device
    M = _mats(lidar2img, dev, "lidar2img")
    V = M.shape[0]
    if W < 1 or H < 1 or V * H * W > MAX_ROWS:
        raise ValueError(f"views must be at least 1x1 with V*H*W <= {MAX_ROWS}, got V={V}, W={W}, H={H}")
    r = torch.as_tensor(ranges).to(device=dev, dtype=torch.int64).contiguous()
    if tuple(r.shape) != (V, 2):
        raise ValueError(f"ranges must be [V,2] = {(V, 2)}, got {tuple(r.shape)}")
    if images is not None:
        if tuple(images.shape) != (V, H, W, 3):
            raise ValueError(f"images must be [V,H,W,3] = {(V, H, W, 3)}, got {tuple(images.shape)}")
        images = images.detach().float().contiguous()
    own_visible = visible is None
    if own_visible:
        visible = torch.zeros(N, dtype=torch.uint8, device=dev)
    elif visible.dtype != torch.uint8 or tuple(visible.shape) != (N,):
        raise ValueError("visible must be uint8 [N]")
    if images is None:
        colors = None
    elif colors is None:
        colors = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    elif colors.dtype != torch.float32 or tuple(colors.shape) != (N, 3):
        raise ValueError("colors must be float32 [N,3]")
    L.require_gpu(x, M, r, images, visible, colors)
    depth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    winner = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    pix = torch.empty(N, dtype=torch.int32, device=dev)
    L.check(L.lib().bds_lidar_project(V, W, H, N, L.ptr(x), L.ptr(M), L.ptr(r), L.ptr(images), L.ptr(winner), L.ptr(depth), L.ptr(pix),
                                      L.ptr(visible), L.ptr(colors), L.stream()), "bds_lidar_project")
    return depth, winner, pix, (visible.bool() if own_visible else visible), colors


@torch.no_grad()
def visible_from(points: Tensor, lidar2img: Tensor, sizes) -> Tensor:
    """bool [N]: the points that any of the V views sees.  ``lidar2img`` [V,3,4] (or [V,4,4]); ``sizes``: [V,2] (W, H) per view, or one
    (W, H) pair for all.  One read-back: the error flag."""
    x = _cloud(points)
    M = _mats(lidar2img, x.device, "lidar2img")
    V = M.shape[0]
    s = torch.as_tensor(sizes, dtype=torch.int32)
    if s.dim() == 1:
        s = s[None].expand(V, 2)
    if tuple(s.shape) != (V, 2):
        raise ValueError(f"sizes must be (W, H) or [V,2], got {tuple(s.shape)}")
    s = s.to(x.device).contiguous()
    out = torch.empty(x.shape[0], dtype=torch.uint8, device=x.device)
    L.check(L.lib().bds_lidar_visible(x.shape[0], L.ptr(x), V, L.ptr(M), L.ptr(s), L.ptr(out), L.stream()), "bds_lidar_visible")
    return out.bool()


def box_tables(poses: Tensor, sizes: Tensor, active: Tensor, instances=None):
    """The active boxes' tables, formed on the host in float32: (``w2o`` [B,3,4] -- one batched inverse of the active poses only --,
    ``half`` [B,3] = size / 2, ``ids`` [B,2] int32 = (instance, frame)), in (frame, instance) order.  ``poses`` [F,I,4,4], ``sizes``
    [I,3], ``active`` [F,I] bool; ``instances``: restrict to these instance ids."""
    poses, sizes, active = poses.detach().cpu().float(), sizes.detach().cpu().float(), active.detach().cpu().bool()
    if poses.dim() != 4 or tuple(poses.shape[2:]) != (4, 4) or tuple(active.shape) != tuple(poses.shape[:2]) or \
            tuple(sizes.shape) != (poses.shape[1], 3):
        raise ValueError(f"poses [F,I,4,4], sizes [I,3], active [F,I]: got {tuple(poses.shape)}, {tuple(sizes.shape)}, {tuple(active.shape)}")
    if instances is not None:
        keep = torch.zeros(poses.shape[1], dtype=torch.bool)
        keep[torch.as_tensor(list(instances), dtype=torch.int64)] = True
        active = active & keep[None]
    f, i = torch.nonzero(active, as_tuple=True)
    w2o = torch.linalg.inv(poses[f, i])[:, :3, :].contiguous() if len(f) else torch.zeros(0, 3, 4)
    return w2o, (sizes / 2)[i].contiguous(), torch.stack([i, f], dim=1).int().contiguous()


@torch.no_grad()
def points_in_boxes(points: Tensor, poses: Tensor, sizes: Tensor, active: Tensor, frame_ranges: Optional[Tensor] = None,
                    emit: bool = False, instances=None, chunk: int = BOX_CHUNK, _checked: bool = False):
    """``points`` [N,3] on the device against the oriented boxes of the active (frame, instance) pairs: ``poses`` [F,I,4,4] (object to
    world), ``sizes`` [I,3], ``active`` [F,I] bool.  A point is inside when ``-size/2 < o < size/2`` holds strictly on every axis for
    ``o = inverse(pose) [p;1]``.  ``frame_ranges`` [F,2] int64 or None: the rows [begin, end) that the boxes of frame f test (its
    sweep); None: every row.  ``instances``: only these instance ids.  ``chunk``: boxes per LDS stage (tests lower it).

    Mask form (``emit=False``): bool [N], the OR over the boxes (filter_pts_in_boxes).  Read-back: the error flag.

    Emit form (``emit=True``): a dict of the M records ordered by (instance, frame, row) -- ``instance``, ``frame``, ``row`` int64 [M]
    and ``xyz`` float32 [M,3], the point in the box's frame (get_init_objects' concatenation order; a point inside two boxes appears
    in both).  Read-backs: the error flag and the record total."""
    x = _cloud(points, check=not _checked)
    N, dev = x.shape[0], x.device
    if not isinstance(chunk, int) or not 1 <= chunk <= BOX_CHUNK:
        raise ValueError(f"chunk must be an integer in 1..{BOX_CHUNK}, got {chunk!r}")
    w2o, half, ids = box_tables(poses, sizes, active, instances)
    B = w2o.shape[0]
    ranges = None
    if frame_ranges is not None:
        fr = torch.as_tensor(frame_ranges).to(device=dev, dtype=torch.int64)
        if tuple(fr.shape) != (poses.shape[0], 2):
            raise ValueError(f"frame_ranges must be [F,2] = {(poses.shape[0], 2)}, got {tuple(fr.shape)}")
        ranges = fr[ids[:, 1].long().to(dev)].contiguous()
    w2o, half, ids = w2o.to(dev), half.to(dev), ids.to(dev)
    lib = L.lib()
    if not emit:
        inside = torch.zeros(N, dtype=torch.uint8, device=dev)
        L.check(lib.bds_lidar_points_in_boxes(N, L.ptr(x), B, L.ptr(w2o), L.ptr(half), L.ptr(ranges), chunk, L.ptr(inside), L.stream()),
                "bds_lidar_points_in_boxes")
        return inside.bool()
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.bds_lidar_boxes_workspace_bytes(N)), 16), dtype=torch.uint8, device=dev)
    L.check(lib.bds_lidar_points_in_boxes_count(N, L.ptr(x), B, L.ptr(w2o), L.ptr(half), L.ptr(ranges), chunk, L.ptr(total), L.ptr(ws),
                                                ws.numel(), L.stream()), "bds_lidar_points_in_boxes_count")
    M = int(total.item()) if N and B else 0
    if M > MAX_ROWS:
        raise ValueError(f"{M} records, more than {MAX_ROWS}")
    rec_ids = torch.empty(M, 3, dtype=torch.int32, device=dev)
    rec_xyz = torch.empty(M, 3, dtype=torch.float32, device=dev)
    L.check(lib.bds_lidar_points_in_boxes_emit(N, L.ptr(x), B, L.ptr(w2o), L.ptr(half), L.ptr(ranges), L.ptr(ids), chunk, L.ptr(ws),
                                               ws.numel(), M, L.ptr(rec_ids), L.ptr(rec_xyz), L.stream()), "bds_lidar_points_in_boxes_emit")
    rec = rec_ids.long()
    # the kernel's order is (row, box); a stable sort by (instance, frame) leaves the rows ascending inside each pair
    order = torch.sort(rec[:, 0] * max(int(poses.shape[0]), 1) + rec[:, 1], stable=True).indices
    rec = rec[order]
    return {"instance": rec[:, 0], "frame": rec[:, 1], "row": rec[:, 2], "xyz": rec_xyz[order]}


def output_size(H: int, W: int, factor: float) -> Tuple[int, int]:
    """floor(H * factor), floor(W * factor): the size F.interpolate(scale_factor=factor) gives."""
    return int(math.floor(float(H) * factor)), int(math.floor(float(W) * factor))


@torch.no_grad()
def downsample_sparse_depth(depth_map: Tensor, factor: float) -> Tensor:
    """pixel_source.py:77-92 for ``depth_map`` [H,W] or [B,H,W] float32 on the device: the area-mean of the window's values over the
    area-mean of its hits (values > 1e-3), 0 where the window has no hit; output [.., floor(H factor), floor(W factor)].  Any
    ``factor`` > 0, as ``F.interpolate(mode="area")`` takes it (above 1 the windows are single pixels or overlap).  No read-back."""
    if depth_map.dim() not in (2, 3):
        raise ValueError(f"depth_map must be [H,W] or [B,H,W], got {tuple(depth_map.shape)}")
    factor = float(factor)
    if not (factor > 0.0 and math.isfinite(factor)):
        raise ValueError(f"factor must be positive and finite, got {factor!r}")
    L.require_gpu(depth_map)
    d = depth_map.detach().float().contiguous()
    batched = d if d.dim() == 3 else d[None]
    B, H, W = batched.shape
    if H < 1 or W < 1 or B * H * W > MAX_ROWS:
        raise ValueError(f"depth_map must hold 1..{MAX_ROWS} values, got {tuple(depth_map.shape)}")
    Ho, Wo = output_size(H, W, factor)
    if B * Ho * Wo > MAX_ROWS:
        raise ValueError(f"the output would hold {B * Ho * Wo} values, more than {MAX_ROWS}")
    out = torch.empty(B, Ho, Wo, dtype=torch.float32, device=d.device)
    L.check(L.lib().bds_lidar_depth_downsample(B, H, W, Ho, Wo, L.ptr(batched), L.ptr(out), L.stream()), "bds_lidar_depth_downsample")
    return out if d.dim() == 3 else out[0]


def sparse_lidar_map_downsampler(lidar_depth_map: Tensor, downscale_factor: float) -> Tensor:
    """pixel_source.py:77-92 under its name."""
    return downsample_sparse_depth(lidar_depth_map, downscale_factor)


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's methods, on any object with the attributes they read
# ----------------------------------------------------------------------------------------------------------------------------------
def _device(dataset) -> torch.device:
    dev = torch.device(getattr(dataset, "device", "cuda"))
    return torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev


def group_by_timestep(timesteps: Tensor, num_timesteps: int) -> Tuple[Tensor, Tensor]:
    """(``perm`` [N], ``offsets`` [T+1]) on the device: ``perm`` a stable sort of the rows by timestep (ties keep the row order; the
    identity for a cloud that is already grouped), rows ``offsets[t] .. offsets[t+1]`` of the sorted cloud are sweep t.  No read-back."""
    t = timesteps.long()
    ordered, perm = torch.sort(t, stable=True)
    offsets = torch.searchsorted(ordered, torch.arange(num_timesteps + 1, dtype=torch.int64, device=t.device))
    return perm, offsets


def _lidar_cloud(ls, dev) -> Tensor:
    return (ls.origins + ls.directions * ls.ranges).to(dev).float()


def camera_matrices(cam) -> Tensor:
    """[F,4,4] float32 on the host: ``pad(K) @ inverse(c2w)`` per frame, formed as the reference forms it (:681-685)."""
    out = []
    for f in range(len(cam)):
        K4 = torch.nn.functional.pad(cam.intrinsics[f].detach().cpu().float(), (0, 1, 0, 1))
        K4[3, 3] = 1.0
        out.append(K4 @ cam.cam_to_worlds[f].detach().cpu().float().inverse())
    return torch.stack(out) if out else torch.zeros(0, 4, 4)


@torch.no_grad()
def project_lidar_pts_on_images(dataset, delete_out_of_view_points: bool = True) -> None:
    """driving_dataset.py:644-727: every camera receives its sparse depth maps (``cam.load_depth`` of [F,H,W] float32), the lidar
    source its ``visible_masks`` and ``colors``; with ``delete_out_of_view_points`` the invisible points are then deleted.  One launch
    sequence per camera on the current stream.  Read-back: the error flag."""
    if any(getattr(cam, "undistort", False) for cam in dataset.pixel_source.camera_data.values()):
        raise NotImplementedError("cam.undistort needs getOptimalNewCameraMatrix: undistort.project_lidar_pts_on_images serves it "
                                  "(undistort.install, after lidar.install)")
    _project_on_images(dataset, delete_out_of_view_points, camera_matrices)


@torch.no_grad()
def _project_on_images(dataset, delete_out_of_view_points: bool, matrices) -> None:
    """``project_lidar_pts_on_images`` with ``matrices(cam)`` -> [F,4,4] forming a camera's lidar-to-image matrices."""
    ls, ps = dataset.lidar_source, dataset.pixel_source
    cams = list(ps.camera_data.values())
    dev = _device(dataset)
    cloud = _lidar_cloud(ls, dev)
    uniq = ls.unique_normalized_timestamps.to(dev)
    perm, offsets = group_by_timestep(ls.timesteps.to(dev), uniq.shape[0])
    x = _cloud(cloud[perm], "the lidar cloud")      # (checked once for all cameras)
    visible = ls.visible_masks.to(dev)[perm].to(torch.uint8)
    colors = ls.colors.to(dev).float()[perm].contiguous()
    for cam in cams:
        F = len(cam)
        closest = torch.argmin(torch.abs(uniq[None, :] - ps.normalized_time[:F].to(dev)[:, None]), dim=1)      # find_closest_timestep
        ranges = torch.stack([offsets[closest], offsets[closest + 1]], dim=1)
        depth = project_points(x, matrices(cam), ranges, cam.WIDTH, cam.HEIGHT, cam.images[:F].to(dev), visible, colors, _checked=True)[0]
        cam.load_depth(depth)
    vis = torch.empty_like(visible)
    vis[perm] = visible
    col = torch.empty_like(colors)
    col[perm] = colors
    ls.visible_masks = vis.bool().to(ls.visible_masks.device)
    ls.colors = col.to(device=ls.colors.device, dtype=ls.colors.dtype)
    if delete_out_of_view_points:
        ls.delete_invisible_pts()


@torch.no_grad()
def check_pts_visibility(dataset, pts_xyz: Tensor) -> Tensor:
    """driving_dataset.py:576-603: bool [N] on the dataset's device, the points that any frame of any camera sees.  One launch.
    Read-back: the error flag."""
    dev = _device(dataset)
    mats, sizes = [], []
    for cam in dataset.pixel_source.camera_data.values():
        mats.append(camera_matrices(cam))
        sizes += [(int(cam.WIDTH), int(cam.HEIGHT))] * len(cam)
    M = torch.cat(mats) if mats else torch.zeros(0, 4, 4)
    return visible_from(pts_xyz.to(dev), M, torch.tensor(sizes, dtype=torch.int32).reshape(-1, 2))


@torch.no_grad()
def get_init_objects(dataset, cur_node_type: str, instance_max_pts: int = 5000, only_moving: bool = True, traj_length_thres: float = 0.5,
                     exclude_smpl: bool = False) -> Dict[int, Dict[str, object]]:
    """driving_dataset.py:280-416: {instance id: {"node_type", "pts" [n,3] in the box's frame, "colors" [n,3], "num_pts", "poses",
    "size", "frame_info"}} for the instances of ``cur_node_type`` ("RigidNodes" / "DeformableNodes"), the points of all frames
    concatenated in frame order, sampled down to ``instance_max_pts`` with ``torch.randperm`` of the host generator in the reference's
    instance order, and, with ``only_moving``, without the instances whose trajectory is no longer than the threshold.  Read-backs:
    the error flag, the record total and the per-instance counts (returned as ints)."""
    if cur_node_type not in ("RigidNodes", "DeformableNodes"):
        raise ValueError(f"cur_node_type must be 'RigidNodes' or 'DeformableNodes', got {cur_node_type!r}")
    if exclude_smpl:
        assert cur_node_type == "DeformableNodes", "Only exclude SMPL for DeformableNodes"
    if getattr(dataset, "type", None) == "KITTI":
        traj_length_thres = 5.0
    ls, ps = dataset.lidar_source, dataset.pixel_source
    dev = _device(dataset)
    F, I = int(dataset.frame_num), int(dataset.instance_num)
    active = ps.per_frame_instance_mask.detach().cpu().bool()[:F, :I]
    types = ps.instances_model_types.detach().cpu().reshape(-1)[:I].long()
    wanted = (types == RIGID_NODES) if cur_node_type == "RigidNodes" else ((types == DEFORMABLE_NODES) | (types == SMPL_NODES))
    if exclude_smpl:
        humans = set(ps.smpl_human_all.keys())
        wanted = wanted & torch.tensor([int(t) not in humans for t in ps.instances_true_id.detach().cpu().reshape(-1)[:I].tolist()],
                                       dtype=torch.bool).reshape(-1)
    eligible = active & wanted[None]
    perm, offsets = group_by_timestep(ls.timesteps.to(dev), F)
    x = _lidar_cloud(ls, dev)[perm]
    frame_ranges = torch.stack([offsets[:-1], offsets[1:]], dim=1)
    rec = points_in_boxes(x, ps.instances_pose[:F, :I], ps.instances_size[:I], eligible, frame_ranges, emit=True)
    colors = ls.colors.to(dev)[perm][rec["row"]]
    counts = torch.bincount(rec["instance"], minlength=I).cpu().tolist() if I else []
    # the reference's dict order: by the first frame in which the instance is eligible, then by id
    el = eligible.numpy()
    keys = sorted((int(el[:, i].argmax()), i) for i in range(I) if el[:, i].any())
    out, start = {}, [0] * (I + 1)
    for i in range(I):
        start[i + 1] = start[i] + counts[i]
    for _, i in keys:
        pts, col, n = rec["xyz"][start[i]:start[i + 1]], colors[start[i]:start[i + 1]], counts[i]
        if n > instance_max_pts:
            sampled = torch.randperm(n)[:instance_max_pts].to(dev)
            pts, col, n = pts[sampled], col[sampled], instance_max_pts
        out[i] = {"node_type": cur_node_type, "pts": pts, "colors": col, "num_pts": n}
    if only_moving:
        trans_all = ps.instances_pose.detach().cpu()[:, :, :3, 3]      # (on the host: no wait per instance)
        mask_all = ps.per_frame_instance_mask.detach().cpu().bool()
        moving = {}
        for k, v in out.items():
            if v["num_pts"] > 0:
                trans = trans_all[:, k][mask_all[:, k]]
                if float(torch.norm(trans[1:] - trans[:-1], dim=-1).sum()) > traj_length_thres:
                    moving[k] = v
        out = moving
    for k, v in out.items():
        v["poses"] = ps.instances_pose[:, k]
        v["size"] = ps.instances_size[k]
        v["frame_info"] = ps.per_frame_instance_mask[:, k]
    return out


@torch.no_grad()
def filter_pts_in_boxes(dataset, seed_pts: Tensor, valid_instances_dict, seed_colors: Optional[Tensor] = None,
                        seed_time: Optional[Tensor] = None) -> Dict[str, Optional[Tensor]]:
    """driving_dataset.py:496-574: the seed points (and their colours and times) that lie in no box of the given instances at any
    frame in which they are active.  One launch over all (frame, instance) boxes.  Read-back: the error flag."""
    ps = dataset.pixel_source
    F = int(dataset.frame_num)
    inside = points_in_boxes(seed_pts, ps.instances_pose[:F], ps.instances_size, ps.per_frame_instance_mask[:F],
                             instances=list(valid_instances_dict.keys()))
    keep = ~inside
    return {"pts": seed_pts[keep], "colors": None if seed_colors is None else seed_colors[keep],
            "time": None if seed_time is None else seed_time[keep]}


_METHODS = {"project_lidar_pts_on_images": project_lidar_pts_on_images, "get_init_objects": get_init_objects,
            "filter_pts_in_boxes": filter_pts_in_boxes, "check_pts_visibility": check_pts_visibility}
_SEAM = Seam()


def install(dataset_class=None, pixel_source_module=None) -> None:
    """Sets the four methods on ``dataset_class`` (the reference's ``DrivingDataset``) and ``sparse_lidar_map_downsampler`` on
    ``pixel_source_module`` (``datasets.base.pixel_source``, whose ``get_image`` looks the name up at call time)."""
    for target, names in ((dataset_class, _METHODS), (pixel_source_module, {"sparse_lidar_map_downsampler": sparse_lidar_map_downsampler})):
        if target is not None:
            _SEAM.install(target, names)


def uninstall(*targets) -> None:
    """Puts back what ``install`` replaced (no target given: on every installed one)."""
    _SEAM.uninstall(*targets)
