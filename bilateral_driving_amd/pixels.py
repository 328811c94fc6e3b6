"""A view's input preparation on the device (csrc/pixels.hip through ``bds_view_fields``, ``bds_image_resize_aa`` and
``bds_masks_resize_nearest``): the rays, the per-pixel fields and the resized image and masks that the trainer and the evaluation
take for one frame of one camera.

Reference: ``CameraData.get_image`` (datasets/base/pixel_source.py:477-657, with ``get_rays`` :38-75) runs in front of every training
step (tools/train.py:257-264 through ``SplitWrapper.next``) and every evaluation render: int64 meshgrids and four full-size fills made
on the host and copied to the device, about a dozen framework launches for the rays, and, under the coarse-to-fine schedule, one
antialiased bicubic resize of the image and up to five nearest resizes of the masks.
``ScenePixelSource.prepare_novel_view_render_data`` (:1070-1132) does the same per pose of a novel trajectory.

* ``view_fields(c2w, intrinsics, H, W, *, scale=1.0, normed_time=None, img_idx, frame_idx, cam_id=None)`` -> dict: every per-pixel
  field of B views in ONE launch.
* ``resize_image(img, factor)``: ``F.interpolate(mode="bicubic", antialias=True)`` of an image [H,W,3].
* ``resize_masks(masks, factor)``: ``F.interpolate(mode="nearest")`` of up to five masks [H,W] in one launch.
* the reference's methods under their names, taking the object as the first argument: ``get_image(camera_data, frame_idx)`` and
  ``prepare_novel_view_render_data(pixel_source, dataset_type, traj)``; ``install(CameraData, ScenePixelSource)`` sets them on the
  reference's classes, ``uninstall`` puts the former back.  An object whose tensors live on the CPU keeps the class's own method.

Deviations.  Every tensor comes back on the device: the reference hands ``normed_time``, ``img_idx``, ``frame_idx`` and ``cam_id`` back on
the CPU and ``train.py`` moves them with ``.cuda()``, which is then a no-op.  The resized image is a contiguous [Ho,Wo,3] tensor; the
reference's is a permuted view of a [3,Ho,Wo] one with the same values.  The resize's weights are the ones of torch's host kernel in
float32; its sums run tap by tap without fused multiply-add, which may differ from torch's in the last bits (bounds: DESIGN.md).
A camera without images can only be asked for ``downscale_factor == 1`` (the reference fails there with an unbound name).

Read-backs: none.  Indices and times that are host values (Python numbers, CPU tensors: what the reference's ``CameraData`` holds) go
to the device in ONE small copy together with ``height`` and ``width``; the ones that are device tensors are stacked there (a
``frame_idx`` that is a device tensor still selects the frame's rows through torch's own indexing, which may wait for it).  Per call
``get_image`` is one launch at ``downscale_factor == 1``, and at most four (fields, image, masks, lidar map) otherwise.

``cam.undistort`` and the loaders that fill ``images`` and the masks live in ``undistort.py`` (``undistort.install``).  The error-map
buffer (``update_image_error_maps``, ``propose_training_image``) lives in ``sampler.py``."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from . import lidar
from ._patch import MISSING, Seam

MAX_MASKS = 5               # include/bds.h BDS_PIXELS_MAX_MASKS
MAX_VIEWS = 65535           # include/bds.h: the launch's second grid dimension
MAX_ROWS = lidar.MAX_ROWS   # flat pixels are 32-bit
MAX_SCALE = 512             # include/bds.h BDS_PIXELS_MAX_SCALE: resize_image takes factors down to 1 / 512


def _is_host(v) -> bool:
    return not (isinstance(v, Tensor) and v.is_cuda)


def _column(v, B: int, what: str) -> np.ndarray:
    a = np.asarray(v.detach().numpy() if isinstance(v, Tensor) else v).reshape(-1)
    if a.size not in (1, B):
        raise ValueError(f"{what} must hold 1 or {B} values, got {a.size}")
    return np.broadcast_to(a, (B,))


def _upload(dev, B: int, cols: Sequence, time, extra: Sequence[int] = ()):
    """(``ids`` [B,3] int64, ``time`` [B] float32 or None, ``extra`` int64 [len(extra)]) on ``dev``.  Host values travel in one copy of
    one buffer; device tensors are stacked on the device."""
    if all(_is_host(c) for c in cols) and _is_host(time):
        n64 = 3 * B + len(extra)
        buf = np.zeros(8 * n64 + 4 * (B if time is not None else 0), np.uint8)
        words = buf[:8 * n64].view(np.int64)
        for k, (c, what) in enumerate(zip(cols, ("img_idx", "frame_idx", "cam_id"))):
            words[k:3 * B:3] = _column(0 if c is None else c, B, what)
        words[3 * B:] = np.asarray(extra, np.int64)
        if time is not None:
            buf[8 * n64:].view(np.float32)[:] = _column(time, B, "normed_time")
        d = torch.from_numpy(buf).to(dev)
        w = d[:8 * n64].view(torch.int64)
        return w[:3 * B].view(B, 3), (d[8 * n64:].view(torch.float32) if time is not None else None), w[3 * B:]

    def on_device(c, dtype, what):
        t = torch.as_tensor(0 if c is None else c).to(device=dev, dtype=dtype).reshape(-1)
        if t.numel() not in (1, B):
            raise ValueError(f"{what} must hold 1 or {B} values, got {t.numel()}")
        return t.expand(B)
    ids = torch.stack([on_device(c, torch.int64, what) for c, what in zip(cols, ("img_idx", "frame_idx", "cam_id"))], dim=1).contiguous()
    t = None if time is None else on_device(time, torch.float32, "normed_time").contiguous()
    return ids, t, (torch.tensor(list(extra), dtype=torch.int64).to(dev) if len(extra) else None)


@torch.no_grad()
def view_fields(c2w: Tensor, intrinsics: Tensor, H: int, W: int, *, scale: float = 1.0, normed_time=None, img_idx, frame_idx,
                cam_id=None) -> Dict[str, Tensor]:
    """``c2w`` [B,4,4] (or [4,4]) and ``intrinsics`` [B,3,3], [1,3,3] or [3,3], unscaled, float32 on the device; ``scale``: the factor
    that ``intrinsics * downscale_factor`` applies; ``normed_time`` (or None), ``img_idx``, ``frame_idx``, ``cam_id`` (or None): one
    value or B, Python numbers, sequences or tensors.  Returns, for [B,4,4] with a leading B and for [4,4] without: ``origins``,
    ``viewdirs`` [H,W,3], ``direction_norm`` [H,W,1], ``pixel_coords`` [H,W,2] (row / H, column / W), ``normed_time`` [H,W] float32 and
    ``cam_id`` [H,W] int64 when given, ``img_idx``, ``frame_idx`` [H,W] int64, and ``intrinsics`` [3,3]: ``intrinsics * scale`` with
    [2,2] = 1.  One launch, no read-back.  BdsError for a CPU pose or intrinsics."""
    return _view_fields(c2w, intrinsics, H, W, scale, normed_time, img_idx, frame_idx, cam_id)[0]


def _view_fields(c2w, intrinsics, H, W, scale, normed_time, img_idx, frame_idx, cam_id, extra: Sequence[int] = ()):
    """``view_fields``; -> (its dict, ``extra`` as int64 on the device, carried by the same upload as the ids)."""
    H, W, scale = int(H), int(W), float(scale)
    single = c2w.dim() == 2
    pose = c2w[None] if single else c2w
    K = intrinsics[None] if intrinsics.dim() == 2 else intrinsics
    if pose.dim() != 3 or tuple(pose.shape[1:]) != (4, 4):
        raise ValueError(f"c2w must be [B,4,4] or [4,4], got {tuple(c2w.shape)}")
    B = pose.shape[0]
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or K.shape[0] not in (1, B):
        raise ValueError(f"intrinsics must be [B,3,3], [1,3,3] or [3,3] with B = {B}, got {tuple(intrinsics.shape)}")
    if H < 0 or W < 0 or B > MAX_VIEWS or B * H * W > MAX_ROWS:
        raise ValueError(f"views must hold B <= {MAX_VIEWS} and B*H*W <= {MAX_ROWS}, got B={B}, H={H}, W={W}")
    if not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    L.require_gpu(pose, K)
    dev = pose.device
    pose, K = pose.detach().float().contiguous(), K.detach().float().contiguous()
    ids, time, extra = _upload(dev, B, (img_idx, frame_idx, cam_id), normed_time, extra)
    L.require_gpu(ids, time)

    def empty(*tail, dtype=torch.float32):
        return torch.empty((B, H, W) + tail, dtype=dtype, device=dev)
    out = {"origins": empty(3), "viewdirs": empty(3), "direction_norm": empty(1), "pixel_coords": empty(2)}
    if time is not None:
        out["normed_time"] = empty()
    out["img_idx"], out["frame_idx"] = empty(dtype=torch.int64), empty(dtype=torch.int64)
    if cam_id is not None:
        out["cam_id"] = empty(dtype=torch.int64)
    out["intrinsics"] = torch.empty(B, 3, 3, dtype=torch.float32, device=dev)
    L.check(L.lib().bds_view_fields(B, H, W, L.ptr(pose), L.ptr(K), K.shape[0], scale, L.ptr(time), L.ptr(ids), L.ptr(out["origins"]),
                                    L.ptr(out["viewdirs"]), L.ptr(out["direction_norm"]), L.ptr(out["pixel_coords"]),
                                    L.ptr(out.get("normed_time")), L.ptr(out["img_idx"]), L.ptr(out["frame_idx"]), L.ptr(out.get("cam_id")),
                                    L.ptr(out["intrinsics"]), L.stream()), "bds_view_fields")
    if B and H * W == 0:
        out["intrinsics"] = (K * scale).expand(B, 3, 3).clone()      # (the entry has nothing to launch for an empty view)
        out["intrinsics"][:, 2, 2] = 1.0
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out, extra


def _factor(factor) -> float:
    factor = float(factor)
    if not (factor > 0.0 and math.isfinite(factor)):
        raise ValueError(f"factor must be positive and finite, got {factor!r}")
    if factor > 1.0:
        raise NotImplementedError(f"factor {factor!r} > 1: the reference never enlarges a view")
    return factor


@torch.no_grad()
def resize_image(img: Tensor, factor: float) -> Tensor:
    """pixel_source.py:492-502 for ``img`` [H,W,3] float32 on the device: torch's antialiased bicubic downscale, width first, then
    height, into a contiguous [floor(H factor), floor(W factor), 3].  ``1 / 512 <= factor <= 1`` (NotImplementedError above 1, ValueError below 1 / 512: a window of more than 2051 taps per axis does not
    fit a workgroup's LDS).  No read-back."""
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"img must be [H,W,3], got {tuple(img.shape)}")
    factor = _factor(factor)
    if factor * MAX_SCALE < 1.0:
        raise ValueError(f"factor must be at least 1/{MAX_SCALE}, got {factor!r}")
    L.require_gpu(img)
    x = img.detach().float().contiguous()
    H, W = int(x.shape[0]), int(x.shape[1])
    if H * W * 3 > MAX_ROWS:
        raise ValueError(f"img holds {H * W * 3} values, more than {MAX_ROWS}")
    Ho, Wo = lidar.output_size(H, W, factor)
    out = torch.empty(Ho, Wo, 3, dtype=torch.float32, device=x.device)
    L.check(L.lib().bds_image_resize_aa(H, W, factor, L.ptr(x), L.ptr(out), L.stream()), "bds_image_resize_aa")
    return out


@torch.no_grad()
def resize_masks(masks: Sequence[Tensor], factor: float) -> List[Tensor]:
    """pixel_source.py:520-579 for up to five ``masks`` [H,W] of one size, float32 on the device: torch's ``mode="nearest"`` with
    ``scale_factor=factor``, values copied, in one launch.  Returns the list of [floor(H factor), floor(W factor)] tensors."""
    masks = list(masks)
    factor = _factor(factor)
    if len(masks) > MAX_MASKS:
        raise ValueError(f"at most {MAX_MASKS} masks in one call, got {len(masks)}")
    if not masks:
        return []
    shape = tuple(masks[0].shape)
    if len(shape) != 2 or any(tuple(m.shape) != shape for m in masks):
        raise ValueError(f"masks must be [H,W] of one size, got {[tuple(m.shape) for m in masks]}")
    L.require_gpu(*masks)
    xs = [m.detach().float().contiguous() for m in masks]
    H, W = shape
    if H * W > MAX_ROWS:
        raise ValueError(f"a mask holds {H * W} values, more than {MAX_ROWS}")
    Ho, Wo = lidar.output_size(H, W, factor)
    outs = [torch.empty(Ho, Wo, dtype=torch.float32, device=xs[0].device) for _ in xs]
    src = (L.C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    dst = (L.C.c_void_p * len(xs))(*[o.data_ptr() for o in outs])
    L.check(L.lib().bds_masks_resize_nearest(len(xs), H, W, factor, src, dst, L.stream()), "bds_masks_resize_nearest")
    return outs


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's methods, on any object with the attributes they read
# ----------------------------------------------------------------------------------------------------------------------------------
def _index_value(v):
    """An index as ``_upload`` takes it: a host value as a Python int, a device tensor as it is."""
    return v if isinstance(v, Tensor) and v.is_cuda else int(v)


@torch.no_grad()
def get_image(self, frame_idx):
    """pixel_source.py:477-657 on a ``CameraData`` (or any object with its attributes) whose tensors live on the device: returns
    ``(image_infos, cam_infos)`` with the reference's keys and shapes, ``None`` entries dropped.  ``height`` and ``width`` are 0-d int64
    on the device, ``intrinsics`` is a fresh tensor, ``camera_to_world`` the row of ``self.cam_to_worlds``, ``cam_name`` the string."""
    s = float(self.downscale_factor)
    c2w = self.cam_to_worlds[frame_idx]
    L.require_gpu(c2w)
    rgb = None
    if self.images is not None:
        rgb = self.images[frame_idx]
        if s != 1.0:
            rgb = resize_image(rgb, s)
            H, W = int(rgb.shape[0]), int(rgb.shape[1])
        else:
            H, W = int(self.HEIGHT), int(self.WIDTH)
    elif s == 1.0:
        H, W = int(self.HEIGHT), int(self.WIDTH)
    else:
        raise ValueError("a camera without images has no size at downscale_factor != 1")
    masks = {"egocar_masks": self.egocar_mask}
    for key, attr in (("sky_masks", self.sky_masks), ("dynamic_masks", self.dynamic_masks), ("human_masks", self.human_masks),
                      ("vehicle_masks", self.vehicle_masks)):
        masks[key] = None if attr is None else attr[frame_idx]
    masks = {k: v for k, v in masks.items() if v is not None}
    if s != 1.0 and masks:
        masks = dict(zip(masks, resize_masks(list(masks.values()), s)))
    depth = None
    if self.lidar_depth_maps is not None:
        depth = self.lidar_depth_maps[frame_idx]
        if s != 1.0:
            depth = lidar.sparse_lidar_map_downsampler(depth, s)
    time = None if self.normalized_time is None else self.normalized_time[frame_idx]
    f, size = _view_fields(c2w, self.intrinsics[frame_idx], H, W, s, time, _index_value(self.unique_img_idx[frame_idx]), _index_value(frame_idx),
                           _index_value(self.cam_id), extra=(H, W))
    image_infos = {"origins": f["origins"], "viewdirs": f["viewdirs"], "direction_norm": f["direction_norm"], "pixel_coords": f["pixel_coords"]}
    if time is not None:
        image_infos["normed_time"] = f["normed_time"]
    image_infos["img_idx"], image_infos["frame_idx"] = f["img_idx"], f["frame_idx"]
    if rgb is not None:
        image_infos["pixels"] = rgb
    for key in ("sky_masks", "dynamic_masks", "human_masks", "vehicle_masks", "egocar_masks"):      # the reference's key order
        if key in masks:
            image_infos[key] = masks[key]
    if depth is not None:
        image_infos["lidar_depth_map"] = depth
    cam_infos = {"cam_id": f["cam_id"], "cam_name": self.cam_name, "camera_to_world": c2w, "height": size[0], "width": size[1],
                 "intrinsics": f["intrinsics"]}
    return image_infos, cam_infos


@torch.no_grad()
def prepare_novel_view_render_data(self, dataset_type: str, traj: Tensor) -> list:
    """pixel_source.py:1070-1132 on a ``ScenePixelSource``: one dict of ``cam_infos`` and ``image_infos`` per pose of ``traj`` [N,4,4],
    all poses in one launch.  As the reference: camera 1 for "argoverse" and camera 0 otherwise, the intrinsics of its frame 0 as they
    are (not copied, [2,2] untouched), ``height`` and ``width`` 1-element tensors, no ``cam_id``, ``frame_idx`` =
    round(linspace(0, num_frames - 1, N)), ``normed_time`` = linspace(0, 1, N), ``img_idx`` = the pose's number."""
    cam = self.camera_data[1 if dataset_type == "argoverse" else 0]
    intrinsics = cam.intrinsics[0]
    H, W = int(cam.HEIGHT), int(cam.WIDTH)
    N = len(traj)
    if N == 0:
        return []
    L.require_gpu(intrinsics)
    frames = torch.linspace(0, self.num_frames - 1, N).round().long()
    f, size = _view_fields(traj.to(intrinsics.device), intrinsics, H, W, 1.0, torch.linspace(0, 1, N), torch.arange(N), frames, None, extra=(H, W))
    return [{"cam_infos": {"camera_to_world": traj[i], "intrinsics": intrinsics, "height": size[0:1], "width": size[1:2]},
             "image_infos": {k: f[k][i] for k in ("origins", "viewdirs", "direction_norm", "img_idx", "frame_idx", "normed_time", "pixel_coords")}}
            for i in range(N)]


_SEAM = Seam()


def _on_device(obj) -> bool:
    """Whether the object's camera tensors live on a GPU (a ``ScenePixelSource``: those of its first camera)."""
    cams = getattr(obj, "camera_data", None)
    if cams is not None:
        obj = next(iter(cams.values()), None) if isinstance(cams, dict) else (cams[0] if len(cams) else None)
    t = getattr(obj, "cam_to_worlds", None)
    return isinstance(t, Tensor) and t.is_cuda


def _dispatch(fn, target, name, seam=None):
    """``fn`` for an object on the device; for one on the CPU the method that ``target`` had: its own, else the inherited one.
    ``seam``: the installing module's (default: this one's)."""
    seam = _SEAM if seam is None else seam

    def method(self, *args, **kwargs):
        if not _on_device(self):
            own = seam.former(target, name)
            if own is not MISSING:
                return own(self, *args, **kwargs)
            inherited = getattr(super(target, self), name, None)
            if inherited is not None:
                return inherited(*args, **kwargs)
        return fn(self, *args, **kwargs)
    method.__name__, method.__doc__, method.__wrapped__ = fn.__name__, fn.__doc__, fn
    return method


def install(camera_data_class=None, scene_pixel_source_class=None) -> None:
    """Sets ``get_image`` on ``camera_data_class`` (the reference's ``CameraData``) and ``prepare_novel_view_render_data`` on
    ``scene_pixel_source_class`` (its ``ScenePixelSource``).  An object whose tensors live on the CPU keeps the class's own method, defined on the class or
    inherited."""
    for target, name, fn in ((camera_data_class, "get_image", get_image),
                             (scene_pixel_source_class, "prepare_novel_view_render_data", prepare_novel_view_render_data)):
        if target is None:
            continue
        _SEAM.install(target, {name: _dispatch(fn, target, name)})


def uninstall(*targets) -> None:
    """Puts back what ``install`` replaced (no target given: on every installed one)."""
    _SEAM.uninstall(*targets)
