"""Lens undistortion on the device (csrc/undistort.hip through ``bds_undistort``): a camera's image and mask stacks, and the lidar
projection onto undistorted images.

Reference: every Waymo config sets ``undistort: True`` (configs/datasets/waymo/{1,3,5}cams.yaml).  ``CameraData.load_images``,
``load_egocar_mask``, ``load_dynamic_masks`` and ``load_sky_masks`` (datasets/base/pixel_source.py:235-375) then run ``cv2.undistort``
frame by frame on the host, and ``DrivingDataset.project_lidar_pts_on_images`` (datasets/driving_dataset.py:670-684) swaps the
intrinsics for ``cv2.getOptimalNewCameraMatrix(K, dist, (W, H), alpha=1)``.

* ``undistort_images(src, K, dist, new_K=None, out="uint8" | "unit" | "mask", device=None)``: ``src`` uint8 [F,H,W,3], [F,H,W] or one
  frame, on the host (numpy or torch) or the device; ``K`` [F,3,3] or [3,3], ``dist`` [F,5] or [5] (k1, k2, p1, p2, k3).  Returns a
  device tensor of the input's shape: uint8, float32 = value / 255 (``"unit"``: the image stack's ``/ 255``) or float32 = value > 0
  (``"mask"``).  A three-dimensional ``src`` is one colour frame [H,W,3] when its last extent is 3 and ``K`` and ``dist`` are single;
  otherwise a stack [F,H,W].
* ``optimal_new_camera_matrix(K, dist, size, alpha=1.0)`` -> float64 [3,3] numpy: ``cv2.getOptimalNewCameraMatrix`` with
  ``newImgSize = imgSize`` and no principal-point centring.
* ``project_lidar_pts_on_images(dataset, delete_out_of_view_points=True)``: the reference's method, cameras with ``undistort``
  included: for such a camera the per-frame matrix is ``pad(optimal_new_camera_matrix(K_f, dist_f, (W, H), 1)) @ inverse(c2w_f)``,
  formed on the host in float32 as ``lidar.camera_matrices`` forms the others; everything else is ``lidar``'s sequence.
* ``install(CameraData, DrivingDataset)`` sets the four loaders on the camera class and ``project_lidar_pts_on_images`` on the
  dataset class; ``uninstall`` puts the former back.  ``lidar.install`` sets a ``project_lidar_pts_on_images`` that refuses
  ``undistort``: call ``undistort.install`` AFTER ``lidar.install`` (and ``undistort.uninstall`` before ``lidar.uninstall``).

The algorithm restates OpenCV 4.x's published one (csrc/undistort_math.h): the map in double, the bilinear taps on the 1/32-pixel
grid with 15-bit integer weights, a constant 0 border.  OpenCV is not installed where this is built: PARITY UNPINNED.  Deviations from
OpenCV: the image is one stripe (OpenCV shifts v0 per stripe of rows); source coordinates beyond +-32767 px count as outside (OpenCV's
16-bit map wraps); ``optimal_new_camera_matrix`` holds its 81 points in float64 (OpenCV: float32).  Deviation from the reference's
loaders: the tensors are born on ``self.device``, so the reference's later ``.to(device)`` is a no-op.

Host work: ``inverse(new K)`` per frame in float64 (numpy), the files' decoding and resize (PIL, the reference's filters).  A host
stack is uploaded in pieces of at most ``STAGE_BYTES`` (whole frames), one launch per piece, so the result is the only full-size
allocation; a device stack is one launch.  No read-back.

Not covered: rational / thin-prism / tilted models (k4..k6, s1..s4, tau), ``alpha`` with ``centerPrincipalPoint``, file decoding on
the device.  ``check_pts_visibility`` keeps the raw intrinsics, as the reference's does."""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from . import lidar
from ._patch import Seam

STAGE_BYTES = 256 << 20      # a host stack is uploaded in pieces of at most this many bytes
MAX_EXTENT = 32767           # include/bds.h: H and W at most
KINDS = {"uint8": 0, "unit": 1, "mask": 2}      # include/bds.h BDS_UNDISTORT_UINT8 / _UNIT / _MASK
GRID = 9                     # getOptimalNewCameraMatrix samples a GRID x GRID lattice of image points
ITERATIONS = 5               # undistortPoints' fixed-point iterations


def _np64(a) -> np.ndarray:
    if isinstance(a, Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def camera_table(K, dist, new_K=None, frames: Optional[int] = None) -> np.ndarray:
    """[F,18] float64: per frame fx, fy, u0, v0 | k1, k2, p1, p2, k3 | inverse(new K) row-major (``new_K`` None: K itself).  ``K``,
    ``new_K`` [F,3,3] or [3,3]; ``dist`` [F,5] or [5]; ``frames``: the F that single entries are repeated to."""
    K, dist = _np64(K), _np64(dist)
    newK = K if new_K is None else _np64(new_K)
    if K.shape[-2:] != (3, 3) or K.ndim not in (2, 3) or newK.shape[-2:] != (3, 3) or newK.ndim not in (2, 3):
        raise ValueError(f"K and new_K must be [F,3,3] or [3,3], got {K.shape} and {newK.shape}")
    if dist.shape[-1] != 5 or dist.ndim not in (1, 2):
        raise ValueError(f"dist must be [F,5] or [5] (k1, k2, p1, p2, k3), got {dist.shape}")
    counts = {a.shape[0] for a, single in ((K, 2), (newK, 2), (dist, 1)) if a.ndim != single}
    if frames is not None:
        counts.add(int(frames))
    if len(counts) > 1:
        raise ValueError(f"K, dist, new_K and the stack disagree on the number of frames: {sorted(counts)}")
    F = counts.pop() if counts else 1
    K, newK, dist = np.broadcast_to(K, (F, 3, 3)), np.broadcast_to(newK, (F, 3, 3)), np.broadcast_to(dist, (F, 5))
    table = np.empty((F, 18), np.float64)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    table[:, 4:9] = dist
    try:
        table[:, 9:] = np.linalg.inv(newK).reshape(F, 9)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the new camera matrix has no inverse: {e}") from None
    if not np.isfinite(table).all():
        raise ValueError("K, dist or inverse(new_K) contains NaN or infinity")
    return table


@torch.no_grad()
def undistort_images(src, K, dist, new_K=None, out: str = "uint8", device=None) -> Tensor:
    """See the module's docstring.  BdsError for a CPU ``device`` (and for a CPU ``src`` when that is all there is to go by: there is
    no CPU path); ValueError for a wrong shape or dtype."""
    if out not in KINDS:
        raise ValueError(f"out must be one of {sorted(KINDS)}, got {out!r}")
    if isinstance(src, np.ndarray):
        src = torch.from_numpy(np.ascontiguousarray(src))
    if not isinstance(src, Tensor) or src.dtype != torch.uint8:
        raise ValueError(f"src must be a uint8 array or tensor, got {getattr(src, 'dtype', type(src))}")
    single_cam = np.ndim(_np64(K)) == 2 and np.ndim(_np64(dist)) == 1 and (new_K is None or np.ndim(_np64(new_K)) == 2)
    shape = tuple(src.shape)
    if src.dim() == 4:
        frames = src
    elif src.dim() == 3 and shape[-1] == 3 and single_cam:
        frames = src[None]
    elif src.dim() == 3:
        frames = src[..., None]
    elif src.dim() == 2:
        frames = src[None, :, :, None]
    else:
        raise ValueError(f"src must be [F,H,W,3], [F,H,W], [H,W,3] or [H,W], got {shape}")
    F, H, W, C = frames.shape
    if C not in (1, 3) or F < 1 or not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT:
        raise ValueError(f"frames must be 1..{MAX_EXTENT} pixels on each side with 1 or 3 channels, at least one of them; got {shape}")
    table = torch.from_numpy(camera_table(K, dist, new_K, F))
    if device is None:
        dev = src.device if src.is_cuda else torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else src.device
    else:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        L.require_gpu(torch.empty(0, device=dev))      # raises: there is no CPU path
    cams = table.to(dev)
    result = torch.empty((F, H, W, C), dtype=torch.uint8 if out == "uint8" else torch.float32, device=dev)
    per_frame = H * W * C
    step = F if frames.device == dev else max(1, STAGE_BYTES // per_frame)
    for f0 in range(0, F, step):
        piece = frames[f0:f0 + step].to(dev).contiguous()
        n = piece.shape[0]
        L.require_gpu(piece, cams, result)
        L.check(L.lib().bds_undistort(n, H, W, C, L.ptr(piece), cams[f0:f0 + n].data_ptr(), KINDS[out], result[f0:f0 + n].data_ptr(),
                                      L.stream()), "bds_undistort")
    return result.reshape(shape)


def _undistort_points(u: np.ndarray, v: np.ndarray, K: np.ndarray, dist: np.ndarray):
    """undistortPoints without R and P: image points to normalised coordinates by ITERATIONS fixed-point steps."""
    k1, k2, p1, p2, k3 = (float(d) for d in dist)
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = x0, y0
    for _ in range(ITERATIONS):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def optimal_new_camera_matrix(K, dist, size, alpha: float = 1.0) -> np.ndarray:
    """``cv2.getOptimalNewCameraMatrix(K, dist, size, alpha)`` (``newImgSize = imgSize``, no principal-point centring) -> float64 [3,3].
    ``size`` = (W, H).  A GRID x GRID lattice over [0, W-1] x [0, H-1] is undistorted to normalised coordinates; the outer rectangle is
    the lattice's bounding box, the inner one the largest of the left and top edges' points and the smallest of the right and bottom
    edges'; f0 = (W - 1) / inner.w, c0 = -f0 inner.x and the same with the outer rectangle (f1, c1) are mixed as
    (1 - alpha) [f0, c0] + alpha [f1, c1], per axis.  Everything in float64."""
    K, dist = _np64(K), _np64(dist)
    if K.shape != (3, 3) or dist.shape != (5,):
        raise ValueError(f"K must be [3,3] and dist [5], got {K.shape} and {dist.shape}")
    W, H = int(size[0]), int(size[1])
    if W < 2 or H < 2:
        raise ValueError(f"size must be at least 2 x 2, got {(W, H)}")
    alpha = float(alpha)
    n = GRID - 1
    gx, gy = np.meshgrid(np.arange(GRID, dtype=np.float64) * (W - 1) / n, np.arange(GRID, dtype=np.float64) * (H - 1) / n)      # [row, column]
    x, y = _undistort_points(gx, gy, K, dist)
    inner_x0, inner_x1, inner_y0, inner_y1 = x[:, 0].max(), x[:, -1].min(), y[0, :].max(), y[-1, :].min()
    outer_x0, outer_x1, outer_y0, outer_y1 = x.min(), x.max(), y.min(), y.max()
    fx0, fy0 = (W - 1) / (inner_x1 - inner_x0), (H - 1) / (inner_y1 - inner_y0)
    fx1, fy1 = (W - 1) / (outer_x1 - outer_x0), (H - 1) / (outer_y1 - outer_y0)
    cx0, cy0, cx1, cy1 = -fx0 * inner_x0, -fy0 * inner_y0, -fx1 * outer_x0, -fy1 * outer_y0
    M = np.zeros((3, 3), np.float64)
    M[0, 0], M[1, 1] = fx0 * (1.0 - alpha) + fx1 * alpha, fy0 * (1.0 - alpha) + fy1 * alpha
    M[0, 2], M[1, 2] = cx0 * (1.0 - alpha) + cx1 * alpha, cy0 * (1.0 - alpha) + cy1 * alpha
    M[2, 2] = 1.0
    return M


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's methods, on any object with the attributes they read
# ----------------------------------------------------------------------------------------------------------------------------------
def camera_matrices(cam) -> Tensor:
    """[F,4,4] float32 on the host: ``lidar.camera_matrices`` with the optimal new camera matrix in place of the intrinsics for a
    camera with ``undistort`` (driving_dataset.py:670-685)."""
    if not getattr(cam, "undistort", False):
        return lidar.camera_matrices(cam)
    out = []
    for f in range(len(cam)):
        new_K = optimal_new_camera_matrix(cam.intrinsics[f], cam.distortions[f], (int(cam.WIDTH), int(cam.HEIGHT)), 1.0)
        K4 = torch.nn.functional.pad(torch.from_numpy(new_K).float(), (0, 1, 0, 1))
        K4[3, 3] = 1.0
        out.append(K4 @ cam.cam_to_worlds[f].detach().cpu().float().inverse())
    return torch.stack(out) if out else torch.zeros(0, 4, 4)


@torch.no_grad()
def project_lidar_pts_on_images(dataset, delete_out_of_view_points: bool = True) -> None:
    """driving_dataset.py:644-727, cameras with ``undistort`` included: ``lidar.project_lidar_pts_on_images``' sequence over
    ``camera_matrices`` above.  With no such camera the results are the same bits."""
    lidar._project_on_images(dataset, delete_out_of_view_points, camera_matrices)


def _camera_device(cam) -> torch.device:
    dev = torch.device(getattr(cam, "device", "cuda"))
    if dev.type != "cuda":
        raise L.BdsError(f"the loaders put their tensors on the GPU (camera device {dev}); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _read(fname, mode: str, size_hw, resample) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(fname).convert(mode).resize((int(size_hw[1]), int(size_hw[0])), resample))


def _load_stack(cam, paths, mode: str, resample, out: str, what: str) -> Tensor:
    """The files read and resized to ``cam.load_size`` as the reference does, stacked, uploaded once, and undistorted in one launch
    with the ``/ 255`` or ``> 0`` fused where ``cam.undistort`` is set; float32 on the camera's device."""
    dev = _camera_device(cam)
    stack = np.stack([_read(fname, mode, cam.load_size, resample) for fname in paths], axis=0)
    if cam.undistort:
        print(f"undistorting {what}")
        return undistort_images(stack, cam.intrinsics[:len(stack)], cam.distortions[:len(stack)], out=out, device=dev)
    u8 = torch.from_numpy(stack).to(dev)
    # (a division by a device tensor: by a Python number the framework multiplies by the reciprocal on the device)
    return u8.float() / torch.full((), 255.0, device=dev) if out == "unit" else (u8 > 0).float()


def load_images(self) -> None:
    """pixel_source.py:235-259: ``self.images`` [F,H,W,3] float32 in [0, 1]."""
    from PIL import Image
    self.images = _load_stack(self, self.img_filepaths, "RGB", Image.BILINEAR, "unit", "rgb")


def load_egocar_mask(self) -> None:
    """pixel_source.py:261-281: ``self.egocar_mask`` [H,W] float32, or None without the file; frame 0's intrinsics."""
    from PIL import Image
    fname = os.path.join("data", "ego_masks", self.dataset_name, f"{self.cam_id}.png")
    if not os.path.exists(fname):
        self.egocar_mask = None
        return
    dev = _camera_device(self)
    mask = _read(fname, "L", self.load_size, Image.BILINEAR)
    if self.undistort:
        self.egocar_mask = undistort_images(mask, self.intrinsics[0], self.distortions[0], out="mask", device=dev)
    else:
        self.egocar_mask = (torch.from_numpy(mask).to(dev) > 0).float()


def load_dynamic_masks(self) -> None:
    """pixel_source.py:283-351: ``self.dynamic_masks``, ``human_masks``, ``vehicle_masks`` [F,H,W] float32."""
    from PIL import Image
    self.dynamic_masks = _load_stack(self, self.dynamic_mask_filepaths, "L", Image.BILINEAR, "mask", "dynamic mask")
    self.human_masks = _load_stack(self, self.human_mask_filepaths, "L", Image.BILINEAR, "mask", "human mask")
    self.vehicle_masks = _load_stack(self, self.vehicle_mask_filepaths, "L", Image.BILINEAR, "mask", "vehicle mask")


def load_sky_masks(self) -> None:
    """pixel_source.py:353-375: ``self.sky_masks`` [F,H,W] float32; the resize is NEAREST."""
    from PIL import Image
    self.sky_masks = _load_stack(self, self.sky_mask_filepaths, "L", Image.NEAREST, "mask", "sky mask")


_LOADERS = {"load_images": load_images, "load_egocar_mask": load_egocar_mask, "load_dynamic_masks": load_dynamic_masks,
            "load_sky_masks": load_sky_masks}
_METHODS = {"project_lidar_pts_on_images": project_lidar_pts_on_images}
_SEAM = Seam()


def install(camera_class=None, dataset_class=None) -> None:
    """Sets the four loaders on ``camera_class`` (the reference's ``CameraData``) and ``project_lidar_pts_on_images`` on
    ``dataset_class`` (``DrivingDataset``).  Call it after ``lidar.install``, which sets a ``project_lidar_pts_on_images`` of its own."""
    for target, names in ((camera_class, _LOADERS), (dataset_class, _METHODS)):
        if target is not None:
            _SEAM.install(target, names)


def uninstall(*targets) -> None:
    """Puts back what ``install`` replaced (no target given: on every installed one)."""
    _SEAM.uninstall(*targets)
