"""Pseudo-lidar generation on the device (csrc/pseudo_lidar.hip through ``bds_pseudo_lidar_from_depth`` and
``bds_pseudo_lidar_from_points``): a rendered depth map turned into a simulated lidar sweep.

Reference: ``generate_lidar/generate_lidar_from_depth.py`` (``depth_map_to_lidar_points`` :95-162, ``pto_ang_map_vertical`` :42-92,
``pto_ang_map`` :6-40) and ``generate_lidar/depth2lidar.py`` (``pto_ang_map`` :41-75, ``gen_sparse_points`` :78-90) unproject every
pixel, move it into the lidar's frame, crop it to the sensor's box and bin it into an ``H x W`` angular map of beams in which numpy's
assignment with duplicate indices keeps the last write; the occupied beams come back in beam order.  The reference does this on the
host per camera and frame: a boolean compaction of the full-resolution depth map, two ``4 x N`` products and a float64 numpy pass.

* ``depth_to_lidar(depths, intrinsics, cam_to_world, lidar_to_world, ...)`` -> ``points`` [C,cap,3], ``counts`` [C] (and ``source``
  [C,cap]), the C cameras of a frame in one call, on the device, nothing read back; ``split=True`` reads the counts once and returns
  the list of [M_c,3] tensors.
* ``cloud_to_lidar(cloud, ...)`` -> ``points`` [cap,4], ``counts`` [1] (and ``source``) for a cloud [N,4] on the device.
* the reference's functions under their names and argument lists, returning what the reference returns (numpy float64 [M,3] / [M,4]):
  ``depth_map_to_lidar_points``, ``pto_ang_map``, ``pto_ang_map_vertical``, ``gen_sparse_points``; ``install(module)`` sets them on the
  reference's module, ``uninstall`` puts the former back.

The winner rule.  Where several pixels fall into one beam the highest linear pixel index ``v * width + u`` wins (for a cloud: the
highest row), always -- the last write of the reference's assignment.  ``source`` names the winner of every emitted point.

Deviations.  (1) The camera-to-lidar matrix ``inverse(lidar_to_world) @ cam_to_world`` is formed once per camera on the host in
float64 from the float32 inputs and rounded once; the reference takes two float32 products through world coordinates, which with world
translations of hundreds of metres costs it about 1e-5 m.  (2) The outputs are float32, the coordinates the kernels computed; the
reference-named wrappers widen them to float64.  (3) The reference marks an empty beam by x == -1 and so also drops an occupied beam
whose winner has x == -1.0 exactly; here such a beam is emitted (with the reference's crop x >= 0 it cannot occur on the depth path).
(4) A cloud given in float64 is rounded to float32.  The angles themselves are taken in double from the widened float32 coordinates,
with the reference's own numpy constants, as the reference's numpy part does.

Read-backs: none in ``depth_to_lidar`` / ``cloud_to_lidar`` (``split=True``: the counts); the reference-named wrappers return numpy
arrays and so read their result back.  The small per-call tables (16 floats per camera, 12 doubles) are formed on the host and
uploaded.  ValueError for a non-finite matrix, intrinsic or cloud coordinate; BdsError for a CPU tensor.

Not covered: ``save_ply``, ``pto_rec_map``, ``gen_sparse_points_all``, the radar and box scripts.  Lens distortion: the
depth maps are renders of undistorted cameras (``undistort`` prepares their images and the lidar projection), so the pinhole model here holds."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam
from .lidar import MAX_ROWS, _cloud as _finite_on_device

VERTICAL, CLASSIC = 0, 1      # include/bds.h BDS_PSEUDO_LIDAR_VERTICAL / _CLASSIC
BEAMS = 12                    # include/bds.h BDS_PSEUDO_LIDAR_BEAMS
MAX_CAMERAS = 65535
CROP = (0.0, 80.0, -50.0, 50.0, -2.5, 3.0)               # generate_lidar_from_depth.py:152-157
SPARSE_CROP = (0.0, 120.0, -50.0, 50.0, -2.5, 1.5)       # depth2lidar.py:82-87
_MODES = {"vertical": VERTICAL, "classic": CLASSIC}


def beam_table(H: int, W: int, mode: str = "vertical", fov=(10.0, -30.0), crop: Optional[Sequence[float]] = CROP,
               max_depth: float = 80.0) -> np.ndarray:
    """The BEAMS doubles of a call, with the reference's own numpy expressions (generate_lidar_from_depth.py:13-14, :51-54, :63-64)."""
    if mode not in _MODES:
        raise ValueError(f"mode must be 'vertical' or 'classic', got {mode!r}")
    t = np.zeros(BEAMS, np.float64)
    t[0], t[1] = np.radians(45.), np.radians(90.0 / W)
    if mode == "vertical":
        up, down = np.radians(fov[0]), np.radians(fov[1])
        t[2], t[3], t[4] = down, up, (up - down) / H
    else:
        t[2], t[3], t[4] = np.radians(2.), 0.0, np.radians(0.4 * 64.0 / H)
    t[5:11] = (-math.inf, math.inf) * 3 if crop is None else np.asarray(crop, np.float64).reshape(6)
    t[11] = np.float32(max_depth)      # (the reference compares the float32 depth with the float32 scalar)
    if np.isnan(t).any() or not np.isfinite(t[:5]).all() or not t[4] > 0 or not t[1] > 0:
        raise ValueError("fov, crop and max_depth must be numbers, with fov_up > fov_down")
    return t


def _sizes(H, W, slice, cameras=1):
    H, W, slice = int(H), int(W), int(slice)
    if H < 1 or W < 1 or slice < 1:
        raise ValueError(f"H, W and slice must be at least 1, got {H}, {W}, {slice}")
    cap = -(-H // slice) * W
    if cameras * H * W > MAX_ROWS or 4 * cameras * cap > MAX_ROWS:
        raise ValueError(f"C*H*W and 4*C*ceil(H/slice)*W must stay below {MAX_ROWS}, got C={cameras}, H={H}, W={W}")
    return H, W, slice, cap


def camera_table(intrinsics: Tensor, cam_to_world: Tensor, lidar_to_world: Tensor, downscale_when_loading: float = 1) -> Tensor:
    """[C,16] float32 on the host: fx fy cx cy divided by ``downscale_when_loading`` (in double, as the reference's Python floats) and
    the first three rows of ``inverse(lidar_to_world) @ cam_to_world``, formed in float64 from the float32 inputs, rounded once."""
    K = torch.as_tensor(intrinsics).detach().cpu()
    if K.dim() != 2 or K.shape[1] < 4:
        raise ValueError(f"intrinsics must be [C,4] (fx, fy, cx, cy), got {tuple(K.shape)}")
    C = K.shape[0]
    c2w = torch.as_tensor(cam_to_world).detach().cpu()
    l2w = torch.as_tensor(lidar_to_world).detach().cpu()
    if l2w.dim() == 2:
        l2w = l2w[None].expand(C, 4, 4)
    if tuple(c2w.shape) != (C, 4, 4) or tuple(l2w.shape) != (C, 4, 4):
        raise ValueError(f"cam_to_world must be [C,4,4] and lidar_to_world [4,4] or [C,4,4] with C = {C}, got {tuple(c2w.shape)}, "
                         f"{tuple(l2w.shape)}")
    if not float(downscale_when_loading) > 0:
        raise ValueError(f"downscale_when_loading must be positive, got {downscale_when_loading!r}")
    K = K[:, :4].float().double() / float(downscale_when_loading)
    c2w, l2w = c2w.float().double(), l2w.float().double()
    if not (torch.isfinite(K).all() and torch.isfinite(c2w).all() and torch.isfinite(l2w).all()):
        raise ValueError("intrinsics, cam_to_world and lidar_to_world must be finite")
    if bool((K[:, :2] == 0).any()):
        raise ValueError("fx and fy must not be 0")
    try:
        M = torch.linalg.inv(l2w) @ c2w if C else torch.zeros(0, 4, 4, dtype=torch.float64)
    except RuntimeError as err:
        raise ValueError(f"lidar_to_world is singular: {err}") from None
    table = torch.cat([K, M[:, :3, :].reshape(C, 12)], dim=1).float().contiguous()
    if not torch.isfinite(table).all():
        raise ValueError("lidar_to_world is singular")
    return table


@torch.no_grad()
def depth_to_lidar(depths: Tensor, intrinsics: Tensor, cam_to_world: Tensor, lidar_to_world: Tensor, H: int = 32, W: int = 256,
                   slice: int = 1, downscale_when_loading: float = 1, mode: str = "vertical", crop: Optional[Sequence[float]] = CROP,
                   max_depth: float = 80.0, fov=(10.0, -30.0), return_source: bool = False, split: bool = False):
    """``depths`` [C,Hi,Wi] (or [Hi,Wi]) float32 on the device, ``intrinsics`` [C,4] (fx, fy, cx, cy), ``cam_to_world`` [C,4,4],
    ``lidar_to_world`` [4,4] or [C,4,4] (any device; read on the host).  ``fov`` = (up, down) in degrees, ``crop`` = (x0, x1, y0, y1,
    z0, z1) or None.  Returns ``points`` [C,cap,3] float32 in the lidar's frame and ``counts`` [C] int32 -- rows [0, counts[c]) of
    camera c are its occupied beams in beam order, the rows behind them are not written -- and with ``return_source`` also ``source``
    [C,cap] int32, the linear pixel ``v * Wi + u`` each point came from; cap = ceil(H / slice) * W.  No read-back.  ``split=True``:
    reads the counts once and returns the list of [M_c,3] tensors (with ``return_source``: and the list of [M_c] sources)."""
    single = depths.dim() == 2
    if depths.dim() not in (2, 3):
        raise ValueError(f"depths must be [C,Hi,Wi] or [Hi,Wi], got {tuple(depths.shape)}")
    table = camera_table(intrinsics, cam_to_world, lidar_to_world, downscale_when_loading)
    C, Hi, Wi = (1, *depths.shape) if single else depths.shape
    if table.shape[0] != C:
        raise ValueError(f"{C} depth maps but {table.shape[0]} cameras")
    H, W, slice, cap = _sizes(H, W, slice, max(C, 1))
    if Hi < 1 or Wi < 1 or C * Hi * Wi > MAX_ROWS or C > MAX_CAMERAS:
        raise ValueError(f"depths must hold 1..{MAX_ROWS} pixels of at most {MAX_CAMERAS} cameras, got {tuple(depths.shape)}")
    beams = beam_table(H, W, mode, fov, crop, max_depth)
    L.require_gpu(depths)
    d = depths.detach().float().contiguous()
    dev = d.device
    cams, beams_d = table.to(dev), torch.from_numpy(beams).to(dev)
    winner = torch.empty(C, H, W, dtype=torch.int32, device=dev)
    points = torch.empty(C, cap, 3, dtype=torch.float32, device=dev)
    counts = torch.zeros(C, dtype=torch.int32, device=dev)
    source = torch.empty(C, cap, dtype=torch.int32, device=dev) if return_source else None
    L.check(L.lib().bds_pseudo_lidar_from_depth(C, Hi, Wi, L.ptr(d), L.ptr(cams), L.ptr(beams_d), H, W, slice, _MODES[mode], L.ptr(winner),
                                                L.ptr(points), L.ptr(counts), L.ptr(source), L.stream()), "bds_pseudo_lidar_from_depth")
    if not split:
        return (points, counts, source) if return_source else (points, counts)
    n = counts.cpu().tolist()
    pts = [points[c, :n[c]] for c in range(C)]
    return (pts, [source[c, :n[c]] for c in range(C)]) if return_source else pts


@torch.no_grad()
def cloud_to_lidar(cloud: Tensor, H: int = 64, W: int = 512, slice: int = 1, mode: str = "classic", crop: Optional[Sequence[float]] = None,
                   fov=(10.0, -30.0), return_source: bool = False):
    """``cloud`` [N,4] (x, y, z, intensity) float32 on the device.  Returns ``points`` [cap,4] -- the winners' rows, copied -- and
    ``counts`` [1] int32 (and ``source`` [cap] int32, the cloud row of each) -- as in ``depth_to_lidar``, rows [0, counts[0]) are the
    occupied beams in beam order, the rows behind them are not written.  One read-back: the flag of the finiteness check."""
    if cloud.dim() != 2 or cloud.shape[1] != 4:
        raise ValueError(f"cloud must be [N,4], got {tuple(cloud.shape)}")
    H, W, slice, cap = _sizes(H, W, slice)
    N = cloud.shape[0]
    if N > MAX_ROWS:
        raise ValueError(f"cloud holds {N} rows, more than {MAX_ROWS}")
    beams = beam_table(H, W, mode, fov, crop)
    L.require_gpu(cloud)
    x = cloud.detach().float().contiguous()
    _finite_on_device(x[:, :3], "cloud")
    dev = x.device
    beams_d = torch.from_numpy(beams).to(dev)
    winner = torch.empty(H, W, dtype=torch.int32, device=dev)
    points = torch.empty(cap, 4, dtype=torch.float32, device=dev)
    counts = torch.zeros(1, dtype=torch.int32, device=dev)
    source = torch.empty(cap, dtype=torch.int32, device=dev) if return_source else None
    L.check(L.lib().bds_pseudo_lidar_from_points(N, L.ptr(x), L.ptr(beams_d), int(crop is not None), H, W, slice, _MODES[mode],
                                                 L.ptr(winner), L.ptr(points), L.ptr(counts), L.ptr(source), L.stream()),
            "bds_pseudo_lidar_from_points")
    return (points, counts, source) if return_source else (points, counts)


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's functions under their names
# ----------------------------------------------------------------------------------------------------------------------------------
def _cloud_on_device(velo_points) -> Tensor:
    if isinstance(velo_points, Tensor):
        return velo_points
    return torch.from_numpy(np.ascontiguousarray(np.asarray(velo_points), dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))


def _emitted(points: Tensor, counts: Tensor) -> np.ndarray:
    return points[:int(counts[0])].cpu().numpy().astype(np.float64)


def pto_ang_map(velo_points, H=64, W=512, slice=1):
    """generate_lidar_from_depth.py:6-40 / depth2lidar.py:41-75: ``velo_points`` [N,4] (numpy, or a tensor on the device) -> numpy
    float64 [M,4], the occupied beams of every ``slice``-th row in beam order."""
    return _emitted(*cloud_to_lidar(_cloud_on_device(velo_points), H, W, slice, "classic"))


def pto_ang_map_vertical(velo_points, H=64, W=512, slice=1, vertical_fov_up=10.0, vertical_fov_down=-30.0):
    """generate_lidar_from_depth.py:42-92."""
    return _emitted(*cloud_to_lidar(_cloud_on_device(velo_points), H, W, slice, "vertical", fov=(vertical_fov_up, vertical_fov_down)))


def depth_map_to_lidar_points(depth_map, cam_intrinsics, cam_to_world, width, height, lidar_to_world, H=32, W=256, slice=1,
                              downscale_when_loading=1):
    """generate_lidar_from_depth.py:95-162: ``depth_map`` [height,width] on the device, ``cam_intrinsics`` (fx, fy, cx, cy) -> numpy
    float64 [M,3] in the lidar's frame."""
    if tuple(depth_map.shape) != (int(height), int(width)):
        raise ValueError(f"depth_map must be [height,width] = {(int(height), int(width))}, got {tuple(depth_map.shape)}")
    K = torch.as_tensor(cam_intrinsics).detach().reshape(-1)[:4][None]
    points, counts = depth_to_lidar(depth_map[None], K, torch.as_tensor(cam_to_world)[None], lidar_to_world, H, W, slice,
                                    downscale_when_loading)
    return _emitted(points[0], counts)


def gen_sparse_points(pl_data_path, args):
    """depth2lidar.py:78-90: the float32 [N,4] file at ``pl_data_path``, cropped to [0,120) x [-50,50) x [-2.5,1.5), through
    ``pto_ang_map(H=args.H, W=args.W, slice=args.slice)``."""
    pc_velo = np.fromfile(pl_data_path, dtype=np.float32).reshape((-1, 4))
    return _emitted(*cloud_to_lidar(_cloud_on_device(pc_velo), args.H, args.W, args.slice, "classic", crop=SPARSE_CROP))


_FUNCTIONS = {"depth_map_to_lidar_points": depth_map_to_lidar_points, "pto_ang_map": pto_ang_map,
              "pto_ang_map_vertical": pto_ang_map_vertical, "gen_sparse_points": gen_sparse_points}
_SEAM = Seam()


def install(module) -> None:
    """Sets the functions on ``module``: those of the four names that it defines (``generate_lidar.generate_lidar_from_depth`` has
    three, ``generate_lidar.depth2lidar`` two), or all four on a module that defines none."""
    names = [n for n in _FUNCTIONS if n in module.__dict__] or list(_FUNCTIONS)
    _SEAM.install(module, {name: _FUNCTIONS[name] for name in names})


def uninstall(*modules) -> None:
    """Puts back what ``install`` replaced (no module given: on every installed one)."""
    _SEAM.uninstall(*modules)
