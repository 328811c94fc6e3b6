"""Evaluation geometry metrics as HIP ops (csrc/geometry.hip through ``bds_geometry_metrics``, ``bds_chamfer_nn`` and
``bds_depth_unproject``): the Chamfer distance between the rendered depth and the lidar returns, and the depth errors.

Reference: ``render_images`` (models/video_utils.py:363-536) unprojects the lidar depth map and the render's expected depth through one
validity mask, calls ``pytorch3d.ops.knn.knn_points`` both ways (utils/chamfer_distance.py:34-52; pytorch3d is CUDA-only), sorts the two
distance arrays and the depth errors for their trimmed means, repeats the clouds and the search for the sky, dynamic, human, vehicle and
background subsets, and reads every value back with ``.item()``.

* ``geometry_metrics(pred_depth, gt_depth, K, c2w, masks, egocar)``: every value of a frame as 0-dim float64 device tensors, without a
  host wait.  The distances are SQUARED (``knn_points(norm=2).dists``; the reference means them as they are), from coordinate
  differences in float32.
* ``chamfer_distance(x, y, norm=2)``, ``depth_map_to_point_cloud(depth_map, K, c2w, valid_mask=None)``: the reference's names and
  arguments; ``install(module)`` sets both on ``utils.chamfer_distance``, which ``render_images`` imports at call time, so the
  unmodified reference evaluates geometry without pytorch3d.
* ``frame_geometry(depth, image_infos, cam_infos)``: lines 363-536 under the reference's per-frame names, floats, one read-back.
* ``GeometryAccumulator``: a split's frames into one device buffer, read once by ``results()`` (lines 558-573).

One deviation: a mask key absent from ``image_infos`` counts as all-false (the reference raises a NameError at line 519 then).  The
class clouds hold the valid pixels where the mask is non-zero, as ``metrics._mask_kind`` reads masks.  Scene initialisation's K > 1
neighbour searches live in ``init.py``."""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam
from .metrics import RowAccumulator, _mask_kind, grown, non_zero_mean

ROW = 32                    # include/bds.h BDS_GEOMETRY_METRICS_ROW
QUERY_BLOCK = 512           # include/bds.h BDS_GEOMETRY_QUERY_BLOCK: queries per workgroup of the pair loop
TARGET_TILE = 512           # include/bds.h BDS_GEOMETRY_TARGET_TILE: targets per LDS tile
MAX_PIXELS = 1 << 24        # include/bds.h: the largest H*W the entries take
CLASSES = ("sky", "dynamic", "human", "vehicle", "background")
MASK_KEYS = ("sky_masks", "dynamic_masks", "human_masks", "vehicle_masks")
TRIMS = ("", "_99", "_97", "_95")
# name -> slot of the row
ROW_SLOTS = {**{f"chamfer{t}": i for i, t in enumerate(TRIMS)},
             "depth_err": 4, "depth_err_rmse_99": 5, "depth_err_rmse_97": 6, "depth_err_rmse_95": 7, "depth_err_median_squared": 8,
             **{f"chamfer_{c}": 9 + i for i, c in enumerate(CLASSES)}, "valid": 14, **{f"{c}_valid": 15 + i for i, c in enumerate(CLASSES)},
             **{f"cham_pred{t}": 20 + i for i, t in enumerate(TRIMS)}, **{f"cham_gt{t}": 24 + i for i, t in enumerate(TRIMS)},
             **{f"abs_err{t}": 28 + i for i, t in enumerate(TRIMS)}}
FRAME_KEYS = tuple(f"chamfer{t}" for t in TRIMS) + ("depth_err", "depth_err_rmse_99", "depth_err_rmse_97", "depth_err_rmse_95",
                                                     "depth_err_median_squared")
RESULT_KEYS = tuple(f"avg_{k}" if k.startswith("chamfer") else k for k in FRAME_KEYS) + tuple(f"avg_chamfer_{c}" for c in CLASSES)


def _depth(t: Tensor, what: str) -> Tensor:
    t = t.squeeze()
    if t.dim() != 2 or t.numel() == 0 or t.numel() > MAX_PIXELS:
        raise ValueError(f"{what} must be [H,W] with at most {MAX_PIXELS} pixels, got {tuple(t.shape)}")
    return t.detach().contiguous().float()


def _camera(K: Tensor, c2w: Tensor) -> Tuple[Tensor, Tensor]:
    """The upper-left 3x3 of the intrinsics and the 4x4 camera-to-world as contiguous float32 tensors (device ops, no host copy)."""
    if K.dim() != 2 or K.shape[0] < 3 or K.shape[1] < 3:
        raise ValueError(f"intrinsics must be at least [3,3], got {tuple(K.shape)}")
    if tuple(c2w.shape) != (4, 4):
        raise ValueError(f"camera_to_world must be [4,4], got {tuple(c2w.shape)}")
    return K.detach()[:3, :3].float().contiguous(), c2w.detach().float().contiguous()


def _masks(masks: list, shape) -> Tuple[list, int]:
    """[mask or None] -> ([contiguous tensor or None], mask kind): one element type for all, as ``metrics._launch``."""
    out = []
    for m in masks:
        if m is not None:
            m = m.squeeze()
            if tuple(m.shape) != tuple(shape):
                raise ValueError(f"mask must be [H,W] = {tuple(shape)}, got {tuple(m.shape)}")
        out.append(m)
    kinds = {_mask_kind(m) for m in out if m is not None}
    if len(kinds) > 1 or -1 in kinds:
        out = [None if m is None else (m if _mask_kind(m) == 0 else (m != 0)) for m in out]
        kinds = {0}
    return [None if m is None else m.detach().contiguous() for m in out], (kinds.pop() if kinds else 0)


def _workspace(H: int, W: int, device, ws: Optional[Tensor]) -> Tensor:
    return grown(ws, int(L.lib().bds_geometry_metrics_workspace_bytes(H, W)), device)


def _launch(pred: Tensor, gt: Tensor, K: Tensor, c2w: Tensor, masks: list, egocar: Optional[Tensor], row: Tensor,
            dists: Optional[Tuple[Tensor, Tensor]] = None, ws: Optional[Tensor] = None) -> None:
    """``pred``, ``gt``: [H,W] float32 contiguous; ``masks``: four [H,W] tensors or None; ``row``: [ROW] float64, contiguous."""
    if pred.shape != gt.shape:
        raise ValueError(f"the rendered depth {tuple(pred.shape)} and the lidar depth map {tuple(gt.shape)} must have the same shape")
    held, kind = _masks([egocar, *masks], pred.shape)
    L.require_gpu(pred, gt, K, c2w, row, *held, *(dists or ()))
    H, W = pred.shape
    ws = _workspace(H, W, pred.device, ws)
    dp, dg = dists if dists is not None else (None, None)
    L.check(L.lib().bds_geometry_metrics(H, W, L.ptr(pred), L.ptr(gt), *[L.ptr(m) for m in held], kind, L.ptr(K), L.ptr(c2w), L.ptr(row),
                                         L.ptr(dp), L.ptr(dg), L.ptr(ws), ws.numel(), L.stream()), "bds_geometry_metrics")


@torch.no_grad()
def geometry_metrics(pred_depth: Tensor, gt_depth: Tensor, K: Tensor, c2w: Tensor, masks: Optional[Mapping[str, Tensor]] = None,
                     egocar: Optional[Tensor] = None, return_distances: bool = False) -> Dict[str, Tensor]:
    """``pred_depth``, ``gt_depth`` [H,W]; ``K`` the intrinsics (its upper-left 3x3), ``c2w`` [4,4], both on the device; ``masks``:
    any of ``sky_masks``, ``dynamic_masks``, ``human_masks``, ``vehicle_masks`` -> [H,W] bool, uint8 or float (non-zero = true; an
    absent key is all-false); ``egocar`` [H,W] or None.  Returns 0-dim float64 device tensors: ``chamfer``, ``chamfer_99/97/95``,
    ``depth_err``, ``depth_err_rmse_99/97/95``, ``depth_err_median_squared``, ``chamfer_<class>`` (NaN for an empty class),
    ``cham_pred*`` / ``cham_gt*`` / ``abs_err*`` (the means the sums are made of), ``valid`` (n) and ``<class>_valid`` (the counts).
    n = 0 gives NaN.  With ``return_distances`` also ``dist_pred`` / ``dist_gt``: [H*W] float32 arrays whose first n entries are the
    squared distance of every pred point to its nearest lidar point, and the converse, in row-major pixel order.  No host wait."""
    masks = dict(masks or {})
    if not set(masks) <= set(MASK_KEYS):
        raise ValueError(f"masks takes the keys {MASK_KEYS}, got {sorted(set(masks) - set(MASK_KEYS))}")
    pred, gt = _depth(pred_depth, "pred_depth"), _depth(gt_depth, "gt_depth")
    K, c2w = _camera(K, c2w)
    row = torch.empty(ROW, dtype=torch.float64, device=pred.device)
    dists = tuple(torch.empty(pred.numel(), dtype=torch.float32, device=pred.device) for _ in range(2)) if return_distances else None
    _launch(pred, gt, K, c2w, [masks.get(k) for k in MASK_KEYS], egocar, row, dists)
    out = {name: row[slot] for name, slot in ROW_SLOTS.items()}
    if return_distances:
        out["dist_pred"], out["dist_gt"] = dists
    return out


@torch.no_grad()
def depth_map_to_point_cloud(depth_map: Tensor, K: Tensor, c2w: Tensor, valid_mask: Optional[Tensor] = None) -> Tensor:
    """utils/chamfer_distance.py:54-75: the world points [n,3] float32 of the pixels where ``valid_mask`` is true (None: all), in
    row-major pixel order.  One read-back, for n."""
    depth = _depth(depth_map, "depth_map")
    K, c2w = _camera(K, c2w)
    (mask,), kind = _masks([valid_mask], depth.shape)
    H, W = depth.shape
    points = torch.empty(H * W, 3, dtype=torch.float32, device=depth.device)
    count = torch.zeros(1, dtype=torch.int64, device=depth.device)
    L.require_gpu(depth, K, c2w, mask)
    ws = _workspace(H, W, depth.device, None)
    L.check(L.lib().bds_depth_unproject(H, W, L.ptr(depth), L.ptr(mask), kind, L.ptr(K), L.ptr(c2w), L.ptr(points), L.ptr(count), L.ptr(ws),
                                        ws.numel(), L.stream()), "bds_depth_unproject")
    return points[:int(count.item())].clone()


@torch.no_grad()
def chamfer_distance(x: Tensor, y: Tensor, norm: int = 2) -> Tuple[Tensor, Tensor]:
    """utils/chamfer_distance.py:34-52: ``x`` [P1,3] and ``y`` [P2,3], or batched [N,P1,3] / [N,P2,3] -> (cham_x, cham_y), per point
    the squared Euclidean distance (``norm=2``) or the sum of absolute differences (``norm=1``) to the nearest point of the other
    cloud, float32 on the device (+inf against an empty cloud)."""
    if not (norm == 1 or norm == 2):
        raise ValueError("Support for 1 or 2 norm.")
    if x.dim() not in (2, 3) or y.dim() not in (2, 3):
        raise ValueError(f"x and y must be [P,3] or [N,P,3], got {tuple(x.shape)} and {tuple(y.shape)}")
    bx, by = (x[None] if x.dim() == 2 else x), (y[None] if y.dim() == 2 else y)
    if bx.shape[2] != 3 or by.shape[2] != 3:
        raise ValueError(f"points must have 3 coordinates, got {tuple(x.shape)} and {tuple(y.shape)}")
    if bx.shape[0] != by.shape[0]:
        raise ValueError("y does not have the correct shape.")
    L.require_gpu(x, y)
    bx, by = bx.detach().float().contiguous(), by.detach().float().contiguous()
    N, P1, P2 = bx.shape[0], bx.shape[1], by.shape[1]
    cx = torch.empty(N, P1, dtype=torch.float32, device=x.device)
    cy = torch.empty(N, P2, dtype=torch.float32, device=x.device)
    lib = L.lib()
    for b in range(N):
        L.check(lib.bds_chamfer_nn(P1, P2, L.ptr(bx[b]), L.ptr(by[b]), norm, L.ptr(cx[b]), L.ptr(cy[b]), L.stream()), "bds_chamfer_nn")
    return (cx[0] if x.dim() == 2 else cx), (cy[0] if y.dim() == 2 else cy)


_SEAM = Seam()


def install(module) -> None:
    """Sets ``chamfer_distance`` and ``depth_map_to_point_cloud`` on ``module`` -- the reference's ``utils.chamfer_distance``, which
    ``render_images`` imports from at call time."""
    _SEAM.install(module, {"chamfer_distance": chamfer_distance, "depth_map_to_point_cloud": depth_map_to_point_cloud})


def uninstall(*modules) -> None:
    """Puts back what ``install`` replaced (no module given: on every installed one)."""
    _SEAM.uninstall(*modules)


def _frame_inputs(depth: Tensor, image_infos: Mapping[str, Tensor], cam_infos: Mapping[str, Tensor]):
    pred, gt = _depth(depth, "depth"), _depth(image_infos["lidar_depth_map"], "image_infos['lidar_depth_map']")
    K, c2w = _camera(cam_infos["intrinsics"], cam_infos["camera_to_world"])
    return pred, gt, K, c2w, [image_infos.get(k) for k in MASK_KEYS], image_infos.get("egocar_masks")


def _row_to_dict(vals) -> Dict[str, float]:
    """The frame's values as the reference's lists receive them: a class value only where neither mean is NaN (:453-536)."""
    out = {k: vals[ROW_SLOTS[k]] for k in FRAME_KEYS}
    for c in CLASSES:
        v = vals[ROW_SLOTS[f"chamfer_{c}"]]
        if not math.isnan(v):
            out[f"chamfer_{c}"] = v
    return out


@torch.no_grad()
def frame_geometry(depth: Tensor, image_infos: Mapping[str, Tensor], cam_infos: Mapping[str, Tensor]) -> Dict[str, float]:
    """One frame's values of video_utils.py:363-536 as floats: ``chamfer``, ``chamfer_99/97/95``, ``depth_err``,
    ``depth_err_rmse_99/97/95``, ``depth_err_median_squared`` and, for every class with at least one valid point, ``chamfer_<class>``."""
    pred, gt, K, c2w, masks, ego = _frame_inputs(depth, image_infos, cam_infos)
    row = torch.empty(ROW, dtype=torch.float64, device=pred.device)
    _launch(pred, gt, K, c2w, masks, ego, row)
    return _row_to_dict(row.cpu().tolist())


class GeometryAccumulator(RowAccumulator):
    """The geometry scores of a split: ``add(depth, image_infos, cam_infos)`` writes the next frame's row into a preallocated
    [num_frames, ROW] device buffer (no host wait); ``results()`` reads the buffer once and returns ``results_dict``'s entries
    (video_utils.py:558-573): per key the mean over the frames that produced it, -1 where none did.  Like the reference, a frame
    without a valid point enters the whole-frame means as NaN."""
    ROW, WORKSPACE_BYTES = ROW, "bds_geometry_metrics_workspace_bytes"

    @torch.no_grad()
    def add(self, depth: Tensor, image_infos: Mapping[str, Tensor], cam_infos: Mapping[str, Tensor]) -> None:
        self._require_room()
        pred, gt, K, c2w, masks, ego = _frame_inputs(depth, image_infos, cam_infos)
        row, ws = self._next(*pred.shape, pred, gt)
        _launch(pred, gt, K, c2w, masks, ego, row, None, ws)
        self.count += 1

    def per_frame(self):
        """[{key: float}] of the frames added so far, the keys ``frame_geometry`` gives (one read-back)."""
        return [_row_to_dict(v) for v in self.rows[:self.count].cpu().tolist()]

    def results(self) -> Dict[str, float]:
        frames = self.per_frame()
        out = {}
        for k in FRAME_KEYS + tuple(f"chamfer_{c}" for c in CLASSES):
            out[f"avg_{k}" if k.startswith("chamfer") else k] = non_zero_mean([f[k] for f in frames if k in f])
        return out
