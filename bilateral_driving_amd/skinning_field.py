"""The SMPL nodes' skinning-weight field on the device: what ``VoxelDeformer._query_weights_smpl`` (models/modules.py:1197-1226) makes
of the template's vertices when a human is created -- for every voxel centre the inverse-distance blend of the skinning weights of its
K = 30 nearest vertices, then thirty relaxation steps over the grid.

The reference forms the blend from ``knn_points``' indices through a [B, d*h*w, K, J] gather (189 MB per human at 16 x 64 x 64 voxels,
K = 30, J = 24).  ``query_weights`` takes it from the search's fused epilogue instead (``p3d.knn_blend``: no indices, no gather) and
runs the relaxation as torch ops on the [B,J,d,h,w] result, as the reference does.

``install(models.modules.VoxelDeformer)`` sets the class's ``_query_weights_smpl`` to that; ``uninstall`` puts the former back.  Without
it the unmodified method runs through the drop-in ``pytorch3d.ops.knn_points`` with its gather.  CPU tensors keep the class's own method."""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
from torch import Tensor

from . import p3d
from ._patch import Seam

K_NEIGHBOURS = 30               # modules.py:1199
CLAMP = (0.0001, 1.0)           # modules.py:1200
SMOOTH_ITERS = 30               # modules.py:1212
SMOOTH_KEEP = 0.7               # modules.py:1221-1223: a cell keeps this share of its offset from its six neighbours' mean
FORMER = "_query_weights_smpl_torch"


def relax(weights: Tensor, iters: int = SMOOTH_ITERS) -> Tensor:
    """modules.py:1212-1225 on ``weights`` [B,J,d,h,w] (changed in place where the steps allow): ``iters`` times, every interior cell
    moves towards the mean of its six face neighbours, then every cell's J weights are divided by their sum."""
    for _ in range(iters):
        inner = weights[:, :, 1:-1, 1:-1, 1:-1]
        mean = (weights[:, :, 2:, 1:-1, 1:-1] + weights[:, :, :-2, 1:-1, 1:-1] + weights[:, :, 1:-1, 2:, 1:-1] + weights[:, :, 1:-1, :-2, 1:-1]
                + weights[:, :, 1:-1, 1:-1, 2:] + weights[:, :, 1:-1, 1:-1, :-2]) / 6.0
        weights[:, :, 1:-1, 1:-1, 1:-1] = (inner - mean) * SMOOTH_KEEP + mean
        weights = weights / weights.sum(1, keepdim=True)
    return weights


@torch.no_grad()
def query_weights(x: Tensor, smpl_verts: Tensor, smpl_weights: Tensor, resolution_dhw: Sequence[int], K: int = K_NEIGHBOURS,
                  smooth_iters: int = SMOOTH_ITERS, clamp: Tuple[float, float] = CLAMP) -> Tensor:
    """``x``: [B, d*h*w, 3] voxel centres (x fastest), ``smpl_verts``: [B,V,3], ``smpl_weights``: [B,V,J], all on the device.
    Returns the [B,J,d,h,w] float32 field, detached."""
    d, h, w = (int(v) for v in resolution_dhw)
    B, J = x.shape[0], smpl_weights.shape[-1]
    if x.shape[1] != d * h * w:
        raise ValueError(f"x holds {x.shape[1]} points, the grid {d} x {h} x {w} = {d * h * w}")
    blend = p3d.knn_blend(x, smpl_verts, smpl_weights, K, clamp)
    return relax(blend.permute(0, 2, 1).reshape(B, J, d, h, w), smooth_iters).detach()


def _query_weights_smpl(self, x, smpl_verts, smpl_weights):
    """``VoxelDeformer._query_weights_smpl`` under its name, arguments and return."""
    if not x.is_cuda:
        return getattr(type(self), FORMER)(self, x, smpl_verts, smpl_weights)
    return query_weights(x, smpl_verts.detach(), smpl_weights, self.resolution_dhw)


_SEAM = Seam()


def install(cls) -> None:
    """Sets ``cls._query_weights_smpl`` (the reference's ``models.modules.VoxelDeformer``); the class's own method stays reachable as
    ``cls._query_weights_smpl_torch`` and serves CPU tensors."""
    _SEAM.install(cls, {"_query_weights_smpl": _query_weights_smpl}, reference=FORMER)


def uninstall(*classes) -> None:
    """Puts back what ``install`` replaced (no class given: on every installed one)."""
    _SEAM.uninstall(*classes)
