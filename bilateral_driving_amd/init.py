"""Scene initialisation on the device (csrc/knn.hip through ``bds_knn_self``): the exact K nearest neighbours of every point of a
cloud among the other points of the same cloud, and the Gaussians' initial parameters from them.

Reference: every Gaussian class takes its initial scales from the mean distance to each point's three nearest neighbours, through
``k_nearest_sklearn`` (models/gaussians/basics.py:208-224: sklearn's kd-tree on the host over the whole cloud, k + 1 neighbours, the
first column dropped) in ``create_from_pcd`` (vanilla.py:79-105) and the rigid nodes' initialiser (nodes/rigid.py:113-120).

* ``k_nearest(x, k)``: distances [N,k] float32 (ascending) and rows [N,k] int64 as device tensors.
* ``init_scales(means, k=3, dims=3, clamp=None)``: the [N,dims] log-scales, from the search's fused epilogue.
* ``k_nearest_sklearn(x, k)``: the reference's name and return convention (two float32 numpy arrays, one read-back);
  ``install(*modules)`` sets it on the reference's modules that bound the name through ``from ...basics import *``
  (``models.gaussians.vanilla``, ``models.nodes.rigid``), ``uninstall`` puts the former functions back.
* ``create_from_pcd(self, init_means, init_colors)``: vanilla.py:79-105 with everything on the device; ``rigid_init_scales`` the
  scale step of rigid.py:113-119, with its clamp.

One deviation: a point is never its own neighbour here (the query is excluded by row), so the rows never hold the query itself.
sklearn's can -- among exact duplicates it drops whichever of them the tree returned first.  The distances are the same either way,
and the reference discards the rows.

Not covered here: K > 8 and queries of one cloud against another.  Those are ``p3d.knn_points`` (pytorch3d's ``knn_points`` of the
SMPL classes: batched, K up to 32, cross-cloud, the query included; brute force) and, for evaluation's K = 1 over large clouds,
``geometry.chamfer_distance``."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor
from torch.nn import Parameter

from . import _lib as L
from ._patch import Seam

MAX_K = 8                   # include/bds.h BDS_KNN_MAX_K
MAX_POINTS = 1 << 30        # include/bds.h BDS_KNN_MAX_POINTS
QUERY_BLOCK = 256           # include/bds.h BDS_KNN_QUERY_BLOCK: queries per workgroup of the brute-force fallback
TARGET_TILE = 512           # include/bds.h BDS_KNN_TARGET_TILE: records per LDS tile of the fallback
RING_MAX = 2                # include/bds.h BDS_KNN_RING_MAX: rings of cells a query walks before the fallback takes it
STATS_WORDS = 32            # include/bds.h BDS_KNN_STATS_WORDS and the BDS_KNN_STAT_* offsets
STAT_EDGE, STAT_DIMS, STAT_UNRESOLVED, STAT_LO, STAT_HI, STAT_CELLS, STAT_CLOUD_LO, STAT_CLOUD_HI = 0, 3, 6, 7, 10, 13, 14, 17
RIGID_CLAMP = (0.002, 100.0)      # rigid.py:118
SH_C0 = 0.28209479177387814       # basics.py:80


def _cloud(x: Tensor, k: int) -> Tensor:
    """The checks sklearn makes on the host, then ``x`` as a contiguous float32 [N,3] device tensor.  One read-back (the flag word
    of ``bds_nonfinite_flags``)."""
    if not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"the cloud must be [N,3], got {tuple(x.shape)}")
    N = x.shape[0]
    if N < k + 1:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k + 1}, n_samples_fit = {N}")
    if N > MAX_POINTS:
        raise ValueError(f"the cloud holds {N} points, more than {MAX_POINTS}")
    L.require_gpu(x)
    x = x.detach().float().contiguous()
    flags = torch.zeros(1, dtype=torch.int32, device=x.device)
    ptrs = (L.C.c_void_p * 1)(x.data_ptr())
    cnts = (L.C.c_int64 * 1)(x.numel())
    L.check(L.lib().bds_nonfinite_flags(1, ptrs, cnts, None, flags.data_ptr(), None, L.stream()), "bds_nonfinite_flags")
    if int(flags.item()):
        raise ValueError("Input X contains NaN or infinity.")
    return x


def _search(x: Tensor, k: int, want_idx: bool, scale_dims: int = 0, clamp: Optional[Tuple[float, float]] = None):
    """``x``: checked by ``_cloud``.  -> (dist [N,k], idx [N,k] int32 or None, log_scales [N,scale_dims] or None, workspace)."""
    N = x.shape[0]
    lib = L.lib()
    ws = torch.empty(max(int(lib.bds_knn_workspace_bytes(N)), 16), dtype=torch.uint8, device=x.device)
    dist = torch.empty(N, k, dtype=torch.float32, device=x.device)
    idx = torch.empty(N, k, dtype=torch.int32, device=x.device) if want_idx else None
    scales = torch.empty(N, scale_dims, dtype=torch.float32, device=x.device) if scale_dims else None
    lo, hi = (0.0, math.inf) if clamp is None else (float(clamp[0]), float(clamp[1]))
    L.check(lib.bds_knn_self(N, L.ptr(x), k, L.ptr(dist), L.ptr(idx), L.ptr(scales), scale_dims, lo, hi, L.ptr(ws), ws.numel(), L.stream()),
            "bds_knn_self")
    return dist, idx, scales, ws


def _stats(ws: Tensor) -> Dict[str, object]:
    """The stats block at the head of the workspace (one read-back)."""
    words = ws[:4 * STATS_WORDS].cpu()
    f, i = words.view(torch.float32).tolist(), words.view(torch.int32).tolist()
    return {"cell_edge": f[STAT_EDGE], "dims": tuple(i[STAT_DIMS:STAT_DIMS + 3]), "unresolved": i[STAT_UNRESOLVED],
            "lo": tuple(f[STAT_LO:STAT_LO + 3]), "hi": tuple(f[STAT_HI:STAT_HI + 3]), "cells": i[STAT_CELLS],
            "cloud_lo": tuple(f[STAT_CLOUD_LO:STAT_CLOUD_LO + 3]), "cloud_hi": tuple(f[STAT_CLOUD_HI:STAT_CLOUD_HI + 3])}


@torch.no_grad()
def k_nearest(x: Tensor, k: int, return_indices: bool = True, return_stats: bool = False):
    """``x``: [N,3] float32 on the device, finite, N >= k + 1; ``k``: 1..8.  Returns the distances [N,k] float32, ascending, and (with
    ``return_indices``) the neighbours' rows [N,k] int64, both on the device; with ``return_stats`` also a dict read back from the
    search's stats block: ``cell_edge``, ``dims`` (cells per axis), ``unresolved`` (the queries the brute-force fallback took), ``lo``,
    ``hi`` (the grid's box: the cloud's with at most N / 128 points trimmed beyond each face), ``cells``, ``cloud_lo``, ``cloud_hi``.
    Exact: candidates are ordered by (squared distance in float32, row), the query's own row excluded, whatever the order of
    evaluation.  ValueError for N < k + 1 and for a NaN / Inf coordinate, as sklearn; BdsError for a CPU tensor."""
    x = _cloud(x, k)
    dist, idx, _, ws = _search(x, k, return_indices)
    out = (dist, idx.long()) if return_indices else (dist,)
    if return_stats:
        out = out + (_stats(ws),)
    return out if len(out) > 1 else out[0]


@torch.no_grad()
def init_scales(means: Tensor, k: int = 3, dims: int = 3, clamp: Optional[Tuple[float, float]] = None) -> Tensor:
    """[N,dims] float32: every column log(mean distance to the ``k`` nearest other points) -- vanilla.py:82-92 for ``dims`` 3, 2
    (gaussian_2d) and 1 (ball_gaussians); a point with ``k`` duplicates gets -inf, as there.  ``clamp=(lo, hi)`` clamps the mean
    first (rigid.py:118: ``RIGID_CLAMP``)."""
    if dims not in (1, 2, 3):
        raise ValueError(f"dims must be 1, 2 or 3, got {dims!r}")
    if clamp is not None and not float(clamp[0]) <= float(clamp[1]):
        raise ValueError(f"clamp must be (lo, hi) with lo <= hi, got {clamp!r}")
    return _search(_cloud(means, k), k, False, dims, clamp)[2]


def rigid_init_scales(means: Tensor) -> Tensor:
    """rigid.py:115-119: the [N,3] log-scales of the rigid nodes' points, the mean distance clamped to (0.002, 100)."""
    return init_scales(means, 3, 3, RIGID_CLAMP)


def k_nearest_sklearn(x: Tensor, k: int):
    """basics.py:208-224 under its name and return convention: (distances [N,k], rows [N,k]) as float32 numpy arrays.  ``x`` may
    live on the host, as the reference passes whatever device its means are on; the search runs on the current GPU."""
    import numpy as np
    if not x.is_cuda:
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    dist, idx = k_nearest(x, k)
    both = torch.cat((dist, idx.float()), dim=1).cpu().numpy()      # (float32 rows, as the reference casts them; one read-back)
    return np.ascontiguousarray(both[:, :k]), np.ascontiguousarray(both[:, k:])


def random_quat_tensor(N: int) -> Tensor:
    """basics.py:47-62: three ``torch.rand(N)`` from the CPU generator in the reference's order, so a seed gives its quaternions."""
    u, v, w = torch.rand(N), torch.rand(N), torch.rand(N)
    return torch.stack([torch.sqrt(1 - u) * torch.sin(2 * math.pi * v), torch.sqrt(1 - u) * torch.cos(2 * math.pi * v),
                        torch.sqrt(u) * torch.sin(2 * math.pi * w), torch.sqrt(u) * torch.cos(2 * math.pi * w)], dim=-1)


def create_from_pcd(self, init_means: Tensor, init_colors: Tensor) -> None:
    """vanilla.py:79-105 for ``VanillaGaussians`` (and the classes that inherit it): sets ``_means`` [N,3], ``_scales`` [N,3]
    ([N,2] with ``self.gaussian_2d``, [N,1] with ``self.ball_gaussians``), ``_quats`` [N,4], ``_features_dc`` [N,3],
    ``_features_rest`` [N, (sh_degree + 1)^2 - 1, 3] and ``_opacities`` [N,1] as float32 Parameters on ``self.device``.  The neighbour
    search and the scales stay on the device; the quaternions are drawn as the reference draws them."""
    device = torch.device(self.device)
    means = init_means.to(device)
    self._means = Parameter(means)
    dims = 1 if getattr(self, "ball_gaussians", False) else (2 if getattr(self, "gaussian_2d", False) else 3)
    self._scales = Parameter(init_scales(self._means.data, 3, dims))
    N = means.shape[0]
    self._quats = Parameter(random_quat_tensor(N).to(device))
    sh_degree = int(self.sh_degree)
    dim_sh = (sh_degree + 1) ** 2
    colors = init_colors.to(device)
    shs = torch.zeros((N, dim_sh, 3), dtype=torch.float32, device=device)
    if sh_degree > 0:
        shs[:, 0, :3] = (colors - 0.5) / SH_C0           # RGB2SH, basics.py:76-81
    else:
        shs[:, 0, :3] = torch.logit(colors, eps=1e-10)
    self._features_dc = Parameter(shs[:, 0, :])
    self._features_rest = Parameter(shs[:, 1:, :])
    self._opacities = Parameter(torch.logit(0.1 * torch.ones(N, 1, device=device)))


_SEAM = Seam()


def install(*modules) -> None:
    """Sets ``k_nearest_sklearn`` on each module.  The reference's ``models.gaussians.vanilla`` and ``models.nodes.rigid`` bind the
    name at import through ``from models.gaussians.basics import *``, so those are the modules to pass (``basics`` itself changes
    nothing for them)."""
    for m in modules:
        _SEAM.install(m, {"k_nearest_sklearn": k_nearest_sklearn})


def uninstall(*modules) -> None:
    """Puts back what ``install`` replaced (no module given: on every installed one)."""
    _SEAM.uninstall(*modules)
