"""What the reference takes from pytorch3d, which has no ROCm build: ``knn_points`` on the device (csrc/knn_cross.hip through
``bds_cross_knn``) and the rotation conversions ``matrix_to_quaternion``, ``quaternion_to_matrix``, ``axis_angle_to_matrix`` and
``standardize_quaternion`` in plain torch.  ``dropin/pytorch3d`` re-exports them under pytorch3d's module paths.

Reference call sites: ``knn_points(x, smpl_verts, K=30)`` in ``VoxelDeformer._query_weights_smpl`` (models/modules.py:1199),
``knn_points(x, x, K=3, return_nn=False)`` in ``SMPLNodes.update_knn`` (models/nodes/smpl.py:186), ``knn_points(_x, _y, norm=norm,
K=1)`` in utils/chamfer_distance.py:45-46; ``matrix_to_quaternion`` in models/nodes/smpl.py:331, rigid.py:187, human_body.py:237 and
six dataset loaders, ``quaternion_to_matrix`` and ``axis_angle_to_matrix`` in human_body.py:12-16 and datasets/tools/postprocess.py:6.

* ``knn_points``: exact, brute force, forward only on the device.  ``dists`` is the SQUARED distance for ``norm=2`` (as pytorch3d)
  from the float32 coordinate differences, ``(dx*dx + dy*dy) + dz*dz`` with every operation rounded on its own; candidates are ordered
  by (value, row of ``p2``), so the row decides ties.  The query is not excluded.  Slots beyond ``lengths2`` and rows beyond
  ``lengths1`` hold zeros.  D = 3 and K <= 32 only.  Where an input requires grad the values are formed again from the rows by torch
  ops, which gives pytorch3d's gradient.  CPU tensors (the dataset loaders, the CPU tests) run a chunked torch formulation with the
  same value expression, order and padding.
* ``knn_blend``: the search with the fused epilogue ``sum_k (w_k / sum w) feat[idx_k]``, ``w_k = 1 / clamp(sqrt(d2_k), lo, hi)``
  (models/modules.py:1200-1206 without its [B,P1,K,J] gather).
* the rotation conversions follow pytorch3d's published behaviour, real part first; ``matrix_to_quaternion`` picks the
  best-conditioned of its four candidates and returns the quaternion with a non-negative real part (the convention of pytorch3d's
  current code; earlier releases left the sign to the candidate).

Unverified against pytorch3d itself: it is not installed anywhere this project runs."""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L

MAX_K = 32                  # include/bds.h BDS_KNN_CROSS_MAX_K
MAX_J = 64                  # include/bds.h BDS_KNN_CROSS_MAX_J
QUERY_BLOCK = 256           # include/bds.h BDS_KNN_CROSS_QUERY_BLOCK: queries of one cloud per workgroup
TARGET_TILE = 512           # include/bds.h BDS_KNN_CROSS_TARGET_TILE: candidate records per LDS tile
DIM = 3
CPU_CHUNK_ELEMS = 1 << 22   # distances formed at a time by the CPU formulation

KNN = namedtuple("KNN", "dists idx knn")


# ---- knn_points ------------------------------------------------------------------------------------------------------------------
def _check(p1: Tensor, p2: Tensor, lengths1, lengths2, norm: int, K: int) -> None:
    if p1.dim() != 3 or p2.dim() != 3:
        raise ValueError(f"p1 and p2 must be [B,P,{DIM}], got {tuple(p1.shape)} and {tuple(p2.shape)}")
    if p1.shape[2] != DIM or p2.shape[2] != DIM:
        raise ValueError(f"knn_points here searches D = {DIM} only, got D = {p1.shape[2]} and {p2.shape[2]}")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError(f"pts1 and pts2 must have the same batch dimension, got {p1.shape[0]} and {p2.shape[0]}")
    if not isinstance(K, int) or not 1 <= K <= MAX_K:
        raise ValueError(f"K must be an integer in 1..{MAX_K}, got {K!r}")
    if norm not in (1, 2):
        raise ValueError(f"Support norm 1 or 2 only, got {norm!r}")
    if p1.is_cuda != p2.is_cuda:
        raise ValueError(f"p1 is on {p1.device} and p2 on {p2.device}")
    for name, n in (("lengths1", lengths1), ("lengths2", lengths2)):
        if n is not None and tuple(n.shape) != (p1.shape[0],):
            raise ValueError(f"{name} must be [{p1.shape[0]}], got {tuple(n.shape)}")


def _value(diff: Tensor, norm: int) -> Tensor:
    """The search's value of coordinate differences [...,3], in the kernel's order of operations."""
    if norm == 2:
        return (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    return (diff[..., 0].abs() + diff[..., 1].abs()) + diff[..., 2].abs()


def _lengths(n: Optional[Tensor], B: int, cap: int, device) -> Tensor:
    if n is None:
        return torch.full((B,), cap, dtype=torch.int64, device=device)
    return n.to(device=device, dtype=torch.int64).clamp(0, cap)


def _slot_mask(len1: Tensor, len2: Tensor, P1: int, K: int) -> Tensor:
    """[B,P1,K] bool: the slots that hold a neighbour."""
    dev = len1.device
    rows = torch.arange(P1, device=dev)[None, :, None] < len1[:, None, None]
    slots = torch.arange(K, device=dev)[None, None, :] < len2[:, None, None]
    return rows & slots


@torch.no_grad()
def _search_cpu(p1: Tensor, p2: Tensor, len1: Tensor, len2: Tensor, norm: int, K: int) -> Tuple[Tensor, Tensor]:
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dists = p1.new_zeros(B, P1, K)
    idx = torch.zeros(B, P1, K, dtype=torch.int64, device=p1.device)
    k = min(K, P2)
    if B == 0 or P1 == 0 or k == 0:
        return dists, idx
    beyond = torch.arange(P2, device=p1.device)[None, None, :] >= len2[:, None, None]
    step = max(1, CPU_CHUNK_ELEMS // max(B * P2, 1))
    for s in range(0, P1, step):
        v = _value(p1[:, s:s + step, None, :] - p2[:, None, :, :], norm).masked_fill(beyond, float("inf"))
        sv, si = torch.sort(v, dim=-1, stable=True)       # equal values keep the order of their rows
        dists[:, s:s + step, :k] = sv[..., :k]
        idx[:, s:s + step, :k] = si[..., :k]
    mask = _slot_mask(len1, len2, P1, K)
    return torch.where(mask, dists, torch.zeros_like(dists)), torch.where(mask, idx, torch.zeros_like(idx))


@torch.no_grad()
def _search_gpu(p1: Tensor, p2: Tensor, lengths1, lengths2, norm: int, K: int, want_dists: bool, want_idx: bool, feat: Optional[Tensor] = None,
                clamp: Tuple[float, float] = (1.0, 1.0)):
    """-> (dists or None, idx or None, blend or None); the inputs are checked, float32, contiguous and on the current GPU."""
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dev = p1.device
    len1 = None if lengths1 is None else lengths1.to(device=dev, dtype=torch.int64).contiguous()
    len2 = None if lengths2 is None else lengths2.to(device=dev, dtype=torch.int64).contiguous()
    dists = torch.empty(B, P1, K, dtype=torch.float32, device=dev) if want_dists else None
    idx = torch.empty(B, P1, K, dtype=torch.int64, device=dev) if want_idx else None
    J = 0 if feat is None else feat.shape[2]
    blend = None if feat is None else torch.empty(B, P1, J, dtype=torch.float32, device=dev)
    if B * P1 == 0:      # (no query: the outputs have no element, and an empty tensor has no address to hand over)
        return dists, idx, blend
    L.check(L.lib().bds_cross_knn(B, P1, P2, L.ptr(p1), L.ptr(p2), L.ptr(len1), L.ptr(len2), K, norm, L.ptr(dists), L.ptr(idx), L.ptr(feat), J,
                                  float(clamp[0]), float(clamp[1]), L.ptr(blend), L.stream()), "bds_cross_knn")
    return dists, idx, blend


def _gather_rows(p2: Tensor, idx: Tensor) -> Tensor:
    """[B,P1,K,D]: the rows ``idx`` [B,P1,K] of ``p2`` [B,P2,D] (a padding slot gathers row 0)."""
    B, P1, K = idx.shape
    if p2.shape[1] == 0:
        return p2.new_zeros(B, P1, K, p2.shape[2])
    return p2.gather(1, idx.reshape(B, P1 * K, 1).expand(-1, -1, p2.shape[2])).reshape(B, P1, K, p2.shape[2])


def knn_points(p1: Tensor, p2: Tensor, lengths1: Optional[Tensor] = None, lengths2: Optional[Tensor] = None, norm: int = 2, K: int = 1,
               version: int = -1, return_nn: bool = False, return_sorted: bool = True) -> KNN:
    """pytorch3d.ops.knn_points for D = 3 and K <= 32: ``(dists [B,P1,K] float32, idx [B,P1,K] int64, knn [B,P1,K,3] or None)``, the
    K nearest rows of ``p2[b]`` for every row of ``p1[b]``, ascending.  ``version`` is ignored, and the result is sorted whatever
    ``return_sorted`` says.  ValueError for D != 3, a batch mismatch, K outside 1..32, a norm other than 1 or 2 and tensors on
    different kinds of device."""
    _check(p1, p2, lengths1, lengths2, norm, K)
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    if p1.is_cuda:
        L.require_gpu(p1, p2)
        a, b = L.f32c(p1.detach()), L.f32c(p2.detach())
        dists, idx, _ = _search_gpu(a, b, lengths1, lengths2, norm, K, True, True)
    else:
        a, b = p1.detach(), p2.detach().to(p1.dtype)
        dists, idx = _search_cpu(a, b, _lengths(lengths1, B, P1, p1.device), _lengths(lengths2, B, P2, p1.device), norm, K)
    needs_grad = torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad)
    nn = _gather_rows(p2, idx) if (return_nn or needs_grad) else None
    if needs_grad:      # the same values again as torch ops on the chosen rows: autograd then gives pytorch3d's gradient
        mask = _slot_mask(_lengths(lengths1, B, P1, p1.device), _lengths(lengths2, B, P2, p1.device), P1, K)
        dists = torch.where(mask, _value(p1[:, :, None, :] - nn, norm), torch.zeros((), dtype=dists.dtype, device=dists.device))
    return KNN(dists, idx, nn if return_nn else None)


def knn_blend(p1: Tensor, p2: Tensor, feat: Tensor, K: int, clamp: Tuple[float, float], lengths1: Optional[Tensor] = None,
              lengths2: Optional[Tensor] = None) -> Tensor:
    """[B,P1,J] float32 on the device: for every row of ``p1[b]`` the blend ``sum_k (w_k / sum w) feat[b, idx_k]`` over its K nearest
    rows of ``p2[b]``, ``w_k = 1 / clamp(distance_k, lo, hi)`` -- models/modules.py:1199-1206 in one launch, without the indices and
    without the [B,P1,K,J] gather.  ``feat``: [B,P2,J], J <= 64.  Forward only."""
    _check(p1, p2, lengths1, lengths2, 2, K)
    if feat.dim() != 3 or feat.shape[:2] != p2.shape[:2] or not 1 <= feat.shape[2] <= MAX_J:
        raise ValueError(f"feat must be [{p2.shape[0]},{p2.shape[1]},J] with J in 1..{MAX_J}, got {tuple(feat.shape)}")
    if not 0.0 < float(clamp[0]) <= float(clamp[1]):
        raise ValueError(f"clamp must be (lo, hi) with 0 < lo <= hi, got {clamp!r}")
    L.require_gpu(p1, p2, feat)
    return _search_gpu(L.f32c(p1.detach()), L.f32c(p2.detach()), lengths1, lengths2, 2, K, False, False, L.f32c(feat.detach()), clamp)[2]


# ---- rotation conversions (pure torch, any device, autograd's gradients) -----------------------------------------------------------
def standardize_quaternion(quaternions: Tensor) -> Tensor:
    """The quaternion [...,4] (real part first) of the same rotation whose real part is non-negative."""
    return torch.where(quaternions[..., 0:1] < 0, -quaternions, quaternions)


def _sqrt_positive_part(x: Tensor) -> Tensor:
    """sqrt(max(0, x)) with a zero (not infinite) gradient where x <= 0."""
    pos = x > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, x, torch.ones_like(x))), torch.zeros_like(x))


def matrix_to_quaternion(matrix: Tensor) -> Tensor:
    """Rotation matrices [...,3,3] -> quaternions [...,4], real part first and non-negative.  Each of the four candidates divides by
    twice one component's magnitude; the one with the largest magnitude (at least 1/2 for a rotation) is taken, so nothing is divided
    by a small number and a half turn gives no NaN."""
    if matrix.shape[-2:] != (3, 3):
        raise ValueError(f"Invalid rotation matrix shape {tuple(matrix.shape)}.")
    batch = matrix.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(matrix.reshape(batch + (9,)), dim=-1)
    q_abs = _sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1))
    r, i, j, k = torch.unbind(q_abs * q_abs, dim=-1)
    candidates = torch.stack([torch.stack([r, m21 - m12, m02 - m20, m10 - m01], dim=-1),
                              torch.stack([m21 - m12, i, m10 + m01, m02 + m20], dim=-1),
                              torch.stack([m02 - m20, m10 + m01, j, m12 + m21], dim=-1),
                              torch.stack([m10 - m01, m20 + m02, m21 + m12, k], dim=-1)], dim=-2)          # [...,4 candidates,4]
    candidates = candidates / (2.0 * q_abs[..., None].clamp(min=0.1))
    best = q_abs.argmax(dim=-1)[..., None, None].expand(batch + (1, 4))
    return standardize_quaternion(candidates.gather(-2, best).squeeze(-2))


def quaternion_to_matrix(quaternions: Tensor) -> Tensor:
    """Quaternions [...,4], real part first, of any non-zero length -> rotation matrices [...,3,3]."""
    r, i, j, k = torch.unbind(quaternions, dim=-1)
    two_s = 2.0 / (quaternions * quaternions).sum(dim=-1)
    rows = (1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))
    return torch.stack(rows, dim=-1).reshape(quaternions.shape[:-1] + (3, 3))


def axis_angle_to_quaternion(axis_angle: Tensor) -> Tensor:
    """Axis times angle [...,3] -> unit quaternions [...,4]; below 1e-6 rad, sin(a/2)/a is its series 1/2 - a^2/48."""
    angles = torch.norm(axis_angle, p=2, dim=-1, keepdim=True)
    half = 0.5 * angles
    small = angles.abs() < 1e-6
    ratio = torch.where(small, 0.5 - angles * angles / 48.0, torch.sin(half) / torch.where(small, torch.ones_like(angles), angles))
    return torch.cat([torch.cos(half), axis_angle * ratio], dim=-1)


def axis_angle_to_matrix(axis_angle: Tensor) -> Tensor:
    """Axis times angle [...,3] -> rotation matrices [...,3,3]."""
    return quaternion_to_matrix(axis_angle_to_quaternion(axis_angle))
