"""Pose transform of the node classes as fused HIP ops (csrc/nodes.hip through ``bds_node_pose_fwd / _bwd``).

Reference: ``RigidNodes`` (vehicles) and ``DeformableNodes`` (pedestrians, cyclists) move their points from instance-local space into
the world in ``get_gaussians`` (models/nodes/rigid.py:385-493, models/nodes/deformable.py:49-114): ``transform_means``,
``transform_quats``, the ``instances_fv`` opacity mask and the activations, then a NaN / Inf scan of the five tensors.

* ``pose_transform(...)`` is the autograd op: world means, world quaternions and masked opacities in one launch; the backward is one
  launch for the point gradients and the per-wave instance sums plus one fixed-order reduce (deterministic instance gradients).
* ``install(cls)`` / ``uninstall(cls)`` swap ``get_gaussians`` on the reference's own ``RigidNodes`` / ``DeformableNodes``.  The
  classes keep their parameters, ``get_deformation`` (and with it ``deform.install``), SH colours and scales; CPU tensors keep the
  class's own method.  Nothing is installed by default.
* ``framework_transform(...)`` is the same expression as framework ops (tests, and the A side of scripts/node_pose_time.py)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from . import gs_ops
from ._patch import Seam

GS_KEYS = ("_means", "_opacities", "_rgbs", "_scales", "_quats")   # the order of get_gaussians' dict and of its NaN / Inf check


def interpolates(in_test_set: bool, cur_frame: int, num_frames: int) -> bool:
    """The test-set form's condition (rigid.py:392-394): ``cur_frame - 1 > 0`` (not ``>= 0``) and ``cur_frame + 1 < num_frames``."""
    return bool(in_test_set) and cur_frame - 1 > 0 and cur_frame + 1 < num_frames


def _normalize(q: Tensor) -> Tensor:
    return q / q.norm(dim=-1, keepdim=True)


def quat_mult(a: Tensor, b: Tensor) -> Tensor:
    """Hamilton product of {w, x, y, z} rows (models/gaussians/basics.py:64-74)."""
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_to_rotmat(q: Tensor) -> Tensor:
    """gsplat's normalising quaternion -> rotation matrix, [..., 4] -> [..., 3, 3]."""
    w, x, y, z = _normalize(q).unbind(-1)
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def interpolate_quats(q1: Tensor, q2: Tensor) -> Tensor:
    """interpolate_quats(q1, q2, 0.5) (models/gaussians/basics.py:17-45) without its in-place edits: slerp of the normalised rows,
    q2 negated where dot < 0, lerp where dot > 0.9995; not normalised."""
    q1, q2 = _normalize(q1), _normalize(q2)
    dot = (q1 * q2).sum(-1).clamp(-1, 1)
    neg = dot < 0
    q2 = torch.where(neg[:, None], -q2, q2)
    dot = torch.where(neg, -dot, dot)
    lerp = q1 + 0.5 * (q2 - q1)
    th0 = torch.acos(dot)
    th = th0 * 0.5
    s1 = torch.cos(th) - dot * torch.sin(th) / torch.sin(th0)
    s2 = torch.sin(th) / torch.sin(th0)
    slerp = s1[:, None] * q1 + s2[:, None] * q2
    return torch.where((dot > 0.9995)[:, None], lerp, slerp)


def framework_transform(means: Tensor, quats: Tensor, logits: Tensor, point_ids: Tensor, instances_quats: Tensor,
                        instances_trans: Tensor, instances_fv: Tensor, cur_frame: int, interpolate: bool = False):
    """The pose transform as framework ops (rigid.py:28-32, 385-471): (world_means [N,3], world_quats [N,4], opacities [N,1])."""
    ids = point_ids[..., 0] if point_ids.dim() == 2 else point_ids
    f = cur_frame
    q_cur, t_cur = instances_quats[f], instances_trans[f]
    q_rot, t_rot = q_cur, t_cur
    if interpolate:
        ok = (instances_fv[f - 1] & instances_fv[f + 1])[:, None]
        q_rot = torch.where(ok, interpolate_quats(instances_quats[f - 1], instances_quats[f + 1]), q_cur)
        t_rot = torch.where(ok, (instances_trans[f - 1] + instances_trans[f + 1]) * 0.5, t_cur)
    rot = quat_to_rotmat(_normalize(q_rot))[ids]
    world_means = torch.bmm(rot, means.unsqueeze(-1)).squeeze(-1) + t_rot[ids]
    world_quats = _normalize(quat_mult(_normalize(q_cur[ids]), _normalize(quats)))
    opacities = torch.sigmoid(logits.reshape(-1, 1)) * instances_fv[f][ids].float().unsqueeze(-1)
    return world_means, world_quats, opacities


class _PoseTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, logits, instances_quats, instances_trans, point_ids, instances_fv, cur_frame, interpolate, bad_ids):
        L.require_gpu(means, quats, logits, point_ids, instances_quats, instances_trans, instances_fv)
        N = means.shape[0]
        F, I = instances_fv.shape
        if point_ids.dtype != torch.int64 or point_ids.numel() != N:
            raise L.BdsError(f"point_ids must be int64 [N,1] with N = {N} (got {point_ids.dtype} {tuple(point_ids.shape)})")
        assert quats.shape == (N, 4) and logits.numel() == N and instances_quats.shape == (F, I, 4) and instances_trans.shape == (F, I, 3)
        m, q, lg, iq, it = (L.f32c(t.detach()) for t in (means, quats, logits, instances_quats, instances_trans))
        lg = lg.reshape(N)
        ids = point_ids.detach().reshape(N).contiguous()
        fv = instances_fv.detach().contiguous().to(torch.bool).view(torch.uint8)
        dev = means.device
        wm, wq, op = torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, 1, device=dev)
        L.check(L.lib().bds_node_pose_fwd(N, F, I, int(cur_frame), int(interpolate), L.ptr(m), L.ptr(q), L.ptr(lg), L.ptr(ids), L.ptr(iq),
                                          L.ptr(it), L.ptr(fv), L.ptr(wm), L.ptr(wq), L.ptr(op), L.ptr(bad_ids), L.stream()),
                "bds_node_pose_fwd")
        ctx.save_for_backward(m, q, lg, ids, iq, fv)
        ctx.cfg = (int(cur_frame), bool(interpolate), tuple(logits.shape))
        return wm, wq, op

    @staticmethod
    def backward(ctx, v_wm, v_wq, v_op):
        m, q, lg, ids, iq, fv = ctx.saved_tensors
        f, interp, lshape = ctx.cfg
        if interp:
            raise RuntimeError("bilateral_driving_amd.nodes.pose_transform: no gradient in the interpolated (test-set) mode -- the "
                               "reference's interpolate_quats edits a tensor in place and its autograd cannot differentiate it either")
        N = m.shape[0]
        F, I = fv.shape
        dev = m.device
        v_iq, v_it = torch.zeros(F, I, 4, device=dev), torch.zeros(F, I, 3, device=dev)
        if N == 0:
            return torch.zeros_like(m), torch.zeros_like(q), torch.zeros(lshape, device=dev), v_iq, v_it, None, None, None, None, None
        v_wm = torch.zeros(N, 3, device=dev) if v_wm is None else v_wm.contiguous().float()
        v_wq = torch.zeros(N, 4, device=dev) if v_wq is None else v_wq.contiguous().float()
        v_op = torch.zeros(N, device=dev) if v_op is None else v_op.contiguous().float().reshape(N)
        v_m, v_q, v_l = torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, device=dev)
        nb = int(L.lib().bds_node_pose_bwd_temp_bytes(N, I))
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        L.check(L.lib().bds_node_pose_bwd(N, F, I, f, L.ptr(m), L.ptr(q), L.ptr(lg), L.ptr(ids), L.ptr(iq), L.ptr(fv), L.ptr(v_wm),
                                          L.ptr(v_wq), L.ptr(v_op), L.ptr(v_m), L.ptr(v_q), L.ptr(v_l), L.ptr(v_iq), L.ptr(v_it),
                                          L.ptr(temp), nb, L.stream()), "bds_node_pose_bwd")
        return v_m, v_q, v_l.reshape(lshape), v_iq, v_it, None, None, None, None, None


def pose_transform(means: Tensor, quats: Tensor, logits: Tensor, point_ids: Tensor, instances_quats: Tensor, instances_trans: Tensor,
                   instances_fv: Tensor, cur_frame: int, interpolate: bool = False,
                   flags: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(world_means [N,3], world_quats [N,4], opacities [N,1]) of means [N,3], quats [N,4] (raw), logits [N,1], point_ids int64 [N,1]
    and the instance tables [F,I,4] / [F,I,3] / [F,I] (bool) at ``cur_frame``; ``interpolate``: the test-set form (``interpolates``),
    forward only.  An id outside [0, I) is never read: with ``flags`` (int32 [2] on the device, zeroed by the caller) it raises
    ``flags[1]`` for the caller's own read-back; without, this call reads the flag back itself and raises ``IndexError``."""
    own = flags is None
    bad = torch.zeros(1, dtype=torch.int32, device=means.device) if own else flags[1:2]
    if own:
        L.require_gpu(means)
    out = _PoseTransform.apply(means, quats, logits, instances_quats, instances_trans, point_ids, instances_fv, cur_frame, interpolate, bad)
    if own and means.shape[0] and int(bad.item()):
        raise IndexError(f"point_ids holds an instance id outside [0, {instances_fv.shape[1]})")
    return out


# ---- get_gaussians of the reference's node classes ----------------------------------------------------------------------------------
def _finite_check(self, gs: dict, flags: Tensor) -> None:
    """The reference's NaN / Inf scan (rigid.py:475-480) as one launch; its flag word and the bad-id word come back in one read."""
    ts = [gs[k] for k in GS_KEYS]
    ptrs = (L.C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    cnts = (L.C.c_int64 * len(ts))(*[t.numel() for t in ts])
    L.check(L.lib().bds_nonfinite_flags(len(ts), ptrs, cnts, None, flags.data_ptr(), None, L.stream()), "bds_nonfinite_flags")
    word, bad = (int(v) for v in flags.cpu())
    if bad:
        raise IndexError(f"point_ids holds an instance id outside [0, {self.instances_fv.shape[1]})")
    for i, k in enumerate(GS_KEYS):
        if word >> i & 1:
            kind = "NaN" if bool(torch.isnan(gs[k]).any()) else "Inf"
            raise ValueError(f"{kind} detected in gaussian {k} at step {self.step}")


def _node_gaussians(self, cam, means: Tensor, quats: Tensor, scales: Tensor) -> dict:
    self.filter_mask = torch.ones_like(self._means[:, 0], dtype=torch.bool)   # (all true: the tensors below are returned whole)
    fv = self.instances_fv
    flags = torch.zeros(2, dtype=torch.int32, device=means.device)
    interp = interpolates(getattr(self, "in_test_set", False), self.cur_frame, fv.shape[0])
    world_means, world_quats, opacities = pose_transform(means, quats, self._opacities, self.point_ids, self.instances_quats,
                                                         self.instances_trans, fv, self.cur_frame, interp, flags=flags)
    colors = torch.cat((self._features_dc[:, None, :], self._features_rest), dim=1)
    if self.sh_degree > 0:
        viewdirs = world_means.detach() - cam.camtoworlds.data[..., :3, 3]
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        n = min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree)
        rgbs = torch.clamp(gs_ops.spherical_harmonics(n, viewdirs, colors) + 0.5, 0.0, 1.0)
    else:
        rgbs = torch.sigmoid(colors[:, 0, :])
    gs = dict(_means=world_means, _opacities=opacities, _rgbs=rgbs, _scales=scales, _quats=world_quats)
    _finite_check(self, gs, flags)
    return gs


def rigid_get_gaussians(self, cam) -> dict:
    """``RigidNodes.get_gaussians`` (rigid.py:445-493) on the fused transform."""
    if not self._means.is_cuda:
        return type(self)._bds_reference_get_gaussians(self, cam)
    scales = self.get_scaling
    gs = _node_gaussians(self, cam, self._means, self._quats, scales)
    self._gs_cache = {"_scales": scales}
    return gs


def deformable_get_gaussians(self, cam) -> dict:
    """``DeformableNodes.get_gaussians`` (deformable.py:49-114) on the fused transform; the deformation network is the class's own
    ``get_deformation`` (fused too under ``deform.install``)."""
    if not self._means.is_cuda:
        return type(self)._bds_reference_get_gaussians(self, cam)
    delta_xyz = delta_quat = delta_scale = None
    if self.ctrl_cfg.use_deformgs_for_nonrigid and self.step > self.ctrl_cfg.use_deformgs_after:
        delta_xyz, delta_quat, delta_scale = self.get_deformation(local_means=self._means)
    if delta_xyz is not None:
        means = (self._means.data if self.ctrl_cfg.stop_optimizing_canonical_xyz else self._means) + delta_xyz
    else:
        means = self._means
    quats = self.get_quats + delta_quat if delta_quat is not None else self._quats
    scales = self.get_scaling + delta_scale if delta_scale is not None else self.get_scaling
    gs = _node_gaussians(self, cam, means, quats, scales)
    self._gs_cache = {"_scales": scales, "local_xyz_deformed": means if delta_xyz is not None else None}
    return gs


_SEAM = Seam()


def install(node_class) -> None:
    """``install(models.nodes.RigidNodes)`` / ``install(models.nodes.DeformableNodes)``: the class's ``get_gaussians`` becomes the fused
    one (a class with ``get_deformation`` gets the deformable form).  The original stays reachable as
    ``node_class._bds_reference_get_gaussians``; ``uninstall`` puts it back."""
    fn = deformable_get_gaussians if hasattr(node_class, "get_deformation") else rigid_get_gaussians
    _SEAM.install(node_class, {"get_gaussians": fn}, reference="_bds_reference_get_gaussians")


def uninstall(*node_classes) -> None:
    _SEAM.uninstall(*node_classes)
