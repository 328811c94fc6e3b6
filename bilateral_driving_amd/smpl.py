"""Pose chain and skinning of the SMPL nodes as fused HIP ops (csrc/smpl.hip through ``bds_smpl_skin_fwd / _bwd``).

Reference: ``SMPLNodes`` (humans) moves its 6890 points per instance from the canonical body into the world in ``get_gaussians``
(models/nodes/smpl.py:343-397): ``transform_means_and_quats`` (:267-341; ``transform_means`` for ball Gaussians) runs the template
(models/human_body.py:158-180: ``quaternion_to_matrix``, the 23-step loop of ``batch_rigid_transform``, the product with ``A0_inv``, the
5-D ``grid_sample`` of ``lbs_voxel_base + voxel_w_correction``), blends the joints' transforms per point, turns the blended (not
orthogonal) matrix into a quaternion by pytorch3d's rule and scatters the present instances' rows into zero containers.

* ``skin_transform(...)`` is the autograd op: one launch forward; backward one per-point launch (point gradients, float atomics into
  the zeroed field gradient, per-workgroup sums of the joints' gradient) and one per-instance launch (fixed-order reduce, the chain
  backward).  Pose and translation gradients are deterministic, the field gradient's summation order is not (as ``grid_sample``'s).
* ``install(cls)`` / ``uninstall(cls)`` swap ``get_gaussians`` on the reference's own ``SMPLNodes``.  CPU tensors and a template with
  ``additional_correction`` keep the class's own method.  Nothing is installed by default.
* ``framework_transform(...)`` is the same expression as framework ops (tests, and the A side of scripts/smpl_skin_time.py)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib as L
from . import gs_ops, nodes, p3d
from ._patch import Seam

JOINTS = 24
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)   # the SMPL kinematic tree


def _normalize(q: Tensor) -> Tensor:
    return q / q.norm(dim=-1, keepdim=True)


def check_parents(parents: Sequence[int]) -> Tuple[int, ...]:
    parents = tuple(int(p) for p in parents)
    if len(parents) != JOINTS or any(not 0 <= parents[j] < j for j in range(1, JOINTS)):
        raise ValueError(f"parents must hold {JOINTS} entries with 0 <= parents[j] < j for j >= 1, got {parents}")
    return parents


def frame_pose(instances_quats: Tensor, smpl_quats: Tensor, instances_trans: Tensor, instances_fv: Tensor, cur_frame: int,
               interpolate: bool) -> Tuple[Tensor, Tensor]:
    """(theta [I,24,4] raw, trans [I,3]) of the frame; ``interpolate``: smpl.py:275-286, 311-322 (``nodes.interpolate_quats`` of frames
    f-1 and f+1 and the mean translation where both frames see the instance)."""
    f = cur_frame
    theta = torch.cat((instances_quats[f], smpl_quats[f]), dim=1)
    trans = instances_trans[f]
    if interpolate:
        prev = torch.cat((instances_quats[f - 1], smpl_quats[f - 1]), dim=1)
        nxt = torch.cat((instances_quats[f + 1], smpl_quats[f + 1]), dim=1)
        ok = instances_fv[f - 1] & instances_fv[f + 1]
        inter = nodes.interpolate_quats(prev.reshape(-1, 4), nxt.reshape(-1, 4)).reshape(theta.shape)
        theta = torch.where(ok[:, None, None], inter, theta)
        trans = torch.where(ok[:, None], (instances_trans[f - 1] + instances_trans[f + 1]) * 0.5, trans)
    return theta, trans


def rigid_chain(rot_mats: Tensor, joints: Tensor, parents: Sequence[int]) -> Tensor:
    """``batch_rigid_transform``'s rel_transforms (lbs.py:362-418): [B,24,3,3], [B,24,3] -> [B,24,4,4]."""
    B = rot_mats.shape[0]
    par = torch.as_tensor(list(parents[1:]), dtype=torch.long, device=joints.device)
    rel = torch.cat((joints[:, :1], joints[:, 1:] - joints[:, par]), dim=1)
    top = torch.cat((rot_mats, rel[..., None]), dim=-1)                                       # [B,24,3,4]
    bottom = top.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(B, JOINTS, 1, 4)
    local = torch.cat((top, bottom), dim=-2)
    chain = [local[:, 0]]
    for j in range(1, JOINTS):
        chain.append(torch.matmul(chain[parents[j]], local[:, j]))
    world = torch.stack(chain, dim=1)
    moved = torch.matmul(world, F.pad(joints[..., None], [0, 0, 0, 1]))                       # [B,24,4,1]
    return world - F.pad(moved, [3, 0])


def normalize_coords(x: Tensor, offset: Tensor, scale: Tensor, ratio: float, ratio_dim: int) -> Tensor:
    """``VoxelDeformer.normalize`` (modules.py:1183-1188) without its in-place edits."""
    n = (x - offset) / scale
    k = ratio_dim % 3
    return torch.cat([n[..., c:c + 1] * ratio if c == k else n[..., c:c + 1] for c in range(3)], dim=-1)


def framework_transform(means: Tensor, quats: Optional[Tensor], instances_quats: Tensor, smpl_quats: Tensor, instances_trans: Tensor,
                        instances_fv: Tensor, cur_frame: int, *, J_canonical: Tensor, A0_inv: Tensor, parents: Sequence[int],
                        voxel_base: Optional[Tensor] = None, voxel_corr: Optional[Tensor] = None, offset: Optional[Tensor] = None,
                        scale: Optional[Tensor] = None, ratio: float = 1.0, ratio_dim: int = -1, W: Optional[Tensor] = None,
                        interpolate: bool = False, ball: bool = False):
    """The transform as framework ops (smpl.py:203-341): (world_means [I*V,3], world_quats [I*V,4] or None for ``ball``)."""
    I = instances_fv.shape[1]
    V = means.shape[0] // I
    mask = instances_fv[cur_frame]
    theta, trans = frame_pose(instances_quats, smpl_quats, instances_trans, instances_fv, cur_frame, interpolate)
    theta = _normalize(theta[mask])
    A = rigid_chain(p3d.quaternion_to_matrix(theta), J_canonical[mask], parents)
    A = torch.einsum("bnij,bnjk->bnik", A, A0_inv[mask])
    x = means.reshape(I, V, 3)
    if voxel_base is not None:
        field = voxel_base if voxel_corr is None else voxel_base + voxel_corr
        grid = normalize_coords(x, offset, scale, ratio, ratio_dim)[:, :, None, None]
        w = F.grid_sample(field, grid, align_corners=True, mode="bilinear", padding_mode="border")
        w = w.squeeze(4).squeeze(3).permute(0, 2, 1)[mask]
    else:
        w = W[mask]
    T = torch.einsum("bnj,bjrc->bnrc", w, A)
    R, t = T[:, :, :3, :3], T[:, :, :3, 3]
    present = mask.nonzero().reshape(-1)
    deformed = torch.einsum("bnij,bnj->bni", R, x[mask]) + t
    world_means = torch.zeros_like(x).index_add(0, present, deformed).reshape(-1, 3)
    world_means = world_means + trans[:, None, :].expand(I, V, 3).reshape(-1, 3)
    if ball:
        return world_means, None
    q = quats.reshape(I, V, 4)
    dq = nodes.quat_mult(_normalize(p3d.matrix_to_quaternion(R)), _normalize(q[mask]))
    unit = torch.zeros_like(q)
    unit[~mask, :, 0] = 1.0
    return world_means, unit.index_add(0, present, dq).reshape(-1, 4)


class _SkinTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, quats, instances_quats, smpl_quats, instances_trans, voxel_corr, instances_fv, cur_frame, interpolate, ball,
                tmpl):
        J, A0, parents, base, offset, scale, ratio, ratio_dim, W = tmpl
        L.require_gpu(*[t for t in (means, quats, instances_quats, smpl_quats, instances_trans, voxel_corr, instances_fv, J, A0, base,
                                    offset, scale, W) if t is not None])
        Fr, I = instances_fv.shape
        N = means.shape[0]
        if I < 1 or N % I or N == 0:
            raise L.BdsError(f"means must hold I * V rows for I = {I} instances (got {N})")
        V = N // I
        parents = check_parents(parents)
        assert means.shape == (N, 3) and (ball or quats.shape == (N, 4))
        assert instances_quats.shape == (Fr, I, 1, 4) and smpl_quats.shape == (Fr, I, JOINTS - 1, 4) and instances_trans.shape == (Fr, I, 3)
        assert J.shape == (I, JOINTS, 3) and A0.shape == (I, JOINTS, 4, 4)
        d = h = w = 0
        if base is not None:
            assert base.dim() == 5 and base.shape[:2] == (I, JOINTS) and (voxel_corr is None or voxel_corr.shape == base.shape)
            assert offset.numel() == I * 3 and scale.numel() == I
            d, h, w = (int(s) for s in base.shape[2:])
        else:
            if W is None or W.shape != (I, V, JOINTS):
                raise L.BdsError(f"without a voxel field the weights W must be [{I},{V},{JOINTS}]")
            voxel_corr = None
        with torch.no_grad():
            theta, trans = frame_pose(instances_quats, smpl_quats, instances_trans, instances_fv, int(cur_frame), bool(interpolate))
            root, body = L.f32c(theta[:, :1]), L.f32c(theta[:, 1:])
            trans = L.f32c(trans)
        m = L.f32c(means.detach())
        q = None if ball else L.f32c(quats.detach())
        corr = None if voxel_corr is None else L.f32c(voxel_corr.detach())
        Jc, A0c, basec, offc, scc, Wc = (None if t is None else L.f32c(t.detach()) for t in (J, A0, base, offset, scale, W))
        present = instances_fv[int(cur_frame)].detach().contiguous().to(torch.bool).view(torch.uint8)
        par = (C.c_int32 * JOINTS)(*parents)
        dev = means.device
        wm = torch.empty(N, 3, device=dev)
        wq = None if ball else torch.empty(N, 4, device=dev)
        A = torch.empty(I, JOINTS, 3, 4, device=dev)
        rdim = int(ratio_dim) % 3
        L.check(L.lib().bds_smpl_skin_fwd(I, V, L.ptr(m), L.ptr(q), L.ptr(root), L.ptr(body), L.ptr(trans), L.ptr(present), L.ptr(Jc), L.ptr(A0c),
                                          par, L.ptr(basec), L.ptr(corr), L.ptr(None if basec is not None else Wc), d, h, w, L.ptr(offc),
                                          L.ptr(scc), float(ratio), rdim, L.ptr(wm), L.ptr(wq), L.ptr(A), L.stream()), "bds_smpl_skin_fwd")
        ctx.save_for_backward(m, q, root, body, present, Jc, A0c, basec, corr, Wc, offc, scc, A)
        ctx.cfg = (I, V, d, h, w, float(ratio), rdim, parents, int(cur_frame), bool(interpolate), bool(ball), Fr, voxel_corr is not None)
        if ball:
            none = wm.new_empty(0)
            ctx.mark_non_differentiable(none)
            return wm, none
        return wm, wq

    @staticmethod
    def backward(ctx, v_wm, v_wq):
        m, q, root, body, present, Jc, A0c, basec, corr, Wc, offc, scc, A = ctx.saved_tensors
        I, V, d, h, w, ratio, rdim, parents, f, interp, ball, Fr, has_corr = ctx.cfg
        if interp:
            raise RuntimeError("bilateral_driving_amd.smpl.skin_transform: no gradient in the interpolated (test-set) mode -- the "
                               "reference's interpolate_quats edits a tensor in place and its autograd cannot differentiate it either")
        dev = m.device
        N = I * V
        v_wm = torch.zeros(N, 3, device=dev) if v_wm is None else v_wm.contiguous().float()
        if not ball:
            v_wq = torch.zeros(N, 4, device=dev) if v_wq is None else v_wq.contiguous().float()
        v_m = torch.empty(N, 3, device=dev)
        v_q = None if ball else torch.empty(N, 4, device=dev)
        v_iq, v_sq, v_it = torch.zeros(Fr, I, 1, 4, device=dev), torch.zeros(Fr, I, JOINTS - 1, 4, device=dev), torch.zeros(Fr, I, 3, device=dev)
        v_corr = torch.empty_like(corr) if has_corr else None
        nb = int(L.lib().bds_smpl_skin_bwd_temp_bytes(I, V))
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        par = (C.c_int32 * JOINTS)(*parents)
        L.check(L.lib().bds_smpl_skin_bwd(I, V, L.ptr(m), L.ptr(q), L.ptr(root), L.ptr(body), L.ptr(present), L.ptr(Jc), L.ptr(A0c), par,
                                          L.ptr(basec), L.ptr(corr), L.ptr(None if basec is not None else Wc), d, h, w, L.ptr(offc), L.ptr(scc),
                                          ratio, rdim, L.ptr(A), L.ptr(v_wm), L.ptr(None if ball else v_wq), L.ptr(v_m), L.ptr(v_q),
                                          L.ptr(v_iq[f]), L.ptr(v_sq[f]), L.ptr(v_it[f]), L.ptr(v_corr), L.ptr(temp), nb, L.stream()),
                "bds_smpl_skin_bwd")
        return v_m, v_q, v_iq, v_sq, v_it, v_corr, None, None, None, None, None


def skin_transform(means: Tensor, quats: Optional[Tensor], instances_quats: Tensor, smpl_quats: Tensor, instances_trans: Tensor,
                   instances_fv: Tensor, cur_frame: int, *, J_canonical: Tensor, A0_inv: Tensor, parents: Sequence[int],
                   voxel_base: Optional[Tensor] = None, voxel_corr: Optional[Tensor] = None, offset: Optional[Tensor] = None,
                   scale: Optional[Tensor] = None, ratio: float = 1.0, ratio_dim: int = -1, W: Optional[Tensor] = None,
                   interpolate: bool = False, ball: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """(world_means [I*V,3], world_quats [I*V,4]; None for ``ball``) of means [I*V,3] and raw quats [I*V,4] (instance i owns rows
    [i V, (i+1) V)), the frame tables instances_quats [F,I,1,4], smpl_quats [F,I,23,4], instances_trans [F,I,3], instances_fv [F,I]
    (bool) at ``cur_frame`` and the template's J_canonical [I,24,3], A0_inv [I,24,4,4], parents (24 host integers) and weights: the
    field voxel_base (+ voxel_corr) [I,24,d,h,w] with offset [I,1,3], scale [I,1,1], ratio, ratio_dim -- or, without a field, the fixed
    W [I,V,24].  ``interpolate``: the test-set form (``nodes.interpolates``), forward only.  world_quats is the reference's
    ``transform_means_and_quats`` result: ``get_gaussians``' final ``quat_act`` is the caller's.  CPU tensors raise ``BdsError``."""
    if ball:
        quats = None
    tmpl = (J_canonical, A0_inv, tuple(parents), voxel_base, offset, scale, float(ratio), int(ratio_dim), W)
    wm, wq = _SkinTransform.apply(means, quats, instances_quats, smpl_quats, instances_trans, voxel_corr, instances_fv, cur_frame,
                                  interpolate, ball, tmpl)
    return wm, (None if ball else wq)


# ---- get_gaussians of the reference's SMPLNodes --------------------------------------------------------------------------------------
def template_tensors(template) -> dict:
    """The keyword arguments of ``skin_transform`` from a ``SMPLTemplate``; the host values (parent table, ratio) are read once."""
    host = template.__dict__.get("_bds_host")
    if host is None:
        vd = getattr(template, "voxel_deformer", None) if template.use_voxel_deformer else None
        host = (check_parents([0] + [int(p) for p in template._template_layer.parents[1:]]), 1.0 if vd is None else float(vd.ratio))
        template.__dict__["_bds_host"] = host
    out = dict(J_canonical=template.J_canonical, A0_inv=template.A0_inv, parents=host[0])
    if template.use_voxel_deformer:
        vd = template.voxel_deformer
        out.update(voxel_base=vd.lbs_voxel_base, voxel_corr=getattr(vd, "voxel_w_correction", None), offset=vd.offset, scale=vd.scale,
                   ratio=host[1], ratio_dim=vd.ratio_dim)
    else:
        out.update(W=template.W)
    return out


def smpl_get_gaussians(self, cam):
    """``SMPLNodes.get_gaussians`` (smpl.py:343-397) on the fused transform."""
    vd = getattr(self.template, "voxel_deformer", None)
    if not self._means.is_cuda or (self.template.use_voxel_deformer and hasattr(vd, "additional_correction")):
        return type(self)._bds_reference_get_gaussians(self, cam)
    self.filter_mask = torch.ones_like(self._means[:, 0], dtype=torch.bool)   # (all true: the tensors below are returned whole)
    fv = self.instances_fv
    if fv[self.cur_frame].sum() == 0:
        return None
    interp = nodes.interpolates(getattr(self, "in_test_set", False), self.cur_frame, fv.shape[0])
    flags = torch.zeros(2, dtype=torch.int32, device=self._means.device)
    world_means, world_quats = skin_transform(self._means, self._quats, self.instances_quats, self.smpl_qauts, self.instances_trans, fv,
                                              self.cur_frame, interpolate=interp, ball=bool(self.ball_gaussians),
                                              **template_tensors(self.template))
    if self.ball_gaussians:
        world_quats = self._quats
    colors = torch.cat((self._features_dc[:, None, :], self._features_rest), dim=1)
    if self.sh_degree > 0:
        viewdirs = world_means.detach() - cam.camtoworlds.data[..., :3, 3]
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        n = min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree)
        rgbs = torch.clamp(gs_ops.spherical_harmonics(n, viewdirs, colors) + 0.5, 0.0, 1.0)
    else:
        rgbs = torch.sigmoid(colors[:, 0, :])
    opacities = torch.sigmoid(self._opacities) * fv[self.cur_frame][self.point_ids[..., 0]].float().unsqueeze(-1)
    scales = torch.exp(self._scales.repeat(1, 3)) if self.ball_gaussians else torch.exp(self._scales)
    gs = dict(_means=world_means, _opacities=opacities, _rgbs=rgbs, _scales=scales, _quats=_normalize(world_quats))
    nodes._finite_check(self, gs, flags)
    self._gs_cache = {"_scales": scales}
    return gs


_SEAM = Seam()


def install(node_class) -> None:
    """``install(models.nodes.SMPLNodes)``: the class's ``get_gaussians`` becomes the fused one.  The original stays reachable as
    ``node_class._bds_reference_get_gaussians`` (and serves CPU tensors and a template with ``additional_correction``); ``uninstall``
    puts it back."""
    _SEAM.install(node_class, {"get_gaussians": smpl_get_gaussians}, reference="_bds_reference_get_gaussians")


def uninstall(*node_classes) -> None:
    _SEAM.uninstall(*node_classes)
