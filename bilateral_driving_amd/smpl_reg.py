"""The SMPL nodes' two every-step regularisers as fused HIP ops (csrc/smpl_reg.hip through ``bds_smpl_knn_reg_*`` and
``bds_voxel_reg_*``).

Reference: ``SMPLNodes.compute_reg_loss`` (models/nodes/smpl.py:399-520).  Of its terms the shipped human config turns on ``knn_reg``
(:462-503: per attribute group the unbiased std over each point's K gathered neighbour values, averaged) and ``voxel_deformer_reg``
(:448-459: ``VoxelDeformer.get_tv`` / ``get_mag``, models/modules.py:1139-1166, of the skinning field's corrections).

* ``reverse_lists(nn_ind)`` turns the neighbour lists into the reverse adjacency the backward gathers through (once per
  ``update_knn``; it validates the indices with one read-back).  ``cached_reverse_lists(node, nn_ind)`` keeps it on the node.
* ``knn_reg(...)`` -> the five terms (dc, rest, opacity, scales, quats; 0 for a frozen group): one launch and a one-workgroup finish
  forward, ONE gather-form launch backward, no atomics -- the gradients are bit-identical run to run.
* ``voxel_reg(field)`` -> (tv, magnitude) of a field [I,J,D,H,W]: one pass forward (plus the finish), one pass backward.
* ``framework_knn_reg`` / ``framework_voxel_reg``: the reference's expressions as framework ops (tests, and the A side of
  scripts/smpl_reg_time.py).
* ``install(cls)`` / ``uninstall(cls)`` swap ``compute_reg_loss`` on the reference's own ``SMPLNodes``: the two terms come from the
  ops above, every other term from the class's own method.  CPU tensors keep the class's method.  Nothing is installed by default.

Deviations: K = 1 and a field with D, H or W = 1 raise ``ValueError`` (the reference returns NaN); an index outside [0, V) raises
``IndexError`` from ``reverse_lists`` (the reference's gather asserts on the device); with no instance present the op returns zeros
(the reference's mean over nothing is NaN; the installed method returns early before that, as the reference)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam

GROUPS = ("features_dc", "features_rest", "opacities", "scales", "quats")
KEYS = ("knn_reg_dc", "knn_reg_rest", "knn_reg_o", "knn_reg_s", "knn_reg_q")                       # loss_dict keys, in the reference's order
LAMBDAS = ("lambda_std_shs_dc", "lambda_std_shs_rest", "lambda_std_o", "lambda_std_s", "lambda_std_q")
MAX_K, MAX_J = 32, 64


def reverse_lists(nn_ind: Tensor) -> Tuple[Tensor, Tensor]:
    """(offsets [I,V+1] int32, edges [I,V K] int32) of nn_ind [I,V,K]: edges[i, offsets[i,r]:offsets[i,r+1]] are the flat
    (point K + slot) pairs of instance i that list row r, ascending; a pair listed twice appears twice.  Raises ``IndexError`` for an
    index outside [0, V) (one read-back: call it where the lists are made, not per step)."""
    if nn_ind.dim() != 3 or nn_ind.dtype not in (torch.int32, torch.int64) or nn_ind.numel() == 0:
        raise ValueError(f"nn_ind must be a non-empty integer tensor [I,V,K], got {tuple(nn_ind.shape)} {nn_ind.dtype}")
    I, V, K = nn_ind.shape
    flat = nn_ind.reshape(I, V * K).long()
    lo, hi = torch.stack((flat.min(), flat.max())).tolist()
    if lo < 0 or hi >= V:
        raise IndexError(f"nn_ind holds indices in [{lo}, {hi}], outside [0, {V})")
    edges = torch.sort(flat, dim=1, stable=True).indices.to(torch.int32)
    rows = (flat + torch.arange(I, device=flat.device)[:, None] * V).reshape(-1)
    counts = torch.bincount(rows, minlength=I * V).reshape(I, V)
    offsets = torch.cat((counts.new_zeros(I, 1), counts.cumsum(1)), dim=1).to(torch.int32)
    return offsets.contiguous(), edges.contiguous()


def cached_reverse_lists(node, nn_ind: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(offsets, edges, nn_ind as int32) kept in ``node.__dict__``, rebuilt when ``node.nn_ind`` is another tensor or was written."""
    hit = node.__dict__.get("_bds_knn_reverse")
    if hit is None or hit[0] is not nn_ind or hit[1] != nn_ind._version:
        offsets, edges = reverse_lists(nn_ind)
        hit = (nn_ind, nn_ind._version, (offsets, edges, nn_ind.to(torch.int32).contiguous()))
        node.__dict__["_bds_knn_reverse"] = hit
    return hit[2]


class _KnnReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nn32, offsets, edges, present, s_dim, *attrs):
        L.require_gpu(nn32, offsets, edges, present, *attrs)
        I, V, K = nn32.shape
        flat = [None if t is None else L.f32c(t.detach()).reshape(I * V, -1) for t in attrs]
        widths = [0 if t is None else t.shape[1] for t in flat]
        c_rest = widths[1]
        ctot = sum(widths)
        dev = nn32.device
        terms, norm = torch.empty(5, device=dev), torch.empty(5, device=dev)
        stats = torch.empty(2, I * V * max(ctot, 1), device=dev)
        nb = int(L.lib().bds_smpl_knn_reg_temp_bytes(I, V, ctot))
        temp = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
        L.check(L.lib().bds_smpl_knn_reg_fwd(I, V, K, L.ptr(nn32), L.ptr(present), L.ptr(flat[0]), L.ptr(flat[1]), c_rest, L.ptr(flat[2]),
                                             L.ptr(flat[3]), s_dim, L.ptr(flat[4]), L.ptr(terms), L.ptr(norm), L.ptr(stats[0]), L.ptr(stats[1]),
                                             L.ptr(temp), nb, L.stream()), "bds_smpl_knn_reg_fwd")
        ctx.save_for_backward(offsets, edges, present, norm, stats, *[t for t in flat if t is not None])
        ctx.cfg = (I, V, K, c_rest, s_dim, [None if t is None else t.shape for t in attrs])
        return terms

    @staticmethod
    def backward(ctx, v_terms):
        offsets, edges, present, norm, stats, *live = ctx.saved_tensors
        I, V, K, c_rest, s_dim, shapes = ctx.cfg
        live = iter(live)
        flat = [None if s is None else next(live) for s in shapes]
        grads = [None if t is None else torch.empty_like(t) for t in flat]
        v_terms = L.f32c(v_terms)
        L.check(L.lib().bds_smpl_knn_reg_bwd(I, V, K, L.ptr(offsets), L.ptr(edges), L.ptr(present), L.ptr(flat[0]), L.ptr(flat[1]), c_rest,
                                             L.ptr(flat[2]), L.ptr(flat[3]), s_dim, L.ptr(flat[4]), L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(norm),
                                             L.ptr(v_terms), *[L.ptr(g) for g in grads], L.stream()), "bds_smpl_knn_reg_bwd")
        return (None, None, None, None, None, *[None if g is None else g.view(s) for g, s in zip(grads, shapes)])


def knn_reg(nn_ind: Tensor, present: Tensor, *, features_dc: Optional[Tensor] = None, features_rest: Optional[Tensor] = None,
            opacities: Optional[Tensor] = None, scales: Optional[Tensor] = None, quats: Optional[Tensor] = None,
            reverse: Optional[Tuple[Tensor, ...]] = None) -> Tensor:
    """The five kNN terms [5] (dc, rest, opacity, scales, quats; before their lambdas) of nn_ind [I,V,K] (within-instance indices,
    2 <= K <= 32), present [I] (bool: ``instances_fv[cur_frame]``) and the RAW parameters features_dc [I V,3], features_rest
    [I V,K_sh-1,3] (degree 1..3), opacities [I V,1], scales [I V,1 or 3], quats [I V,4]; ``None`` is a frozen group (term 0, no
    gradient).  ``reverse``: ``cached_reverse_lists``' result; without it the lists are built (and validated, with a read-back) here.
    CPU tensors raise ``BdsError``."""
    attrs = (features_dc, features_rest, opacities, scales, quats)
    if nn_ind.dim() != 3:
        raise ValueError(f"nn_ind must be [I,V,K], got {tuple(nn_ind.shape)}")
    I, V, K = nn_ind.shape
    if not 2 <= K <= MAX_K:
        raise ValueError(f"knn_reg needs 2 <= K <= {MAX_K} neighbours (the unbiased std of one value is NaN), got K = {K}")
    want = (3, None, 1, None, 4)
    for name, t, w in zip(GROUPS, attrs, want):
        if t is None:
            continue
        width = t.numel() // (I * V) if t.shape[0] == I * V else -1
        ok = width == w if w is not None else (width in (9, 24, 45) if name == "features_rest" else width in (1, 3))
        if not ok:
            raise ValueError(f"{name} must hold I * V = {I * V} rows of {w or ('9, 24 or 45' if name == 'features_rest' else '1 or 3')} floats, got {tuple(t.shape)}")
    if present.shape != (I,):
        raise ValueError(f"present must be [{I}], got {tuple(present.shape)}")
    L.require_gpu(nn_ind, present, *attrs)
    if reverse is None:
        offsets, edges = reverse_lists(nn_ind)
        nn32 = nn_ind.to(torch.int32).contiguous()
    else:
        offsets, edges, nn32 = reverse
    present = present.detach().contiguous().to(torch.bool).view(torch.uint8)
    s_dim = 3 if scales is None else scales.numel() // (I * V)
    return _KnnReg.apply(nn32, offsets, edges, present, s_dim, *attrs)


class _VoxelReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field):
        L.require_gpu(field)
        x = L.f32c(field.detach())
        I, J, D, H, W = x.shape
        dev = x.device
        terms, rnorm = torch.empty(2, device=dev), torch.empty(I, D, H, W, device=dev)
        nb = int(L.lib().bds_voxel_reg_temp_bytes(I, D, H, W))
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        L.check(L.lib().bds_voxel_reg_fwd(I, J, D, H, W, L.ptr(x), L.ptr(terms), L.ptr(rnorm), L.ptr(temp), nb, L.stream()), "bds_voxel_reg_fwd")
        ctx.save_for_backward(x, rnorm)
        return terms

    @staticmethod
    def backward(ctx, v_terms):
        x, rnorm = ctx.saved_tensors
        I, J, D, H, W = x.shape
        v_x = torch.empty_like(x)
        L.check(L.lib().bds_voxel_reg_bwd(I, J, D, H, W, L.ptr(x), L.ptr(rnorm), L.ptr(L.f32c(v_terms)), L.ptr(v_x), L.stream()), "bds_voxel_reg_bwd")
        return v_x


def voxel_reg(field: Tensor) -> Tensor:
    """(tv, magnitude) [2] of a field [I,J,D,H,W] (1 <= J <= 64; D, H, W >= 2): ``VoxelDeformer.get_tv`` and ``get_mag`` of it.  The
    backward returns the field's gradient (autograd adds it to the skinning's).  CPU tensors raise ``BdsError``."""
    if field.dim() != 5 or field.numel() == 0:
        raise ValueError(f"field must be a non-empty [I,J,D,H,W], got {tuple(field.shape)}")
    if min(field.shape[2:]) < 2:
        raise ValueError(f"voxel_reg needs D, H, W >= 2 (the reference's mean over an empty slice is NaN), got {tuple(field.shape)}")
    if field.shape[1] > MAX_J:
        raise ValueError(f"voxel_reg serves up to {MAX_J} channels, got {field.shape[1]}")
    L.require_gpu(field)
    return _VoxelReg.apply(field)


# ---- the reference's expressions as framework ops ------------------------------------------------------------------------------------
def framework_knn_reg(nn_ind: Tensor, present: Tensor, *, features_dc: Optional[Tensor] = None, features_rest: Optional[Tensor] = None,
                      opacities: Optional[Tensor] = None, scales: Optional[Tensor] = None, quats: Optional[Tensor] = None) -> Tensor:
    """smpl.py:462-503 on the raw parameters -> the five terms [5] (0 for a frozen group); NaN with no instance present, as there."""
    I, V, K = nn_ind.shape
    mask = present.to(torch.bool)
    nn = nn_ind[mask].long()
    ref = next(t for t in (features_dc, features_rest, opacities, scales, quats) if t is not None)
    out = []
    for t, act in ((features_dc, None), (features_rest, None), (opacities, torch.sigmoid), (scales, torch.exp), (quats, None)):
        if t is None:
            out.append(ref.new_zeros(()))
            continue
        a = t if act is None else act(t)
        valid = a.reshape(I, V, -1)[mask]
        C = valid.shape[-1]
        gathered = torch.gather(valid.unsqueeze(2).expand(-1, -1, K, -1), 1, nn.unsqueeze(-1).expand(-1, -1, -1, C))
        out.append(gathered.std(dim=2).mean())
    return torch.stack(out)


def framework_voxel_reg(field: Tensor) -> Tensor:
    """modules.py:1148-1151 and :1166 -> (tv, magnitude) [2]."""
    d = field
    tv_x = torch.abs(d[:, :, 1:, :, :] - d[:, :, :-1, :, :]).mean()
    tv_y = torch.abs(d[:, :, :, 1:, :] - d[:, :, :, :-1, :]).mean()
    tv_z = torch.abs(d[:, :, :, :, 1:] - d[:, :, :, :, :-1]).mean()
    return torch.stack(((tv_x + tv_y + tv_z) / 3.0, torch.norm(d, dim=1).mean()))


# ---- compute_reg_loss of the reference's SMPLNodes -----------------------------------------------------------------------------------
HIDDEN = ("voxel_deformer_reg", "knn_reg")


class _Without:
    """``reg_cfg`` as the class's own method sees it while the fused terms are computed here: ``get`` answers the default for the two
    hidden keys, everything else is the config's."""

    def __init__(self, cfg):
        self._cfg = cfg

    def get(self, key, default=None):
        return default if key in HIDDEN else self._cfg.get(key, default)

    def __getattr__(self, name):
        return getattr(self._cfg, name)

    def __getitem__(self, key):
        return self._cfg[key]

    def __contains__(self, key):
        return key not in HIDDEN and key in self._cfg


def frames_with_instances(node) -> Tuple[bool, ...]:
    """Per frame, whether any instance is present: a host copy of ``instances_fv`` made once (and again when the tensor changes)."""
    fv = node.instances_fv
    hit = node.__dict__.get("_bds_fv_host")
    if hit is None or hit[0] is not fv or hit[1] != fv._version:
        hit = (fv, fv._version, tuple(bool(b) for b in fv.any(dim=1).tolist()))
        node.__dict__["_bds_fv_host"] = hit
    return hit[2]


def _field_terms(vd, attr: str, name: str):
    if hasattr(vd, attr):
        t = voxel_reg(getattr(vd, attr))
        return t[0], t[1]
    return vd.get_tv(name), vd.get_mag(name)      # (the reference's zeros)


def _on_device(node) -> bool:
    return node._means.is_cuda


def smpl_compute_reg_loss(self):
    """``SMPLNodes.compute_reg_loss`` (smpl.py:399-520) with ``voxel_deformer_reg`` and ``knn_reg`` from the fused ops; every other term
    (the ``VanillaGaussians`` ones, ``smpl_temporal_smooth``, ``x_offset``, the early return on a frame without instances) is the
    class's own method, called with the two keys hidden from it."""
    own = type(self)._bds_reference_compute_reg_loss
    if not _on_device(self):
        return own(self)
    cfg = self.reg_cfg
    self.reg_cfg = _Without(cfg)
    try:
        rest = own(self)
    finally:
        self.reg_cfg = cfg
    if not frames_with_instances(self)[self.cur_frame]:
        return rest
    ours = {}
    vox = cfg.get("voxel_deformer_reg", None)
    if vox is not None and self.use_voxel_deformer:
        vd = self.template.voxel_deformer
        w_std, w_norm = _field_terms(vd, "voxel_w_correction", "dc")
        w_rest_std, w_rest_norm = _field_terms(vd, "additional_correction", "rest")
        ours["voxel_deformer_reg"] = vox.lambda_std_w * w_std + vox.lambda_std_w_rest * w_rest_std + vox.lambda_w_norm * w_norm + \
            vox.lambda_w_rest_norm * w_rest_norm
    knn = cfg.get("knn_reg", None)
    if knn is not None:
        c = self.ctrl_cfg
        live = (not c.freeze_shs_dc, not c.freeze_shs_rest and self.sh_degree > 0, not c.freeze_o, not c.freeze_s, not c.freeze_q)
        params = (self._features_dc, self._features_rest, self._opacities, self._scales, self._quats)
        terms = knn_reg(self.nn_ind, self.instances_fv[self.cur_frame], reverse=cached_reverse_lists(self, self.nn_ind),
                        **{g: (p if on else None) for g, p, on in zip(GROUPS, params, live)})
        for k, (key, lam) in enumerate(zip(KEYS, LAMBDAS)):
            if live[k]:
                ours[key] = terms[k] * getattr(knn, lam)
    out = {k: v for k, v in rest.items() if k != "x_offset"}      # the reference's order: ..., the field term, the kNN terms, x_offset
    out.update(ours)
    if "x_offset" in rest:
        out["x_offset"] = rest["x_offset"]
    return out


_SEAM = Seam()


def install(node_class) -> None:
    """``install(models.nodes.SMPLNodes)``: the class's ``compute_reg_loss`` becomes the fused one (composes with ``smpl.install``: the
    two touch different methods).  The original stays reachable as ``node_class._bds_reference_compute_reg_loss``; ``uninstall`` puts
    it back."""
    _SEAM.install(node_class, {"compute_reg_loss": smpl_compute_reg_loss}, reference="_bds_reference_compute_reg_loss")


def uninstall(*node_classes) -> None:
    _SEAM.uninstall(*node_classes)
