"""Density control of the periodic-vibration Gaussians on the device (csrc/refine.hip ``pvg_*`` kernels, csrc/pvg_math.h): drop-ins for
``PeriodicVibrationGaussians.after_train`` (models/gaussians/pvg.py:100-133), ``refinement_after`` (:148-265, with split_gaussians
:298-354, dup_gaussians :356-372, cull_gaussians :267-284 and the optimiser surgery of models/gaussians/basics.py:162-206 over the
class's NINE named groups, :135-146) and ``compute_reg_loss`` (:427-436, the ``velocity_reg`` term).

* ``after_train`` is one statistics launch behind two small ones that turn ``filter_mask`` into the kept rows' offsets; the reference
  runs about ten masked-index operations, each with a host wait.
* ``refinement_after`` plans the densification (``bds_pvg_refine_plan``: the EXISTING flags / ranks / totals layout, no cull), reads
  the counts back once -- the noise tensor's size has to be known -- writes the four arrays a split changes
  (``bds_pvg_refine_geometry``) and moves the other 23 with ``densify.move_rows``.  The cull is evaluated on the NEW rows
  (``bds_pvg_cull_mask``: every child is judged by gamma of its own mean, so two children of one parent can fare differently) and
  compacted by ``densify.compact_rows`` (``densify`` is the core: this class is ``PERIODIC_ROWS`` plus its three kernels), with one more
  read-back.  The two order-preserving compactions leave the reference's rows in the reference's order; on a refinement step every
  array is therefore written twice.
* ``velocity_reg`` is the bare operator (fixed-order reduction, no float atomics; a zero velocity gets gradient 0, not NaN).
* ``install(cls)`` / ``uninstall(*classes)`` swap the three methods on the reference's own class, independently of ``pvg.install``;
  both read the ``filter_mask`` either ``get_gaussians`` leaves behind.  CPU tensors keep the class's own methods; the operators
  raise ``BdsError`` for them.  Nothing is installed by default.
* ``framework_*``: the reference's sequence as framework ops in the tensors' own dtype and device (tests, and the A side of
  scripts/pvg_refine_time.py).

Not covered: ball / 2-D Gaussians, ``reorder=``, ``dist.refinement_after_synced`` and the lazy one-view path.  ``reorder=`` now needs
only the wiring: ``densify.reorder_rows(..., PERIODIC_ROWS)`` moves all nine arrays, their moments and the four statistics."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import _lib as L
from . import densify as core
from ._patch import Seam
from .densify import PERIODIC_ROWS, _ctrl_get

ATTRS, GROUPS, STATS = PERIODIC_ROWS.attrs, PERIODIC_ROWS.groups, PERIODIC_ROWS.stats
SIZE_FAC = 1.6


def schedule(step: int, ctrl, num_train_images: int, num_points: int) -> dict:
    """The shared switches (``densify.schedule``) with the class's own term: no densification from
    ``densify_until_num_points`` rows on (pvg.py:158)."""
    sch = core.schedule(step, ctrl, num_train_images)
    sch["do_densify"] = bool(sch["do_densify"] and num_points < ctrl.densify_until_num_points)
    return sch


def _mask_u8(mask: Tensor) -> Tensor:
    mask = mask.reshape(-1).contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)


def _radii(radii: Tensor) -> Tuple[Tensor, int]:
    radii = radii.detach().reshape(-1)
    if radii.dtype == torch.int32:
        return radii.contiguous(), 0
    return radii.float().contiguous(), 1


def _origin(scene_origin, like: Tensor) -> Tensor:
    o = torch.as_tensor(scene_origin, dtype=torch.float32, device=like.device).reshape(-1).contiguous()
    assert o.numel() == 3
    return o


# ---- after_train ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def densify_stats(stats: Optional[Tuple[Tensor, Tensor, Tensor, Tensor]], filter_mask: Tensor, radii: Tensor, xys_grad: Tensor,
                  taus_grad: Tensor, last_size: int, sx: float = 1.0, sy: float = 1.0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``bds_pvg_densify_stats``: (xys_grad_norm, t_grad_accum, vis_counts, max_2Dsize), each [N] float32.  ``stats`` None: the
    initialising call (new arrays); otherwise the four arrays, updated in place.  ``filter_mask`` [N] bool keeps M rows, the rows
    of ``radii`` [M] and ``xys_grad`` [M,2]; ``taus_grad`` [N] or [N,1].  ``sx, sy``: 1 for gradients the trainer has scaled
    (base.py:285-286); a ``DensifyStats``-style caller with raw gradients passes width / 2 and height / 2 (times the batch size)."""
    L.require_gpu(filter_mask, radii, xys_grad, taus_grad, *(stats or ()))
    N, M = filter_mask.numel(), radii.numel()
    assert M <= N and xys_grad.numel() == 2 * M and taus_grad.numel() == N
    dev = filter_mask.device
    first = stats is None
    if first:
        stats = tuple(torch.empty(N, dtype=torch.float32, device=dev) for _ in range(4))
    for t in stats:
        assert t.shape == (N,) and t.dtype == torch.float32 and t.is_contiguous()
    rad, rad_float = _radii(radii)
    nb = int(L.lib().bds_pvg_mask_temp_bytes(N))
    temp = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    L.check(L.lib().bds_pvg_densify_stats(N, M, L.ptr(_mask_u8(filter_mask)), L.ptr(L.f32c(xys_grad.detach()).reshape(-1, 2)), float(sx),
                                          float(sy), L.ptr(rad), rad_float, L.ptr(L.f32c(taus_grad.detach()).reshape(-1)), int(last_size),
                                          int(first), *[L.ptr(t) for t in stats], L.ptr(temp), nb, L.stream()), "bds_pvg_densify_stats")
    return stats


def after_train(self, radii: Tensor, xys_grad: Tensor, last_size: int) -> None:
    """``PeriodicVibrationGaussians.after_train`` (pvg.py:100-133)."""
    if not self._means.is_cuda:
        return type(self)._bds_reference_after_train(self, radii, xys_grad, last_size)
    first = self.xys_grad_norm is None
    if first:
        stats = None
    else:
        assert self.vis_counts is not None
        if self.max_2Dsize is None:
            self.max_2Dsize = torch.zeros(self._means.shape[0], device=radii.device, dtype=torch.float32)
        stats = (self.xys_grad_norm, self.t_grad_accum, self.vis_counts, self.max_2Dsize)
    out = densify_stats(stats, self.filter_mask, radii, xys_grad, self._taus.grad, last_size)
    self.xys_grad_norm, self.t_grad_accum, self.vis_counts, self.max_2Dsize = out


# ---- refinement_after -----------------------------------------------------------------------------------------------------------------
def refine_plan(xys_grad_norm: Tensor, t_grad_accum: Tensor, vis_counts: Tensor, max_2Dsize: Tensor, log_scales: Tensor, betas: Tensor,
                means: Tensor, scene_origin: Tensor, scene_scale: float, *, grad_thresh: float, t_grad_thresh: float, size_thresh: float,
                t_size_thresh: float, split_by_screen: bool, split_screen_size: float):
    """``bds_pvg_refine_plan``: (flags [N] u8, kinds [N] u8, ranks [N,4] i32, totals [5] i64), the densification decisions without a
    cull.  ``size_thresh``: densify_size_thresh * scene_scale."""
    L.require_gpu(xys_grad_norm, t_grad_accum, vis_counts, max_2Dsize, log_scales, betas, means, scene_origin)
    N = log_scales.shape[0]
    flags, ranks, totals, temp = core.plan_outputs(N, log_scales.device)
    kinds = torch.empty_like(flags)
    flat = lambda t: L.f32c(t.detach()).reshape(-1)
    args = [flat(t) for t in (xys_grad_norm, t_grad_accum, vis_counts, max_2Dsize, log_scales, betas, means)]
    assert all(a.numel() == N * w for a, w in zip(args, (1, 1, 1, 1, 3, 1, 3)))
    L.check(L.lib().bds_pvg_refine_plan(N, *[L.ptr(a) for a in args], L.ptr(scene_origin), float(scene_scale), float(grad_thresh),
                                        float(t_grad_thresh), float(size_thresh), float(t_size_thresh), int(split_by_screen),
                                        float(split_screen_size), L.ptr(flags), L.ptr(kinds), L.ptr(ranks), L.ptr(totals), L.ptr(temp),
                                        temp.numel(), L.stream()), "bds_pvg_refine_plan")
    return flags, kinds, ranks, totals


def refine_geometry(flags: Tensor, kinds: Tensor, ranks: Tensor, totals: Tensor, n_new: int, samps: int, samples: Tensor, means: Tensor,
                    quats: Tensor, log_scales: Tensor, velocity: Tensor, taus: Tensor, betas: Tensor, T: float,
                    no_time_split: bool) -> Dict[str, Tensor]:
    """``bds_pvg_refine_geometry``: the new ``_means [n_new,3] _scales [n_new,3] _taus [n_new,1] _betas [n_new,1]``."""
    L.require_gpu(flags, kinds, ranks, totals, samples, means, quats, log_scales, velocity, taus, betas)
    N, dev = means.shape[0], means.device
    out = {"_means": torch.empty(n_new, 3, device=dev), "_scales": torch.empty(n_new, 3, device=dev),
           "_taus": torch.empty(n_new, 1, device=dev), "_betas": torch.empty(n_new, 1, device=dev)}
    src = [L.f32c(t.detach()) for t in (samples, means, quats, log_scales, velocity, taus, betas)]
    assert samples.shape[1:] == (4,) and quats.shape == (N, 4) and taus.numel() == N and betas.numel() == N
    L.check(L.lib().bds_pvg_refine_geometry(N, int(samps), int(no_time_split), float(T), L.ptr(flags), L.ptr(kinds), L.ptr(ranks),
                                            L.ptr(totals), *[L.ptr(t) for t in src], *[L.ptr(out[k]) for k in ("_means", "_scales", "_taus", "_betas")],
                                            L.stream()), "bds_pvg_refine_geometry")
    return out


def cull_mask(logits: Tensor, log_scales: Tensor, means: Tensor, max_2Dsize: Optional[Tensor], scene_origin: Tensor, scene_scale: float, *,
              cull_alpha_thresh: float, cull_by_scale: bool, cull_scale_thresh: float, cull_by_screen: bool,
              cull_screen_size: float) -> Tensor:
    """``bds_pvg_cull_mask``: [N'] u8 over the NEW rows; ``max_2Dsize`` covers the first ``len(max_2Dsize)`` of them (children: 0).
    ``cull_scale_thresh``: the ctrl value times scene_scale."""
    L.require_gpu(logits, log_scales, means, max_2Dsize, scene_origin)
    N = means.shape[0]
    mask = torch.empty(N, dtype=torch.uint8, device=means.device)
    m2 = None if max_2Dsize is None else L.f32c(max_2Dsize.detach()).reshape(-1)
    n_old = 0 if m2 is None else m2.numel()
    lg, ls, m = (L.f32c(t.detach()) for t in (logits, log_scales, means))
    assert lg.numel() == N and ls.shape == (N, 3) and m.shape == (N, 3)
    L.check(L.lib().bds_pvg_cull_mask(N, n_old, L.ptr(lg), L.ptr(ls), L.ptr(m), L.ptr(m2), L.ptr(scene_origin), float(scene_scale),
                                      float(cull_alpha_thresh), int(cull_by_scale), float(cull_scale_thresh), int(cull_by_screen),
                                      float(cull_screen_size), L.ptr(mask), L.stream()), "bds_pvg_cull_mask")
    return mask


@torch.no_grad()
def refinement_after(self, step: int, optimizer: torch.optim.Optimizer, samples: Optional[Tensor] = None) -> None:
    """``PeriodicVibrationGaussians.refinement_after(step, optimizer)`` (pvg.py:148-265).  ``samples`` (optional,
    [n_split_samples * n_split, 4]) replaces the two draws of split_gaussians: columns 0-2 the ``torch.randn`` of :305, column 3 a
    unit normal z that stands for ``torch.normal(0, std)`` = std * z (:332).  Two host read-backs: the counts of the plan, and the
    size the cull leaves."""
    if not self._means.is_cuda:
        return type(self)._bds_reference_refinement_after(self, step, optimizer)
    assert step == self.step
    ctrl = self.ctrl_cfg
    if self.step <= ctrl.warmup_steps:
        return
    if getattr(self, "ball_gaussians", False) or getattr(self, "gaussian_2d", False):
        raise NotImplementedError("ball / 2-D Gaussians are not covered by the fused refinement")
    N = self._means.shape[0]
    sch = schedule(self.step, ctrl, self.num_train_images, N)
    print(f"Class {self.class_prefix} current points: {N} @ step {self.step}")
    for a in ATTRS:
        L.require_gpu(getattr(self, a))
    dev = self._means.device
    scale = float(self.scene_scale)
    origin = _origin(self.scene_origin, self._means) if (sch["do_densify"] or sch["do_cull"]) else None
    max_2Dsize = self.max_2Dsize
    if sch["do_densify"]:
        assert self.xys_grad_norm is not None and self.vis_counts is not None and self.max_2Dsize is not None
        samps = int(ctrl.n_split_samples)
        flags, kinds, ranks, totals = refine_plan(
            self.xys_grad_norm, self.t_grad_accum, self.vis_counts, self.max_2Dsize, self._scales, self._betas, self._means, origin, scale,
            grad_thresh=ctrl.densify_grad_thresh, t_grad_thresh=ctrl.densify_t_grad_thresh, size_thresh=ctrl.densify_size_thresh * scale,
            t_size_thresh=ctrl.densify_t_size_thresh, split_by_screen=sch["by_screen"], split_screen_size=ctrl.split_screen_size)
        n_split, n_dup = (int(v) for v in totals[:2].tolist())               # host read-back 1: the noise tensor's size
        print(f"    Split: {n_split}")
        print(f"      Dup: {n_dup}")
        if samples is None:                                                   # :305 and :332, from the same stream
            samples = torch.cat((torch.randn((samps * n_split, 3), device=dev), torch.randn((samps * n_split, 1), device=dev)), 1)
        samples = samples.to(device=dev, dtype=torch.float32).contiguous()
        assert samples.shape == (samps * n_split, 4)
        n_new = N + samps * n_split + n_dup
        if n_new != N:
            geometry = refine_geometry(flags, kinds, ranks, totals, n_new, samps, samples, self._means, self._quats, self._scales,
                                       self._velocity, self._taus, self._betas, float(self.T), bool(_ctrl_get(ctrl, "no_time_split", False)))
            core.move_rows(self, optimizer, PERIODIC_ROWS, flags, ranks, totals, samps, n_new, geometry)
    if sch["do_cull"]:
        n_bef = self._means.shape[0]
        n_left = n_bef
        if n_bef:
            by_screen = sch["cull_by_scale"] and sch["by_screen"]
            assert not by_screen or max_2Dsize is not None
            mask = cull_mask(self._opacities, self._scales, self._means, max_2Dsize if by_screen else None, origin, scale,
                             cull_alpha_thresh=ctrl.cull_alpha_thresh, cull_by_scale=sch["cull_by_scale"],
                             cull_scale_thresh=ctrl.cull_scale_thresh * scale, cull_by_screen=by_screen,
                             cull_screen_size=ctrl.cull_screen_size)
            n_left = core.compact_rows(self, optimizer, PERIODIC_ROWS, mask)    # host read-back 2: the new size
        print(f"     Cull: {n_bef - n_left}")
    print(f"Class {self.class_prefix} left points: {self._means.shape[0]}")
    if sch["do_reset"]:                                                       # pvg.py:249-261
        core.reset_opacity(self, optimizer, PERIODIC_ROWS, ctrl.reset_alpha_value)
    for name in STATS:
        setattr(self, name, None)


# ---- velocity_reg ---------------------------------------------------------------------------------------------------------------------
class _VelocityReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, velocity, betas, filter_mask, radii, T):
        L.require_gpu(velocity, betas, filter_mask, radii)
        N, M, dev = velocity.shape[0], radii.numel(), velocity.device
        assert velocity.shape == (N, 3) and betas.numel() == N and filter_mask.numel() == N and M <= N
        v, b = L.f32c(velocity.detach()), L.f32c(betas.detach()).reshape(-1)
        rad, rad_float = _radii(radii)
        vis = torch.empty(N, dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        nb = int(L.lib().bds_pvg_mask_temp_bytes(N))
        temp = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
        L.check(L.lib().bds_pvg_velocity_reg_fwd(N, M, float(T), L.ptr(_mask_u8(filter_mask)), L.ptr(rad), rad_float, L.ptr(v), L.ptr(b),
                                                 L.ptr(vis), L.ptr(out), L.ptr(temp), nb, L.stream()), "bds_pvg_velocity_reg_fwd")
        ctx.save_for_backward(v, b, vis)
        ctx.cfg = (float(T), betas.shape)
        ctx.mark_non_differentiable(out)
        return out[0].float(), out

    @staticmethod
    def backward(ctx, g_total, _g_out):
        v, b, vis = ctx.saved_tensors
        T, beta_shape = ctx.cfg
        N = v.shape[0]
        g_v = torch.empty(N, 3, device=v.device)
        g_b = torch.empty(beta_shape, device=v.device)
        scale = g_total.detach().reshape(1).float().contiguous()
        L.check(L.lib().bds_pvg_velocity_reg_bwd(N, T, L.ptr(vis), L.ptr(scale), L.ptr(v), L.ptr(b), L.ptr(g_v), L.ptr(g_b), L.stream()),
                "bds_pvg_velocity_reg_bwd")
        return g_v, g_b, None, None, None


def velocity_reg(velocity: Tensor, betas: Tensor, filter_mask: Tensor, radii: Tensor, T: float) -> Tuple[Tensor, Tensor]:
    """(total, out): ``total`` (0-d float32, differentiable towards ``velocity`` [N,3] and ``betas`` [N,1]) is the sum of
    |velocity exp(-0.5 exp(beta) / T)| over the rows kept by ``filter_mask`` [N] whose ``radii`` [M] entry is > 0; ``out`` [2]
    float64 on the device holds {that sum, the number of such rows} for ONE read-back.  The term of pvg.py:435 is
    ``total / count * w``."""
    return _VelocityReg.apply(velocity, betas, filter_mask, radii, T)


def _compute_reg_loss(self, owner) -> dict:
    """``PeriodicVibrationGaussians.compute_reg_loss`` (pvg.py:427-436): the inherited terms and ``velocity_reg``."""
    if not self._means.is_cuda:
        return owner._bds_reference_compute_reg_loss(self)
    loss_dict = super(owner, self).compute_reg_loss()
    cfg = self.reg_cfg.get("velocity_reg", None)
    if cfg:
        total, out = velocity_reg(self._velocity, self._betas, self.filter_mask, self.cur_radii, float(self.T))
        _, count = out.tolist()                                               # the sum arrives with it: one read-back
        if count:                                                             # no visible row: the key is absent (:433)
            loss_dict["velocity_reg"] = total / count * cfg.w
    return loss_dict


_SEAM = Seam()


def install(cls) -> None:
    """``install(models.gaussians.pvg.PeriodicVibrationGaussians)``: ``after_train``, ``refinement_after`` and ``compute_reg_loss``
    become the fused ones.  The originals stay reachable as ``cls._bds_reference_<name>``; ``uninstall`` puts them back."""
    def compute_reg_loss(self):
        return _compute_reg_loss(self, cls)
    for name, fn in (("after_train", after_train), ("refinement_after", refinement_after), ("compute_reg_loss", compute_reg_loss)):
        _SEAM.install(cls, {name: fn}, reference="_bds_reference_" + name)


def uninstall(*classes) -> None:
    _SEAM.uninstall(*classes)


# ---- the reference's sequence as framework ops ---------------------------------------------------------------------------------------
def framework_gamma(means: Tensor, scene_origin: Tensor, scene_scale: float) -> Tensor:
    g = (means - scene_origin).norm(dim=-1) * scene_scale - 1                 # pvg.py:96-97
    return torch.where(g <= 1, torch.ones_like(g), g) / scene_scale


def framework_after_train(stats: Optional[dict], filter_mask: Tensor, radii: Tensor, xys_grad: Tensor, taus_grad: Tensor,
                          last_size: int) -> dict:
    """pvg.py:100-133 on a dict of the four statistics (None: the initialising call); returns the dict (updated in place)."""
    N = filter_mask.numel()
    visible = (radii > 0).flatten()
    full = torch.zeros(N, device=radii.device, dtype=torch.bool)
    full[filter_mask] = visible
    grads = xys_grad.norm(dim=-1)
    t_grads = taus_grad.clone().abs().reshape(N, 1)[filter_mask].squeeze(-1)
    if stats is None:
        stats = dict(xys_grad_norm=torch.zeros(N, device=grads.device, dtype=grads.dtype),
                     t_grad_accum=torch.zeros(N, device=grads.device, dtype=grads.dtype))
        stats["xys_grad_norm"][filter_mask] = grads
        stats["t_grad_accum"][filter_mask] = t_grads
        stats["vis_counts"] = torch.ones_like(stats["xys_grad_norm"])
        stats["max_2Dsize"] = torch.zeros(N, device=radii.device, dtype=grads.dtype)
    else:
        stats["vis_counts"][full] = stats["vis_counts"][full] + 1
        stats["xys_grad_norm"][full] = grads[visible] + stats["xys_grad_norm"][full]
        stats["t_grad_accum"][full] = t_grads[visible] + stats["t_grad_accum"][full]
    new = (radii[visible] / float(last_size)).to(stats["max_2Dsize"].dtype)
    stats["max_2Dsize"][full] = torch.maximum(stats["max_2Dsize"][full], new)
    return stats


def _rotmat(quats: Tensor) -> Tensor:
    w, x, y, z = torch.unbind(F.normalize(quats, dim=-1), dim=-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)


def framework_decisions(P: dict, stats: dict, sch: dict, ctrl, scene_scale: float, scene_origin: Tensor) -> dict:
    """pvg.py:165-202: ``splits``, ``dups`` and the two child masks ``small_xyz`` (after the shrink), ``small_t``, each [N] bool."""
    vis = stats["vis_counts"]
    high_xyz = (stats["xys_grad_norm"] / vis > ctrl.densify_grad_thresh).reshape(-1)
    high_t = (stats["t_grad_accum"] / vis > ctrl.densify_t_grad_thresh).reshape(-1)
    high = high_xyz | high_t
    thr = ctrl.densify_size_thresh * scene_scale * framework_gamma(P["_means"], scene_origin, scene_scale)
    st = torch.exp(P["_betas"]).max(dim=1).values
    splits = (torch.exp(P["_scales"]).max(dim=-1).values > thr) | ((st > ctrl.densify_t_size_thresh) & high_t)
    if sch["by_screen"]:
        splits = splits | (stats["max_2Dsize"] > ctrl.split_screen_size).reshape(-1)
    splits = splits & high
    shrunk = torch.where(splits[:, None], torch.log(torch.exp(P["_scales"]) / SIZE_FAC), P["_scales"])      # :323
    small_xyz = torch.exp(shrunk).max(dim=-1).values <= thr
    small_t = st <= ctrl.densify_t_size_thresh
    dups = (small_xyz | (small_t & high_t)) & high
    return dict(splits=splits, dups=dups, small_xyz=small_xyz, small_t=small_t, shrunk=shrunk)


def framework_cull(P: dict, max_2Dsize: Optional[Tensor], sch: dict, ctrl, scene_scale: float, scene_origin: Tensor) -> Tensor:
    """pvg.py:267-284: the ``culls`` mask over the rows of ``P``."""
    culls = (torch.sigmoid(P["_opacities"]) < ctrl.cull_alpha_thresh).reshape(-1)
    if sch["cull_by_scale"]:
        gamma = framework_gamma(P["_means"], scene_origin, scene_scale)
        culls = culls | (torch.exp(P["_scales"]).max(dim=-1).values > ctrl.cull_scale_thresh * scene_scale * gamma)
        if sch["by_screen"]:
            culls = culls | (max_2Dsize > ctrl.cull_screen_size).reshape(-1)
    return culls


def framework_refinement(P: dict, M: Optional[dict], V: Optional[dict], stats: dict, step: int, ctrl, scene_scale: float,
                         scene_origin: Tensor, num_train_images: int, T: float, samples: Optional[Tensor]):
    """``refinement_after`` of the reference on dicts of the nine arrays ``P`` and their Adam moments ``M``, ``V`` (or None), in the
    tensors' own dtype and device -> (P, M, V, counts).  ``samples`` [samps * n_split, 4] as ``refinement_after`` takes them (or a
    function of the row count).  ``P`` may leave out arrays no decision reads (the features); ``counts`` also carries ``parent``
    (the input row of every row before the cull), ``pre_cull`` (those rows) and ``culls`` (their mask)."""
    N = P["_means"].shape[0]
    attrs = tuple(a for a in ATTRS if a in P)
    sch = schedule(step, ctrl, num_train_images, N)
    counts = dict(split=0, dup=0, cull=0)
    P = dict(P)
    M = None if M is None else dict(M)
    V = None if V is None else dict(V)
    if step <= ctrl.warmup_steps:
        return P, M, V, counts
    max_2Dsize = stats.get("max_2Dsize")
    if sch["do_densify"]:
        d = framework_decisions(P, stats, sch, ctrl, scene_scale, scene_origin)
        sm, dm, samps = d["splits"], d["dups"], int(ctrl.n_split_samples)
        n_split = int(sm.sum().item())
        rep = lambda t: t[sm].repeat(samps, *([1] * (t.dim() - 1)))
        if callable(samples):
            samples = samples(samps * n_split)
        counts["samples"] = samples
        noise, z = samples[:, :3].to(P["_means"].dtype), samples[:, 3:4].to(P["_means"].dtype)
        assert samples.shape[0] == samps * n_split
        scaled = rep(torch.exp(P["_scales"])) * noise
        quats = P["_quats"][sm]
        quats = quats / quats.norm(dim=-1, keepdim=True)
        rotated = torch.bmm(_rotmat(quats.repeat(samps, 1)), scaled[..., None]).squeeze(-1)
        new_means = rotated + rep(P["_means"])
        st = torch.exp(P["_betas"])
        samples_t = torch.zeros_like(z) + rep(st) * z                                                  # :330-332
        new_taus = samples_t + rep(P["_taus"])
        velocity = P["_velocity"] * torch.exp(-0.5 * (st / T))
        new_means = new_means + rep(velocity) * samples_t
        new_scales = rep(d["shrunk"])
        sx = d["small_xyz"][sm].repeat(samps)
        new_scales[sx] = torch.log(torch.exp(rep(d["shrunk"])))[sx]                                   # :343-345
        new_betas = torch.log(rep(st) / SIZE_FAC)
        stm = d["small_t"][sm].repeat(samps)
        new_betas[stm] = torch.log(rep(st))[stm]
        if _ctrl_get(ctrl, "no_time_split", False):
            new_betas = torch.log(rep(st))
        split_children = {"_means": new_means, "_scales": new_scales, "_taus": new_taus, "_betas": new_betas}
        P["_scales"] = d["shrunk"]
        new = {}
        for a in attrs:
            new[a] = torch.cat([P[a], split_children[a] if a in split_children else rep(P[a]), P[a][dm]], dim=0)
        n_add = new["_means"].shape[0] - N
        for S in (M, V):
            if S is not None:
                for a in attrs:
                    S[a] = torch.cat([S[a], torch.zeros((n_add,) + tuple(S[a].shape[1:]), dtype=S[a].dtype, device=S[a].device)], dim=0)
        P = new
        max_2Dsize = torch.cat([max_2Dsize, torch.zeros(n_add, dtype=max_2Dsize.dtype, device=max_2Dsize.device)])
        counts.update(split=n_split, dup=int(dm.sum().item()), decisions=d,
                      parent=torch.cat([torch.arange(N, device=sm.device), torch.where(sm)[0].repeat(samps), torch.where(dm)[0]]))
    if sch["do_cull"]:
        culls = framework_cull(P, max_2Dsize, sch, ctrl, scene_scale, scene_origin)
        counts.update(pre_cull=P, culls=culls, pre_cull_max_2Dsize=max_2Dsize)
        keep = ~culls
        P = {a: P[a][keep] for a in attrs}
        for S in (M, V):
            if S is not None:
                for a in attrs:
                    S[a] = S[a][keep]
        counts["cull"] = int(culls.sum().item())
    if sch["do_reset"]:
        op = torch.sigmoid(P["_opacities"])
        P["_opacities"] = torch.logit(torch.min(op, torch.ones_like(op) * ctrl.reset_alpha_value))
        for S in (M, V):
            if S is not None:
                S["_opacities"] = torch.zeros_like(S["_opacities"])
    return P, M, V, counts


def framework_velocity_reg(velocity: Tensor, betas: Tensor, filter_mask: Tensor, radii: Tensor, T: float) -> Optional[Tensor]:
    """pvg.py:433-435 without the weight: the mean over the visible kept rows, None when there is none."""
    seen = radii.reshape(-1) > 0
    if not bool(seen.sum()):
        return None
    v = (velocity * torch.exp(-0.5 * (torch.exp(betas) / T))).norm(dim=-1)[filter_mask]
    return v[seen].mean()
