"""Image loss of the training step on the path's outputs (reference:
models/trainers/base.py:518-565 + models/losses.py, affine TV :590-594 + models/modules.py:445,466-472):
``photometric_tv_loss`` (L1 + per-level TV as ONE node accumulating into one device scalar -- the benchmark's loss),
``ssim`` / ``ssim_loss``, and ``image_terms``: all six image terms of ``compute_losses`` at every option of models/losses.py as one node,
with ``install`` / ``uninstall`` of that method.

There is ONE node for the per-pixel terms (``_ImageLoss``, over ``bds_image_loss_fwd`` / ``_bwd``).  ``pixel_loss`` (rgb L1 + sky-mask BCE +
lidar depth, the first three terms at the trainer's default options) and ``reg_losses`` (opacity entropy + inverse-depth smoothness +
dynamic-region L1, the last three, unweighted) are its two older option sets, kept as names: each is one call of ``image_terms``."""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam
from .bilagrid import _levels_struct


class _PhotometricTV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb: Tensor, target: Tensor, tv_weights: tuple, grid_grads, *grids: Tensor):
        L.require_gpu(rgb, target, *grids)
        lib, st = L.lib(), L.stream()
        assert rgb.shape == target.shape and rgb.dtype == torch.float32 and target.dtype == torch.float32
        rgb, target = L.f32c_aligned(rgb), L.f32c_aligned(target)      # bds_l1_mean_fwd reads 16 bytes at a time: a row slice of an image is copied
        grids = [g.contiguous() for g in grids]
        out = torch.zeros(1, device=rgb.device, dtype=torch.float32)
        L.check(lib.bds_l1_mean_fwd(rgb.numel(), L.ptr(rgb), L.ptr(target), L.ptr(out), st), "bds_l1_mean_fwd")
        if grids:
            lv = _levels_struct(grids, None, [1] * len(grids))
            wts = (C.c_float * len(grids))(*[float(w) for w in tv_weights])
            L.check(lib.bds_bilagrid_tv_ms_fwd(len(grids), lv, wts, L.ptr(out), st), "bds_bilagrid_tv_ms_fwd")
        ctx.save_for_backward(rgb, target, *grids)
        ctx.tv_weights = tuple(float(w) for w in tv_weights)
        ctx.grid_grads = grid_grads
        return out.reshape(())

    @staticmethod
    def backward(ctx, v_out):
        rgb, target, *grids = ctx.saved_tensors
        lib, st = L.lib(), L.stream()
        v = v_out.reshape(1).to(torch.float32).contiguous()
        v_rgb = None
        if ctx.needs_input_grad[0]:
            v_rgb = torch.empty_like(rgb)
            L.check(lib.bds_l1_mean_bwd(rgb.numel(), L.ptr(rgb), L.ptr(target), L.ptr(v), L.ptr(v_rgb), st), "bds_l1_mean_bwd")
        v_grids = [None] * len(grids)
        need = [ctx.needs_input_grad[4 + i] for i in range(len(grids))]
        if any(need) and ctx.grid_grads is not None:    # add in place to the caller's accumulators, return nothing
            sel = [g for i, g in enumerate(grids) if need[i]]
            sel_v = [a for i, a in enumerate(ctx.grid_grads) if need[i]]
            lv = _levels_struct(sel, sel_v, [1] * len(sel))
            wts = (C.c_float * len(sel))(*[ctx.tv_weights[i] for i in range(len(grids)) if need[i]])
            L.check(lib.bds_bilagrid_tv_ms_bwd(len(sel), lv, wts, L.ptr(v), st), "bds_bilagrid_tv_ms_bwd")
        elif any(need):
            sizes = [(g.numel() + 3) // 4 * 4 if need[i] else 0 for i, g in enumerate(grids)]   # 16-byte aligned slices
            flat = torch.zeros(sum(sizes), device=rgb.device, dtype=torch.float32)               # one fill for all levels
            off, sel, sel_v, sel_w = 0, [], [], []
            for i, g in enumerate(grids):
                if not need[i]:
                    continue
                vg = flat[off:off + g.numel()].view(g.shape)
                off += sizes[i]
                v_grids[i] = vg
                sel.append(g); sel_v.append(vg); sel_w.append(ctx.tv_weights[i])
            lv = _levels_struct(sel, sel_v, [1] * len(sel))
            wts = (C.c_float * len(sel))(*sel_w)
            L.check(lib.bds_bilagrid_tv_ms_bwd(len(sel), lv, wts, L.ptr(v), st), "bds_bilagrid_tv_ms_bwd")
        return (v_rgb, None, None, None, *v_grids)


def loss_slots(dev) -> Tensor:
    """Zeroed accumulator of the one-launch training losses: LOSS_SLOTS slots, LOSS_SLOT_STRIDE floats apart (``slots_value``)."""
    return torch.zeros(L.LOSS_SLOTS * L.LOSS_SLOT_STRIDE, device=dev, dtype=torch.float32)


def slots_value(buf: Tensor) -> Tensor:
    return buf.view(L.LOSS_SLOTS, L.LOSS_SLOT_STRIDE)[:, 0].sum()


def photometric_tv_train(rgb: Tensor, target: Tensor, grids: Sequence[Tensor], tv_weights: Sequence[float], grid_grads: Sequence[Tensor],
                         slots: bool = False):
    """The direct step's loss (no autograd graph; ``fused_view.train_view``): value and gradient of
    mean|rgb - target| + sum_l tv_weights[l] * total_variation(grids[l]) in ONE launch (``bds_l1_tv_train``): returns
    (loss [0-d], v_rgb); the TV gradient is ADDED to ``grid_grads`` (the grids' ``.grad`` slices) with atomics.
    ``slots=True``: the first result is the slotted accumulator instead (``slots_value`` sums it: a caller with a better place for
    that small reduction than right behind this launch)."""
    L.require_gpu(rgb, target, *grids)
    lib, st = L.lib(), L.stream()
    assert rgb.shape == target.shape and rgb.dtype == torch.float32 and target.dtype == torch.float32
    rgb, target = L.f32c_aligned(rgb), L.f32c_aligned(target)      # bds_l1_tv_train: 16-byte aligned a, b (and v_a, allocated here)
    grids = [g.contiguous() for g in grids]
    assert len(grid_grads) == len(grids) and all(a.numel() == g.numel() and a.is_contiguous() for a, g in zip(grid_grads, grids))
    out = loss_slots(rgb.device)
    v_rgb = torch.empty_like(rgb)
    lv = _levels_struct(grids, list(grid_grads), [1] * len(grids)) if grids else None
    wts = (C.c_float * max(len(grids), 1))(*[float(w) for w in tv_weights])
    L.check(lib.bds_l1_tv_train(rgb.numel(), L.ptr(rgb), L.ptr(target), len(grids), lv, wts, 1.0, L.ptr(out), L.LOSS_SLOTS, L.ptr(v_rgb), st),
            "bds_l1_tv_train")
    return (out if slots else slots_value(out)), v_rgb


def photometric_tv_loss(rgb: Tensor, target: Tensor, grids: Sequence[Tensor], tv_weights: Sequence[float],
                        grid_grads: Sequence[Tensor] = None) -> Tensor:
    """mean|rgb - target| + sum_l tv_weights[l] * total_variation(grids[l])  (grids [n_img,12,L,gy,gx]).
    ``grid_grads`` (optional, one tensor per grid, same shapes): the TV gradient is ADDED to these in place (accumulators that
    already are the grids' ``.grad``, ``dist.FrameExchange.tail_grads()``) and autograd receives no gradient for the grids."""
    assert len(grids) == len(tv_weights)
    if grid_grads is not None:
        assert len(grid_grads) == len(grids) and all(a.numel() == g.numel() and a.is_contiguous() for a, g in zip(grid_grads, grids))
        grid_grads = list(grid_grads)
    return _PhotometricTV.apply(rgb, target, tuple(tv_weights), grid_grads, *grids)


class _SSIM(torch.autograd.Function):
    """mean SSIM(target, pred) of [H,W,C] images: pytorch_msssim.SSIM(data_range=1, size_average=True) as the reference
    trainer calls it (models/trainers/base.py:114,541); gradient w.r.t. pred only (the ground truth is data)."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor):
        L.require_gpu(pred, target)
        lib, st = L.lib(), L.stream()
        pred, target = pred.contiguous(), target.contiguous()
        assert pred.shape == target.shape and pred.dim() == 3 and pred.dtype == torch.float32 and target.dtype == torch.float32
        H, W, CH = pred.shape
        if H < 11 or W < 11:
            raise ValueError("SSIM needs images of at least 11x11 pixels (window 11, valid region)")
        out = torch.zeros(1, device=pred.device, dtype=torch.float32)
        ws = None
        if ctx.needs_input_grad[0]:
            ws = torch.empty(lib.bds_ssim_workspace_bytes(H, W, CH), device=pred.device, dtype=torch.uint8)
        L.check(lib.bds_ssim_fwd(H, W, CH, L.ptr(target), L.ptr(pred), L.ptr(out), L.ptr(ws), 0 if ws is None else ws.numel(), st),
                "bds_ssim_fwd")
        ctx.save_for_backward(pred, target, ws)
        return out.reshape(())

    @staticmethod
    def backward(ctx, v_out):
        pred, target, ws = ctx.saved_tensors
        if ws is None:
            return None, None
        H, W, CH = pred.shape
        v = v_out.reshape(1).to(torch.float32).contiguous()
        v_pred = torch.empty_like(pred)
        L.check(L.lib().bds_ssim_bwd(H, W, CH, L.ptr(target), L.ptr(pred), L.ptr(ws), ws.numel(), L.ptr(v), L.ptr(v_pred), L.stream()),
                "bds_ssim_bwd")
        return v_pred, None


def ssim(pred: Tensor, target: Tensor) -> Tensor:
    """Mean structural similarity of two [H,W,C] images in [0,1] (11x11 Gaussian window, valid region)."""
    return _SSIM.apply(pred, target)


def ssim_loss(pred: Tensor, target: Tensor) -> Tensor:
    """1 - ssim: the reference's `ssim_loss` before its weight (models/trainers/base.py:541-544)."""
    return 1.0 - ssim(pred, target)


# ---- the whole image loss under compute_losses --------------------------------------------------------------------------------------
IMAGE_TERMS = ("rgb_loss", "sky_loss_opacity", "depth_loss", "opacity_entropy_loss", "inverse_depth_smoothness_loss", "vehicle_region_rgb_loss")
_MASK_KINDS = {"bce": 1, "safe_bce": 2}
_DEPTH_TYPES = {"l1": 0, "l2": 1, "smooth_l1": 2}
_DEPTH_REDUCTIONS = {"mean_on_hit": 0, "mean_on_hw": 1, "sum": 2}


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, opacity, depth, pixels, sky_masks, lidar, egocar, dyn_opacity, cfg):
        L.require_gpu(rgb, opacity, depth, pixels, sky_masks, lidar, egocar, dyn_opacity)
        lib = L.lib()
        rgb, opacity, depth, pixels, sky_masks, lidar, egocar, dyn_opacity = (L.f32c(t) for t in (rgb, opacity, depth, pixels, sky_masks, lidar,
                                                                                                   egocar, dyn_opacity))
        assert rgb.dim() == 3 and rgb.shape[-1] == 3 and pixels.shape == rgb.shape
        H, W = rgb.shape[0], rgb.shape[1]
        for t in (opacity, depth, sky_masks, lidar, egocar, dyn_opacity):
            assert t is None or t.numel() == H * W, "per-pixel inputs must have H*W elements"
        mask_kind, safe_limit, depth_type, normalize, inverse, max_depth, reduction, entropy, smoothness, dyn_threshold, weights = cfg
        images = (H, W, L.ptr(rgb), L.ptr(pixels), L.ptr(opacity), L.ptr(depth), L.ptr(sky_masks), L.ptr(lidar), L.ptr(egocar), L.ptr(dyn_opacity))
        options = (mask_kind, safe_limit, depth_type, normalize, inverse, max_depth, reduction, entropy, smoothness, dyn_threshold,
                   (C.c_float * 6)(*weights))
        terms = torch.empty(6, device=rgb.device, dtype=torch.float32)
        sums = torch.empty(9, device=rgb.device, dtype=torch.float32)
        temp = torch.empty(lib.bds_image_loss_temp_bytes(H, W), device=rgb.device, dtype=torch.uint8)
        L.check(lib.bds_image_loss_fwd(*images, *options, L.ptr(terms), L.ptr(sums), L.ptr(temp), temp.numel(), L.stream()), "bds_image_loss_fwd")
        ctx.save_for_backward(rgb, opacity, depth, pixels, sky_masks, lidar, egocar, dyn_opacity, sums)
        ctx.cfg = cfg
        return terms

    @staticmethod
    def backward(ctx, v_terms):
        rgb, opacity, depth, pixels, sky_masks, lidar, egocar, dyn_opacity, sums = ctx.saved_tensors
        mask_kind, safe_limit, depth_type, normalize, inverse, max_depth, reduction, entropy, smoothness, dyn_threshold, weights = ctx.cfg
        H, W = rgb.shape[0], rgb.shape[1]
        v_terms = L.f32c(v_terms)
        v_rgb = torch.empty_like(rgb) if ctx.needs_input_grad[0] else None
        v_op = torch.empty_like(opacity) if (opacity is not None and ctx.needs_input_grad[1]) else None   # (all of its terms off: zeros)
        v_dp = torch.empty_like(depth) if (depth is not None and ctx.needs_input_grad[2]) else None
        images = (H, W, L.ptr(rgb), L.ptr(pixels), L.ptr(opacity), L.ptr(depth), L.ptr(sky_masks), L.ptr(lidar), L.ptr(egocar), L.ptr(dyn_opacity))
        options = (mask_kind, safe_limit, depth_type, normalize, inverse, max_depth, reduction, entropy, smoothness, dyn_threshold,
                   (C.c_float * 6)(*weights))
        L.check(L.lib().bds_image_loss_bwd(*images, *options, L.ptr(sums), L.ptr(v_terms), L.ptr(v_rgb), L.ptr(v_op), L.ptr(v_dp), L.stream()),
                "bds_image_loss_bwd")
        return v_rgb, v_op, v_dp, None, None, None, None, None, None


def image_terms(rgb: Tensor, pixels: Tensor, opacity: Tensor = None, depth: Tensor = None, sky_masks: Tensor = None, lidar_depth: Tensor = None,
                egocar_masks: Tensor = None, dyn_opacity: Tensor = None, *, weights: Sequence[float], mask_loss: str = "bce",
                safe_limit: float = 0.1, depth_loss_type: str = "l1", depth_normalize: bool = False, depth_inverse: bool = False,
                max_depth: float = 80.0, depth_reduction: str = "mean_on_hit", entropy: bool = False, smoothness: bool = False,
                dyn_threshold: float = 0.2) -> Tensor:
    """The image loss of ``BasicTrainer.compute_losses`` (models/trainers/base.py:518-585, 638-652) in ONE pass each way at every option of
    models/losses.py: returns the six WEIGHTED terms in the order of ``IMAGE_TERMS`` (``weights``: six host floats, so a decayed depth
    weight costs no device work); the terms and their gradients are bit-identical run to run.  rgb / pixels [H,W,3]; opacity, depth,
    dyn_opacity [H,W,1] or [H,W]; sky_masks, lidar_depth, egocar_masks [H,W].

    A term is on where its images are given: the sky term with ``opacity`` and ``sky_masks`` (``mask_loss``: ``"bce"`` or ``"safe_bce"``
    with ``safe_limit``), the depth term with ``depth`` and ``lidar_depth`` (``DepthLoss(loss_type, normalize, use_inverse_depth,
    upper_bound=max_depth, reduction)``), the dynamic-region term with ``dyn_opacity`` (``outputs["Dynamic_opacity"]``, data as the
    reference's ``.data``; 0 when no pixel qualifies, where the reference adds no term); ``entropy`` (needs ``opacity``) and
    ``smoothness`` (needs ``depth``) are flags.  A term that is off is 0.  ``depth_reduction="none"`` and a depth-error percentile are not
    built."""
    if len(weights) != 6:
        raise ValueError("weights: one per term of IMAGE_TERMS")
    if sky_masks is not None and mask_loss not in _MASK_KINDS:
        raise NotImplementedError(f"Unknown loss type: {mask_loss}")
    if depth_loss_type not in _DEPTH_TYPES:
        raise NotImplementedError(f"Unknown loss type: {depth_loss_type}")
    if depth_reduction not in _DEPTH_REDUCTIONS:
        raise NotImplementedError(f"Unknown reduction method: {depth_reduction}")
    if (sky_masks is not None and opacity is None) or (lidar_depth is not None and depth is None):
        raise ValueError("sky_masks needs opacity and lidar_depth needs depth")
    if (entropy and opacity is None) or (smoothness and depth is None):
        raise ValueError("entropy needs opacity and smoothness needs depth")
    cfg = (_MASK_KINDS[mask_loss] if sky_masks is not None else 0, float(safe_limit), _DEPTH_TYPES[depth_loss_type], int(bool(depth_normalize)),
           int(bool(depth_inverse)), float(max_depth), _DEPTH_REDUCTIONS[depth_reduction], int(bool(entropy)), int(bool(smoothness)),
           float(dyn_threshold), tuple(float(w) for w in weights))
    return _ImageLoss.apply(rgb, opacity, depth, pixels, sky_masks, lidar_depth, egocar_masks, None if dyn_opacity is None else dyn_opacity.detach(),
                            cfg)


def pixel_loss(rgb: Tensor, opacity: Tensor, depth: Tensor, pixels: Tensor, sky_masks: Tensor, lidar_depth: Tensor,
               egocar_masks: Tensor = None, w_rgb: float = 0.8, w_mask: float = 0.05, w_depth: float = 0.01,
               depth_loss_type: str = "l1", max_depth: float = 80.0) -> Tensor:
    """The per-pixel terms of ``BasicTrainer.compute_losses`` (models/trainers/base.py:518-565) in one pass each way:
    returns the three WEIGHTED terms ``[rgb_loss, sky_loss_opacity, depth_loss]`` (sum them for the total; they are what
    the trainer logs).  rgb / pixels [H,W,3]; opacity, depth [H,W,1] or [H,W]; sky_masks, lidar_depth, egocar_masks [H,W].
    Pass ``opacity=None`` / ``depth=None`` to drop a term."""
    if depth_loss_type not in ("l1", "l2"):
        raise NotImplementedError(f"Unknown loss type: {depth_loss_type}")   # DepthLoss (models/losses.py:150) also has smooth_l1
    if rgb.dim() != 3:                                                        # any shape ending in 3: no term here looks at a neighbour
        rgb, pixels = rgb.reshape(1, -1, 3), pixels.reshape(1, -1, 3)
    use_mask = opacity is not None and sky_masks is not None and w_mask != 0.0
    use_depth = depth is not None and lidar_depth is not None and w_depth != 0.0
    return image_terms(rgb, pixels, opacity, depth, sky_masks if use_mask else None, lidar_depth if use_depth else None, egocar_masks,
                       weights=(w_rgb, w_mask, w_depth, 0.0, 0.0, 0.0), depth_loss_type=depth_loss_type, max_depth=max_depth)[:3]


def reg_losses(pixels: Tensor, opacity: Tensor = None, depth: Tensor = None, rgb: Tensor = None, dyn_opacity: Tensor = None,
               egocar_masks: Tensor = None, dyn_threshold: float = 0.2) -> Tensor:
    """The regularisers of ``BasicTrainer.compute_losses`` (models/trainers/base.py:566-585, 638-659) in one pass each way; returns the
    three UNWEIGHTED terms ``[opacity_entropy, inverse_depth_smoothness, dynamic_region_l1]`` (the trainer multiplies them by
    ``losses.opacity_entropy.w`` / ``losses.inverse_depth_smoothness.w`` / ``losses.dynamic_region.w``).  pixels / rgb [H,W,3];
    opacity, depth, dyn_opacity (``outputs["Dynamic_opacity"]``, treated as data like the reference's ``.data``) [H,W,1] or [H,W].
    Pass ``None`` to drop a term (it is then 0).  The dynamic-region term is 0 when no pixel qualifies (the reference adds none)."""
    if dyn_opacity is None:      # the rgb term has weight 0 and no other term reads rgb: it may be absent, and it gets no gradient
        rgb = pixels.detach()
    return image_terms(rgb, pixels, opacity, depth, egocar_masks=egocar_masks, dyn_opacity=dyn_opacity, weights=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0),
                       entropy=opacity is not None, smoothness=depth is not None, dyn_threshold=dyn_threshold)[3:]


def _affine_loss(self, affine_reg, outputs, image_infos, valid):
    """The affine branch of compute_losses (models/trainers/base.py:587-635) on whatever module the trainer holds -> the term, or None."""
    kind = self.model_config.Affine.type
    model = self.models["Affine"]

    def identity_term(affine_trs):
        reg_mat, reg_shift = torch.eye(3, device=self.device), torch.zeros(3, device=self.device)
        return torch.abs(affine_trs[..., :3, :3] - reg_mat).mean() + torch.abs(affine_trs[..., :3, 3:] - reg_shift).mean()

    masked = lambda img: img if valid is None else img * valid[..., None]
    if kind in ("models.modules.BilateralAffineTransform", "models.modules.NeuralBilateralAffineTransform",
                "models.modules.MultiScaleNeuralBilateralAffineTransform"):
        return affine_reg.w * model.tv_loss()
    if kind == "models.modules.AffineTransform":
        return affine_reg.w * identity_term(model({"img_idx": image_infos["img_idx"].flatten()[0]}))
    if kind == "models.modules.MultiTransform":
        img_idx = image_infos["img_idx"].flatten()[0]
        if img_idx % 3 == 0:
            return affine_reg.w * model.tv_loss()
        return affine_reg.w * identity_term(model(masked(outputs["rgb"]), {"img_idx": image_infos["img_idx"].flatten()[0]}))
    if kind == "models.modules.MultiScaleBilateralAffineTransform":
        loss_affine = model.tv_loss()
        original_rgb = masked(outputs["original_rgb"])          # (a KeyError where the render left none: SURVEY.md Q1, as the reference)
        return affine_reg.w * loss_affine + affine_reg.w1 * model.inverse_loss(masked(image_infos["pixels"]), original_rgb)
    return None


def _on_device(outputs) -> bool:
    return outputs["rgb"].is_cuda


def image_compute_losses(self, outputs, image_infos, cam_infos):
    """``BasicTrainer.compute_losses`` (models/trainers/base.py:518-659): the reference's keys in the reference's order, the six image
    terms from ``image_terms`` (one node), SSIM from ``ssim_loss``, the affine and per-class regularisers from the trainer's own modules.
    Deviations: ``vehicle_region_rgb_loss`` is present with value 0 where no pixel qualifies (the reference leaves the key out after a
    host read-back); the images are read as contiguous float32.  CPU tensors take the class's own method."""
    if not _on_device(outputs):
        return type(self)._bds_reference_compute_losses(self, outputs, image_infos, cam_infos)
    ld = self.losses_dict
    ego = image_infos["egocar_masks"] if "egocar_masks" in image_infos else None
    valid = None if ego is None else (1.0 - ego).float()
    rgb, pixels = outputs["rgb"], image_infos["pixels"]
    kw, w = {}, [float(ld.rgb.w), 0.0, 0.0, 0.0, 0.0, 0.0]
    if self.sky_opacity_loss_fn is not None:
        kw.update(sky_masks=image_infos["sky_masks"], mask_loss=ld.mask.opacity_loss_type)        # (_init_losses, :230-239: limit 0.1)
        w[1] = float(ld.mask.w)
    fn = self.depth_loss_fn
    if fn is not None:
        if getattr(fn, "depth_error_percentile", None) is not None:
            raise NotImplementedError("depth_error_percentile is not built")
        decay = ld.depth.get("lidar_w_decay", -1)
        w[2] = float(ld.depth.w * (math.exp(-self.step / 8000 * decay) if decay > 0 else 1))
        kw.update(lidar_depth=image_infos["lidar_depth_map"], depth_loss_type=fn.loss_type, depth_normalize=fn.normalize,
                  depth_inverse=fn.use_inverse_depth, max_depth=fn.upper_bound, depth_reduction=fn.reduction)
    entropy, smooth, dyn = ld.get("opacity_entropy", None), ld.get("inverse_depth_smoothness", None), ld.get("dynamic_region", None)
    if entropy is not None:
        w[3] = float(entropy.w)
    if smooth is not None:
        w[4] = float(smooth.w)
    dyn_on = False
    if dyn is not None:
        start_from = dyn.get("start_from", 0)
        if self.step == start_from:
            self.render_dynamic_mask = True
        dyn_on = self.step > start_from and "Dynamic_opacity" in outputs
        w[5] = float(dyn.get("w", 1.0))
    need_opacity, need_depth = "sky_masks" in kw or entropy is not None, fn is not None or smooth is not None
    terms = image_terms(rgb, pixels, outputs["opacity"] if need_opacity else None, outputs["depth"] if need_depth else None,
                        egocar_masks=ego, dyn_opacity=outputs["Dynamic_opacity"] if dyn_on else None, weights=w,
                        entropy=entropy is not None, smoothness=smooth is not None, **kw)
    loss_dict = {"rgb_loss": terms[0],
                 "ssim_loss": ld.ssim.w * ssim_loss(rgb if valid is None else rgb * valid[..., None],
                                                    pixels if valid is None else pixels * valid[..., None])}
    for k, on in ((1, "sky_masks" in kw), (2, fn is not None), (3, entropy is not None), (4, smooth is not None)):
        if on:
            loss_dict[IMAGE_TERMS[k]] = terms[k]
    affine_reg = ld.get("affine", None)
    if affine_reg is not None and "Affine" in self.models:
        loss_affine = _affine_loss(self, affine_reg, outputs, image_infos, valid)
        if loss_affine is not None:
            loss_dict["affine_loss"] = loss_affine
    if dyn_on:
        loss_dict[IMAGE_TERMS[5]] = terms[5]
    for class_name in self.gaussian_classes.keys():
        for k, v in self.models[class_name].compute_reg_loss().items():
            loss_dict[f"{class_name}_{k}"] = v
    return loss_dict


_SEAM = Seam()


def install(trainer_class) -> None:
    """``install(models.trainers.base.BasicTrainer)``: the class's ``compute_losses`` becomes ``image_compute_losses`` (``MultiTrainer`` and
    ``SingleTrainer`` only call ``super()``).  The original stays reachable as ``trainer_class._bds_reference_compute_losses``;
    ``uninstall`` puts it back.  Needs neither ``kornia`` nor ``pytorch_msssim``."""
    _SEAM.install(trainer_class, {"compute_losses": image_compute_losses}, reference="_bds_reference_compute_losses")


def uninstall(*trainer_classes) -> None:
    _SEAM.uninstall(*trainer_classes)
