"""Time transform of the periodic-vibration Gaussians as a fused HIP op (csrc/pvg.hip through ``bds_pvg_fwd / _bwd``).

Reference: ``PeriodicVibrationGaussians.get_gaussians`` (models/gaussians/pvg.py:374-425) evaluates, every step over all N points, the
marginal and the temporal means / opacities (:65-88), the activations, a concatenation of the two SH parameters, a dense SH pass,
five boolean-mask gathers and ten NaN / Inf reductions, each gather and reduction with a host wait of its own.

* ``time_transform(...)`` is the autograd op: the five tensors of the kept rows (``marg > 0.05``) compacted in the original order,
  and the bool mask.  Three launches forward, one backward; the row count M and the NaN / Inf flags of the five tensors reach the
  host in ONE read-back (the outputs are allocated for N rows and returned as ``narrow(0, 0, M)`` views).  The drop-in adds one
  more read, of the call's time scalars, where the class keeps its timestamps on the device.
* ``install(cls)`` / ``uninstall(cls)`` swap ``get_gaussians`` on the reference's own class; CPU tensors keep the class's own method.
  Nothing is installed by default.
* ``framework_transform(...)`` is the same expression as framework ops (tests, and the A side of scripts/pvg_time.py)."""
from __future__ import annotations

import math
import random
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam

GS_KEYS = ("_means", "_opacities", "_rgbs", "_scales", "_quats")   # the order of get_gaussians' dict and of its NaN / Inf check
KEEP = 0.05                                                        # pvg.py:389


def sh_colors(degrees_to_use: int, dirs: Tensor, coeffs: Tensor) -> Tensor:
    """Real SH up to degree 3 of unit ``dirs`` [N,3] with ``coeffs`` [N,K,3] as framework ops (the recurrences of csrc/gs_math.h)."""
    x, y, z = dirs.unbind(-1)
    B = [torch.full_like(x, 0.2820947917738781)]
    if degrees_to_use >= 1:
        B += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if degrees_to_use >= 2:
        z2, t0b, c1, s1 = z * z, -1.092548430592079 * z, x * x - y * y, 2.0 * x * y
        B += [0.5462742152960395 * s1, t0b * y, 0.9461746957575601 * z2 - 0.3153915652525201, t0b * x, 0.5462742152960395 * c1]
    if degrees_to_use >= 3:
        t0c, t1b = -2.285228997322329 * z2 + 0.4570457994644658, 1.445305721320277 * z
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        B += [-0.5900435899266435 * s2, t1b * s1, t0c * y, z * (1.865881662950577 * z2 - 1.119528997770346), t0c * x, t1b * c1,
              -0.5900435899266435 * c2]
    Bm = torch.stack(B, -1)
    return (Bm[..., None] * coeffs[:, :Bm.shape[-1], :]).sum(1)


def framework_transform(means: Tensor, velocity: Tensor, taus: Tensor, betas: Tensor, logits: Tensor, log_scales: Tensor, quats: Tensor,
                        features_dc: Tensor, features_rest: Tensor, cam_pos: Tensor, cur_time: float, delta_t: float, in_smooth: bool,
                        T: float, degrees_to_use: int, sh: Optional[Callable] = None):
    """The time transform as framework ops over ALL rows: (means, opacities, rgbs, scales, quats, keep mask [N] bool).  The caller
    gathers ``x[mask]``.  ``sh(degrees_to_use, dirs, coeffs [N,K,3])``: the SH evaluation (default: ``sh_colors``)."""
    a = 1.0 / T * math.pi * 2
    s_t = torch.exp(betas)
    marg = torch.exp(-0.5 * (taus - cur_time) ** 2 / s_t ** 2)
    mask = (marg > KEEP).reshape(-1)
    out_means = means + velocity * torch.sin((cur_time - taus) * a) / a
    if in_smooth:
        out_means = out_means + velocity * torch.exp(-0.5 * (s_t / T)) * delta_t
    opacities = torch.sigmoid(logits) * marg
    scales = torch.exp(log_scales)
    out_quats = quats / quats.norm(dim=-1, keepdim=True)
    if features_rest.shape[1] > 0:
        dirs = out_means.detach() - cam_pos.reshape(-1)[:3]
        dirs = dirs / dirs.norm(dim=-1, keepdim=True)
        colors = torch.cat((features_dc[:, None, :], features_rest), dim=1)
        rgbs = torch.clamp((sh or sh_colors)(degrees_to_use, dirs, colors) + 0.5, 0.0, 1.0)
    else:
        rgbs = torch.sigmoid(features_dc)
    return out_means, opacities, rgbs, scales, out_quats, mask


class _TimeTransform(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, velocity, taus, betas, logits, log_scales, quats, features_dc, features_rest, cam_pos, cfg, info):
        L.require_gpu(means, velocity, taus, betas, logits, log_scales, quats, features_dc, features_rest, cam_pos)
        cur_time, delta_t, in_smooth, T, deg = cfg
        N = means.shape[0]
        K = features_rest.shape[1] + 1
        assert velocity.shape == (N, 3) and taus.numel() == N and betas.numel() == N and logits.numel() == N
        assert log_scales.shape == (N, 3) and quats.shape == (N, 4) and features_dc.shape == (N, 3) and features_rest.shape == (N, K - 1, 3)
        dev = means.device
        m, v, ta, be, lg, ls, q, dc, rest = (L.f32c(x.detach()) for x in (means, velocity, taus, betas, logits, log_scales, quats,
                                                                          features_dc, features_rest))
        cam = L.f32c(cam_pos.detach()).reshape(-1)[:3].contiguous()
        o_m, o_o, o_c, o_s, o_q, raw = (torch.empty(N, w, device=dev) for w in (3, 1, 3, 3, 4, 3))
        mask = torch.empty(N, dtype=torch.bool, device=dev)
        nbytes = int(L.lib().bds_pvg_temp_bytes(N))
        temp = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        L.check(L.lib().bds_pvg_fwd(N, K, deg, cur_time, delta_t, int(in_smooth), T, L.ptr(m), L.ptr(v), L.ptr(ta), L.ptr(be), L.ptr(lg),
                                    L.ptr(ls), L.ptr(q), L.ptr(dc), L.ptr(rest) if K > 1 else None, L.ptr(cam), L.ptr(o_m), L.ptr(o_o),
                                    L.ptr(o_c), L.ptr(o_s), L.ptr(o_q), L.ptr(raw), L.ptr(mask), L.ptr(temp), nbytes, L.stream()),
                "bds_pvg_fwd")
        M, flags = (int(x) for x in temp[:8].view(torch.int32).cpu()) if N else (0, 0)      # the one read-back of the call
        info["M"], info["flags"] = M, flags
        outs = tuple(t.narrow(0, 0, M) for t in (o_m, o_o, o_c, o_s, o_q))
        ctx.save_for_backward(v, ta, be, lg, ls, q, cam, mask, temp, o_m, raw)
        ctx.cfg = (cfg, N, M, K, tuple(x.shape for x in (taus, betas, logits)))
        ctx.mark_non_differentiable(mask)
        return outs + (mask,)

    @staticmethod
    def backward(ctx, v_m, v_o, v_c, v_s, v_q, _v_mask):
        v, ta, be, lg, ls, q, cam, mask, temp, o_m, raw = ctx.saved_tensors
        (cur_time, delta_t, in_smooth, T, deg), N, M, K, shapes = ctx.cfg
        dev = v.device
        vin = [torch.zeros(M, w, device=dev) if g is None else g.contiguous().float() for g, w in zip((v_m, v_o, v_c, v_s, v_q), (3, 1, 3, 3, 4))]
        g_m, g_v, g_ls, g_q, g_dc = (torch.empty(N, w, device=dev) for w in (3, 3, 3, 4, 3))
        g_ta, g_be, g_lg = (torch.empty(s, device=dev) for s in shapes)
        g_rest = torch.empty(N, K - 1, 3, device=dev)
        L.check(L.lib().bds_pvg_bwd(N, M, K, deg, cur_time, delta_t, int(in_smooth), T, L.ptr(v), L.ptr(ta), L.ptr(be), L.ptr(lg), L.ptr(ls),
                                    L.ptr(q), L.ptr(cam), L.ptr(mask), L.ptr(temp), temp.numel(), L.ptr(o_m), L.ptr(raw),
                                    *[L.ptr(x) for x in vin], L.ptr(g_m), L.ptr(g_v), L.ptr(g_ta), L.ptr(g_be), L.ptr(g_lg), L.ptr(g_ls),
                                    L.ptr(g_q), L.ptr(g_dc), L.ptr(g_rest) if K > 1 else None, L.stream()), "bds_pvg_bwd")
        return g_m, g_v, g_ta, g_be, g_lg, g_ls, g_q, g_dc, g_rest, None, None, None


def time_transform(means: Tensor, velocity: Tensor, taus: Tensor, betas: Tensor, logits: Tensor, log_scales: Tensor, quats: Tensor,
                   features_dc: Tensor, features_rest: Tensor, cam_pos: Tensor, cur_time: float, delta_t: float, in_smooth: bool, T: float,
                   degrees_to_use: int, info: Optional[dict] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(means [M,3], opacities [M,1], rgbs [M,3], scales [M,3], quats [M,4], filter_mask [N] bool) of the raw parameters means [N,3],
    velocity [N,3], taus / betas / logits [N,1], log_scales [N,3], quats [N,4], features_dc [N,3], features_rest [N,K-1,3]
    (K in {1, 4, 9, 16}; K = 1: sigmoid colours) seen from ``cam_pos`` [3] at ``cur_time``; ``in_smooth``: the smoothing term with
    ``delta_t``; ``T``: the cycle length.  Row r of the outputs is the r-th row with ``filter_mask`` set.  ``info`` (a dict) receives
    ``M`` and ``flags`` (bit 2 i: NaN, bit 2 i + 1: Inf among the kept rows of output i) from the call's one read-back."""
    cfg = (float(cur_time), float(delta_t), bool(in_smooth), float(T), int(degrees_to_use))
    return _TimeTransform.apply(means, velocity, taus, betas, logits, log_scales, quats, features_dc, features_rest, cam_pos, cfg,
                                {} if info is None else info)


# ---- get_gaussians of the reference's PeriodicVibrationGaussians ---------------------------------------------------------------------
def _set_time(self) -> None:
    """Side state of a call (contract of pvg.py:376-387): ``cur_time`` is the frame's time on the training time axis; a training
    call smooths with probability ``smooth_probability`` (one ``random.random()``, drawn only when smoothing is enabled) and then
    shifts ``cur_time`` by one ``Uniform`` sample of up to ``distribution_span`` frame intervals, ``delta_t`` being the way back to
    the frame's time.  Evaluation never smooths and draws nothing.  The values keep the reference's types and float32 arithmetic."""
    cfg = self.ctrl_cfg
    frame_time = self.normalized_timestamps[self.cur_frame] * self.train_time_scale
    smooth = bool(self.training) and bool(cfg.enable_temporal_smoothing) and random.random() < cfg.smooth_probability
    if smooth:
        span = self.normalized_time_interval * cfg.distribution_span * self.train_time_scale
        shifted = frame_time + torch.distributions.Uniform(-span, span).sample((1,)).item()
    self.in_smooth = smooth
    self.cur_time = shifted if smooth else frame_time
    self.delta_t = frame_time - shifted if smooth else 0.0


def _host_scalars(cur_time, delta_t) -> Tuple[float, float]:
    """The two time scalars as Python floats: where the timestamps live on the device they are 0-d device tensors, read in ONE copy."""
    if isinstance(cur_time, Tensor) and isinstance(delta_t, Tensor):
        c, d = torch.stack((cur_time, delta_t.to(cur_time.dtype))).tolist()
        return c, d
    return float(cur_time), float(delta_t)


def pvg_get_gaussians(self, cam) -> dict:
    """``PeriodicVibrationGaussians.get_gaussians`` (pvg.py:374-425) on the fused transform."""
    if not self._means.is_cuda:
        return type(self)._bds_reference_get_gaussians(self, cam)
    _set_time(self)
    n = min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree) if self.sh_degree > 0 else 0
    cur_time, delta_t = _host_scalars(self.cur_time, self.delta_t)
    info = {}
    means, opacities, rgbs, scales, quats, mask = time_transform(
        self._means, self._velocity, self._taus, self._betas, self._opacities, self._scales, self._quats, self._features_dc,
        self._features_rest, cam.camtoworlds.data[..., :3, 3], cur_time, delta_t, self.in_smooth, float(self.T), n, info=info)
    self.filter_mask = mask
    gs = dict(_means=means, _opacities=opacities, _rgbs=rgbs, _scales=scales, _quats=quats)
    for i, k in enumerate(GS_KEYS):      # the reference's scan of the filtered tensors: first key in dict order, NaN before Inf
        if info["flags"] >> (2 * i) & 1:
            raise ValueError(f"NaN detected in gaussian {k} at step {self.step}")
        if info["flags"] >> (2 * i + 1) & 1:
            raise ValueError(f"Inf detected in gaussian {k} at step {self.step}")
    return gs


_SEAM = Seam()


def install(cls) -> None:
    """``install(models.gaussians.pvg.PeriodicVibrationGaussians)``: the class's ``get_gaussians`` becomes the fused one.  The original
    stays reachable as ``cls._bds_reference_get_gaussians``; ``uninstall`` puts it back."""
    _SEAM.install(cls, {"get_gaussians": pvg_get_gaussians}, reference="_bds_reference_get_gaussians")


def uninstall(*classes) -> None:
    _SEAM.uninstall(*classes)
