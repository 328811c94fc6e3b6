"""Deformation network of deformable Gaussians as one fused HIP op each way (csrc/deform.hip through ``bds_deform_fwd / _bwd``).

Reference: ``ConditionalDeformNetwork`` (DeformableNodes, every OmniRe config) and ``DeformNetwork`` (configs/deformablegs.yaml) in
the reference's models/modules.py:925-1012, with the encoding ``get_embedder`` / ``Embedder`` (:874-922).  The kernels are
built for the shipped size (``supported``): D 8, W 256, x / t multires 10, input_ch 3, embed_dim 0 or 16, any head flags.

* ``ConditionalDeformNetwork`` / ``DeformNetwork`` here mirror the reference classes: same constructor arguments, same parameter
  names (a reference ``deform_network.*`` state_dict loads with ``strict=True``), same ``(d_xyz, rotation, scaling)`` return.
* ``install(cls)`` swaps ``forward`` on the reference's own class for the fused one (the module keeps its parameters, so optimizer
  groups and checkpoints are untouched); ``uninstall(cls)`` puts the original back.
* Outside the supported set the mirrors run the same expression as framework ops (with a warning) and the hook keeps the class's
  own forward."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib as L
from ._patch import Seam

D_LAYERS, WIDTH, MULTIRES, INPUT_CH = 8, 256, 10, 3
EMBED_DIMS = (0, 16)
X_EMB, T_EMB = 3 * (1 + 2 * MULTIRES), 1 * (1 + 2 * MULTIRES)


def supported(D: int, W: int, x_multires: int, t_multires: int, embed_dim: int, input_ch: int = INPUT_CH) -> bool:
    """The sizes the kernels are built for: the shipped D 8, W 256, multires 10 / 10, input_ch 3, embed_dim in {0, 16}."""
    return (D == D_LAYERS and W == WIDTH and x_multires == MULTIRES and t_multires == MULTIRES and input_ch == INPUT_CH
            and embed_dim in EMBED_DIMS)


def embed(v: Tensor, multires: int) -> Tensor:
    """``Embedder.embed`` (modules.py:874-922): [v, sin(2^0 v), cos(2^0 v), ..., sin(2^(L-1) v), cos(2^(L-1) v)]."""
    freqs = 2.0 ** torch.linspace(0.0, multires - 1, multires)
    out = [v]
    for f in freqs.tolist():
        out += [torch.sin(v * f), torch.cos(v * f)]
    return torch.cat(out, -1)


def framework_forward(linear, heads, x: Tensor, t: Tensor, condition: Optional[Tensor], x_multires: int, t_multires: int):
    """The network as framework ops (modules.py:956-964 / 995-1012): the path outside the supported set, and the A side of
    scripts/deform_time.py.  ``heads`` = (warp, rotation or None, scaling or None) modules."""
    x_emb, t_emb = embed(x, x_multires), embed(t, t_multires)
    h0 = torch.cat([x_emb, t_emb] + ([condition] if condition is not None else []), -1)
    h = h0
    skip = len(linear) // 2
    for i, lin in enumerate(linear):
        h = F.relu(lin(h))
        if i == skip:
            h = torch.cat([h0, h], -1)
    return tuple(None if m is None else m(h) for m in heads)


def _net_struct(ws: List[Optional[Tensor]]):
    """16 layer tensors (w0, b0, ..., w7, b7) + warp w/b, rotation w/b, scaling w/b (None = off) -> bds_deform_net."""
    s = L.BdsDeformNet()
    for i in range(D_LAYERS):
        s.w[i] = None if ws[2 * i] is None else ws[2 * i].data_ptr()
        s.b[i] = None if ws[2 * i + 1] is None else ws[2 * i + 1].data_ptr()
    names = ("warp_w", "warp_b", "rot_w", "rot_b", "scale_w", "scale_b")
    for k, n in enumerate(names):
        setattr(s, n, None if ws[16 + k] is None else ws[16 + k].data_ptr())
    return s


class _Deform(torch.autograd.Function):
    """x [N,3], t [N,1], cond [N,E] or None, then the 22 parameter tensors (heads that are off: None) -> d_xyz, rotation, scaling."""

    @staticmethod
    def forward(ctx, x: Tensor, t: Tensor, cond: Optional[Tensor], *params: Optional[Tensor]):
        L.require_gpu(x, t, *[p for p in params if p is not None])
        N = x.shape[0]
        E = 0 if cond is None else cond.shape[1]
        assert E in EMBED_DIMS and x.shape == (N, 3) and t.shape[0] == N and t.numel() == N
        xc, tc = x.detach().contiguous().float(), t.detach().reshape(N).contiguous().float()
        cc = None if cond is None else cond.detach().contiguous().float()
        ws = [None if p is None else p.detach().contiguous().float() for p in params]
        dev = x.device
        d_xyz = torch.empty(N, 3, device=dev)
        rot = torch.empty(N, 4, device=dev) if ws[18] is not None else None
        scale = torch.empty(N, 3, device=dev) if ws[20] is not None else None
        net = _net_struct(ws)
        L.check(L.lib().bds_deform_fwd(N, E, L.ptr(xc), L.ptr(tc), L.ptr(cc), C.byref(net), L.ptr(d_xyz), L.ptr(rot), L.ptr(scale),
                                       L.stream()), "bds_deform_fwd")
        ctx.save_for_backward(xc, tc, cc if cc is not None else xc.new_empty(0), *[w if w is not None else xc.new_empty(0) for w in ws])
        ctx.cfg = (E, [w is not None for w in ws], t.shape)
        return d_xyz, rot, scale

    @staticmethod
    def backward(ctx, v_xyz, v_rot, v_scale):
        xc, tc, cc, *ws = ctx.saved_tensors
        E, present, t_shape = ctx.cfg
        ws = [w if p else None for w, p in zip(ws, present)]
        cc = cc if E else None
        N = xc.shape[0]
        need = ctx.needs_input_grad
        dev = xc.device
        if N == 0:
            return (torch.zeros_like(xc) if need[0] else None, torch.zeros(t_shape, device=dev) if need[1] else None,
                    None if cc is None or not need[2] else torch.zeros_like(cc), *[None if w is None or not need[3 + i] else torch.zeros_like(w)
                                                                                    for i, w in enumerate(ws)])
        gs = [None if v is None else v.contiguous().float() for v in (v_xyz, v_rot, v_scale)]
        if gs[0] is None:
            gs[0] = torch.zeros(N, 3, device=dev)
        v_x = torch.empty(N, 3, device=dev) if need[0] else None
        v_t = torch.empty(N, device=dev) if need[1] else None
        v_c = torch.empty(N, E, device=dev) if (E and need[2]) else None
        v_w = [torch.empty_like(w) if (w is not None and need[3 + i]) else None for i, w in enumerate(ws)]
        nb = int(L.lib().bds_deform_bwd_temp_bytes(N, E))
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        net, grad = _net_struct(ws), _net_struct(v_w)
        L.check(L.lib().bds_deform_bwd(N, E, L.ptr(xc), L.ptr(tc), L.ptr(cc), C.byref(net), L.ptr(gs[0]), L.ptr(gs[1]), L.ptr(gs[2]),
                                       L.ptr(v_x), L.ptr(v_t), L.ptr(v_c), C.byref(grad), 0, L.ptr(temp), nb, L.stream()), "bds_deform_bwd")
        return (v_x, None if v_t is None else v_t.reshape(t_shape), v_c, *v_w)


def _params(linear, warp, rotation, scaling) -> List[Optional[Tensor]]:
    ps: List[Optional[Tensor]] = []
    for lin in linear:
        ps += [lin.weight, lin.bias]
    for m in (warp, rotation, scaling):
        ps += [None, None] if m is None else [m.weight, m.bias]
    return ps


def deform(linear, warp, rotation, scaling, x: Tensor, t: Tensor, condition: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """The fused network: ``linear`` = the 8 ``nn.Linear`` of the reference's ``linear`` list, heads (None = off) ->
    (d_xyz, rotation, scaling) for x [N,3], t [N,1], condition [N,E] or None.  Leading dimensions of x / t / condition are flattened
    and restored."""
    lead = x.shape[:-1]
    N = x[..., 0].numel()
    cond = None if condition is None else condition.reshape(N, condition.shape[-1])
    out = _Deform.apply(x.reshape(N, 3), t.reshape(N, 1), cond, *_params(linear, warp, rotation, scaling))
    return tuple(None if o is None else o.reshape(*lead, o.shape[-1]) for o in out)


_warned = set()


def _warn_fallback(what: str) -> None:
    if what not in _warned:
        _warned.add(what)
        warnings.warn(f"bilateral_driving_amd.deform: {what} is outside the fused kernels' sizes (D 8, W 256, multires 10 / 10, "
                      "input_ch 3, embed_dim 0 or 16): running the network as framework ops", stacklevel=3)


class ConditionalDeformNetwork(nn.Module):
    """Mirror of models/modules.py:967-1012 (DeformableNodes' network)."""

    def __init__(self, D=8, W=256, input_ch=3, embed_dim=10, x_multires=10, t_multires=10, deform_quat=True, deform_scale=True):
        super().__init__()
        self.D, self.W, self.embed_dim = D, W, embed_dim
        self.deform_quat, self.deform_scale = deform_quat, deform_scale
        self.x_multires, self.t_multires = x_multires, t_multires
        self.skips = [D // 2]
        self.fused = supported(D, W, x_multires, t_multires, embed_dim, input_ch)
        self.input_ch = input_ch * (1 + 2 * x_multires) + (1 + 2 * t_multires) + embed_dim
        self.linear = nn.ModuleList([nn.Linear(self.input_ch, W)] + [
            nn.Linear(W, W) if i not in self.skips else nn.Linear(W + self.input_ch, W) for i in range(D - 1)])
        self.gaussian_warp = nn.Linear(W, 3)
        if deform_quat:
            self.gaussian_rotation = nn.Linear(W, 4)
        if deform_scale:
            self.gaussian_scaling = nn.Linear(W, 3)

    def _heads(self):
        return (self.gaussian_warp, self.gaussian_rotation if self.deform_quat else None,
                self.gaussian_scaling if self.deform_scale else None)

    def forward(self, x, t, condition):
        if self.fused:
            return deform(self.linear, *self._heads(), x, t, condition)
        _warn_fallback(f"ConditionalDeformNetwork(D={self.D}, W={self.W}, embed_dim={self.embed_dim})")
        return framework_forward(self.linear, self._heads(), x, t, condition, self.x_multires, self.t_multires)


class DeformNetwork(nn.Module):
    """Mirror of models/modules.py:925-964 (DeformableGaussians' network: no condition, all three heads)."""

    def __init__(self, D=8, W=256, input_ch=3, output_ch=59, x_multires=10, t_multires=10):
        super().__init__()
        self.D, self.W, self.output_ch = D, W, output_ch
        self.x_multires, self.t_multires = x_multires, t_multires
        self.skips = [D // 2]
        self.fused = supported(D, W, x_multires, t_multires, 0, input_ch)
        self.input_ch = input_ch * (1 + 2 * x_multires) + (1 + 2 * t_multires)
        self.linear = nn.ModuleList([nn.Linear(self.input_ch, W)] + [
            nn.Linear(W, W) if i not in self.skips else nn.Linear(W + self.input_ch, W) for i in range(D - 1)])
        self.gaussian_warp = nn.Linear(W, 3)
        self.gaussian_rotation = nn.Linear(W, 4)
        self.gaussian_scaling = nn.Linear(W, 3)

    def forward(self, x, t):
        heads = (self.gaussian_warp, self.gaussian_rotation, self.gaussian_scaling)
        if self.fused:
            return deform(self.linear, *heads, x, t)
        _warn_fallback(f"DeformNetwork(D={self.D}, W={self.W})")
        return framework_forward(self.linear, heads, x, t, None, self.x_multires, self.t_multires)


# ---- the hook on the reference's own classes ----------------------------------------------------------------------------------------
def _module_config(m) -> Optional[Tuple[int, Tuple]]:
    """(embed_dim, heads) when a reference-layout module has the fused sizes, else None.  The reference keeps neither the multires
    nor the raw input_ch, so they are read from the module's own embedders and layer shapes."""
    cached = m.__dict__.get("_bds_deform_cfg")
    if cached is not None:
        return cached[0]
    cfg = None
    try:
        E = int(getattr(m, "embed_dim", 0)) if hasattr(m, "deform_quat") else 0
        lin = m.linear
        with torch.no_grad():
            xe = m.embed_fn(torch.zeros(1, 3)).shape[-1]
            te = m.embed_time_fn(torch.zeros(1, 1)).shape[-1]
        ok = (len(lin) == D_LAYERS and m.W == WIDTH and xe == X_EMB and te == T_EMB and E in EMBED_DIMS
              and lin[0].in_features == X_EMB + T_EMB + E and lin[D_LAYERS // 2 + 1].in_features == WIDTH + X_EMB + T_EMB + E
              and list(m.skips) == [D_LAYERS // 2])
        if ok:
            if hasattr(m, "deform_quat"):
                heads = (m.gaussian_warp, m.gaussian_rotation if m.deform_quat else None, m.gaussian_scaling if m.deform_scale else None)
            else:
                heads = (m.gaussian_warp, m.gaussian_rotation, m.gaussian_scaling)
            cfg = (E, heads)
    except (AttributeError, TypeError):
        cfg = None
    m.__dict__["_bds_deform_cfg"] = (cfg,)
    return cfg


def _fused_forward(self, x, t, condition=None):
    cfg = _module_config(self)
    if cfg is None or not x.is_cuda:
        return type(self)._bds_reference_forward(self, x, t, *(() if condition is None else (condition,)))
    E, heads = cfg
    if E == 0:
        condition = None
    return deform(self.linear, *heads, x, t, condition)


_SEAM = Seam()


def install(network_class) -> None:
    """``install(models.modules.ConditionalDeformNetwork)`` (or ``DeformNetwork``): the class's ``forward`` becomes the fused one for
    modules with the supported sizes (others keep the original).  The original stays reachable as
    ``network_class._bds_reference_forward``; ``uninstall`` puts it back."""
    _SEAM.install(network_class, {"forward": _fused_forward}, reference="_bds_reference_forward")


def uninstall(*network_classes) -> None:
    _SEAM.uninstall(*network_classes)
