"""``rasterization`` with the signature the reference imports from gsplat v1.3.0
(/root/reference/project/models/gaussians/basics.py:12; called at
/root/reference/project/models/trainers/base.py:393-408 and :811-826).

Pipeline (every stage a hand-written gfx950 kernel behind libbds.so):
    projection -> tile intersection + ordering -> alpha compositing -> expected-depth normalise
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

import weakref

from . import _lib as L
from .lazy_gaussians import lazy_scene, lazy_source, materialised


_SPLIT_RENDER = os.environ.get("BDS_API_SPLIT_RENDER", "1") == "1"


class SplitRender(torch.Tensor):
    """``render_colors`` [..., H, W, 4] of the raw one-view node as a placeholder over its TWO outputs, rgb [..., H, W, 3] and depth
    [..., H, W, 1].  The reference's trainer takes ``renders[0]`` and splits it at once (``torch.split(renders, [3, 1], dim=-1)``,
    /root/reference/project/models/trainers/base.py:409-419); through a 4-channel tensor that costs a select backward, a slice backward
    (an image of zeros + a copy each) and a contiguous copy of the colours for the transform -- 0.13 ms of GPU and 0.15 ms of host time
    per 1080p view.  The placeholder answers exactly those uses with the node's own outputs (leading integer index, ``split([3, 1],
    -1)``, ``[..., :3]``, ``[..., 3:4]``, metadata); ANYTHING else first materialises ``torch.cat((rgb, depth), -1)`` -- an ordinary
    tensor with the same values and the same gradients (the mechanism of ``lazy_gaussians.LazyField``)."""

    @staticmethod
    def __new__(cls, rgb: Tensor, depth: Tensor, first=None):
        """``first``: (rgb[0], depth[0]) when the caller already holds them as tensors of their own (the node's outputs are [H,W,3] /
        [H,W,1]; the [1,H,W,.] form is an unsqueeze of them, whose backward is a view -- a select's is an image of zeros + a copy)."""
        assert rgb.shape[:-1] == depth.shape[:-1] and rgb.shape[-1] == 3 and depth.shape[-1] == 1
        r = torch.Tensor._make_wrapper_subclass(cls, tuple(rgb.shape[:-1]) + (4,), dtype=rgb.dtype, device=rgb.device,
                                                requires_grad=rgb.requires_grad or depth.requires_grad)
        r._rgb, r._depth, r._cat, r._first = rgb, depth, None, first
        return r

    def materialise(self) -> Tensor:
        if self._cat is None:
            self._cat = torch.cat((self._rgb, self._depth), dim=-1)
        return self._cat

    def __repr__(self):
        return f"SplitRender(rgb={tuple(self._rgb.shape)}, depth={tuple(self._depth.shape)})"

    @staticmethod
    def _channel_slice(idx):
        """'rgb' / 'depth' for an index that selects channels 0:3 / 3:4 of the last dimension and everything else, else None."""
        if not (isinstance(idx, tuple) and len(idx) == 2 and idx[0] is Ellipsis and isinstance(idx[1], slice)):
            return None
        sl = idx[1]
        if sl.step not in (None, 1):
            return None
        lo, hi = sl.start or 0, 4 if sl.stop is None else sl.stop
        return "rgb" if (lo, hi) == (0, 3) else ("depth" if (lo, hi) == (3, 4) else None)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        from .lazy_gaussians import _meta_funcs
        kwargs = kwargs or {}
        if func in _meta_funcs():
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)
        me = args[0] if args and isinstance(args[0], SplitRender) else None
        if me is not None and func is torch.Tensor.__getitem__ and len(args) == 2:
            idx = args[1]
            if isinstance(idx, int) and me.dim() > 3:                       # renders[0]
                if me._first is not None and idx in (0, -me.shape[0]) and me.shape[0] == 1:
                    return SplitRender(*me._first)
                return SplitRender(me._rgb[idx], me._depth[idx])
            which = cls._channel_slice(idx)
            if which is not None:
                return me._rgb if which == "rgb" else me._depth
            if isinstance(idx, tuple) and len(idx) >= 2 and isinstance(idx[0], int) and me.dim() > 3:   # renders[0, ..., :3]
                return me[idx[0]][idx[1:] if len(idx) > 2 else idx[1]]
        if me is not None and func in (torch.split, torch.Tensor.split):
            sizes = args[1] if len(args) > 1 else kwargs.get("split_size_or_sections", kwargs.get("split_size"))
            dim = args[2] if len(args) > 2 else kwargs.get("dim", 0)
            if list(sizes) == [3, 1] if isinstance(sizes, (list, tuple)) else False:
                if dim in (-1, me.dim() - 1):
                    return me._rgb, me._depth
        return func(*_split_materialised(args), **_split_materialised(kwargs))

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        return func(*_split_materialised(args), **_split_materialised(kwargs or {}))


def _split_materialised(x):
    if isinstance(x, SplitRender):
        return x.materialise()
    if isinstance(x, (list, tuple)):
        return type(x)(_split_materialised(v) for v in x)
    if isinstance(x, dict):
        return {k: _split_materialised(v) for k, v in x.items()}
    return x
from .fused_view import (_Front, _composite, _composite_backward, _image_buffers, _lists_begin, _lists_finish, _project_backward,
                         _view_front)
from .gs_ops import (TILE_SIZE, fully_fused_projection, isect_tiles, rasterize_to_pixels, spherical_harmonics)


class _Meta(dict):
    """The ``meta`` dict of gsplat's rasterization().  ``isect_ids`` (the sorted 64-bit keys, which nothing on
    the reference's path reads) is materialised on first access instead of on every step -- and, on the one-view fast path
    (``_RasterizeView``), so are gsplat's per-16-px-tile lists (``tiles_per_gauss`` / ``flatten_ids`` / ``isect_offsets``): the
    compositor there walks compact lists of 64-px tiles that never take gsplat's layout (the reference reads ``means2d`` / ``radii`` /
    ``width`` / ``height``: models/trainers/base.py:279-297,422-430)."""
    _LISTS = ("tiles_per_gauss", "flatten_ids", "isect_offsets")

    # (every reading accessor goes through __getitem__: meta.get(..), .items(), .values(), dict(meta) and ** unpacking see the lists too)
    def get(self, key, default=None):
        return self[key] if key in self else default

    def __iter__(self):      # (overridden on purpose: CPython's dict(meta) / ** take a raw-copy fast path for dict subclasses that keep dict's iterator)
        return iter(list(dict.keys(self)))

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def __getitem__(self, key):
        if key in self._LISTS and dict.__getitem__(self, key) is None:
            cull = dict.__getitem__(self, "_cull")
            tpg, _, fids, offs = isect_tiles(self["means2d"], self["radii"], self["depths"], self["tile_size"], self["tile_width"],
                                             self["tile_height"], want_isect_ids=False, conics=self["conics"] if cull else None,
                                             opacities=self["opacities"].contiguous() if cull else None)
            dict.__setitem__(self, "tiles_per_gauss", tpg)
            dict.__setitem__(self, "flatten_ids", fids)
            dict.__setitem__(self, "isect_offsets", offs)
        if key == "isect_ids" and dict.__getitem__(self, key) is None:
            self["isect_ids"] = _isect_ids_from(self["isect_offsets"], self["flatten_ids"], self["depths"])
        return dict.__getitem__(self, key)


@torch.no_grad()
def _isect_ids_from(isect_offsets: Tensor, flatten_ids: Tensor, depths: Tensor) -> Tensor:
    M = flatten_ids.numel()
    idx = torch.arange(M, device=flatten_ids.device)
    tile = torch.bucketize(idx, isect_offsets.reshape(-1).long(), right=True) - 1  # camera*tiles + tile
    bits = depths.detach().reshape(-1)[flatten_ids.long()].contiguous().view(torch.int32).long()
    return (tile << 32) | bits


# Exact tile culling (see gs_ops.isect_tiles): on by default -- images and gradients are identical, only the
# intersection lists in ``meta`` (tiles_per_gauss / flatten_ids / isect_ids / isect_offsets) are shorter than
# gsplat's bounding-square lists.  Switch off to reproduce gsplat's lists entry for entry.
_TILE_CULLING = os.environ.get("BDS_TILE_CULL", "1") != "0"


def set_tile_culling(on: bool) -> None:
    global _TILE_CULLING
    _TILE_CULLING = bool(on)


# One camera, post-activation colours [N,3], "RGB" / "RGB+ED", either rasterize_mode, no backgrounds -- the reference's two call patterns
# (models/trainers/base.py:393-408,811-826) -- run as ONE autograd node over compact lists (BDS_API_FUSED=0: the operator chain below)
_ONE_VIEW_NODE = os.environ.get("BDS_API_FUSED", "1") != "0"
_CHECK_FINITE = os.environ.get("BDS_API_CHECK_FINITE", "1") != "0"    # the raw one-view node's NaN / Inf check (vanilla.py:407-412)
_LIST_TILE = 64          # list tiles of the one-view node (the splat records carry the radii: the image is the 16-px one)


class _RasterizeView(torch.autograd.Function):
    """gsplat's rasterization() for one camera as one node: general projection (activated scales), visibility compaction + depth
    order + 64-px tile lists in compact positions (ONE host wait for the two list counts, overlapped with packing the colours),
    48-byte splat records of the visible Gaussians only, forward composite; backward: composite -> 64-byte gradient records of the
    visible Gaussians -> list-driven projection backward into dense, zero-initialised gradients (rows of culled Gaussians stay
    zero, as gsplat returns them).  Against the operator chain: no dense record pack / dense gradient records over all N, no dense
    projection backward, ~12 launches instead of ~45."""

    @staticmethod
    def forward(ctx, means, quats, scales, opacities, colors, viewmat, Kmat, cfg):
        L.require_gpu(means, quats, scales, opacities, colors, viewmat, Kmat)
        means, quats, scales, opacities, colors, viewmat, Kmat = map(L.f32c, (means, quats, scales, opacities, colors, viewmat, Kmat))
        lib, st = L.lib(), L.stream()
        dev = means.device
        W, H, N = cfg["width"], cfg["height"], means.shape[0]
        radii = torch.empty(1, N, device=dev, dtype=torch.int32)
        means2d, depths, conics = torch.empty(1, N, 2, device=dev), torch.empty(1, N, device=dev), torch.empty(1, N, 3, device=dev)
        opac_eff = torch.empty(1, N, device=dev) if cfg["aa"] else None      # antialiased: opacity * comp, what tiles and compositor read
        with L.timed("project_fwd"):
            L.check(lib.bds_project_fwd(1, N, L.ptr(means), L.ptr(quats), L.ptr(scales), None if opac_eff is None else L.ptr(opacities),
                                        L.ptr(viewmat), L.ptr(Kmat), W, H, cfg["eps2d"], cfg["near_plane"], cfg["far_plane"], cfg["radius_clip"],
                                        L.ptr(radii), L.ptr(means2d), L.ptr(depths), L.ptr(conics), None, L.ptr(opac_eff), st), "bds_project_fwd")
        opac_c = opacities.view(1, N) if opac_eff is None else opac_eff
        s = _lists_begin(means2d, radii, depths, (L.ptr(conics), L.ptr(opac_c)) if cfg["cull"] else None, W, H, _LIST_TILE)
        images = _image_buffers(W, H, dev)     # (while the two counts travel to the host)
        _lists_finish(s)
        f = _Front()         # the lists + what else _composite reads
        f.flatten, f.vis_ids, f.M, f.n_vis, f.m_dev, f.nvis_dev, f.rec_buf = s.flatten, s.vis_ids, s.M, s.n_vis, s.m_dev, s.nvis_dev, s.rec_buf
        f.cfg, f.W, f.H, f.list_tile, f.tw, f.th = cfg, W, H, _LIST_TILE, math.ceil(W / TILE_SIZE), math.ceil(H / TILE_SIZE)
        f.means2d, f.depths, f.conics, f.radii, f.isect_offsets = means2d, depths, conics, radii, s.isect_offsets
        f.opac = f.opac_row = opac_c
        f.colors = colors.reshape(N, 3)      # post-activation: the pack adds the depths (bds_splat_pack_rgbd)
        rec, render, alphas, last_ids = _composite(f, f.opac, images)
        ctx.save_for_backward(means, quats, scales, opacities, viewmat, Kmat, rec, f.vis_ids, s.ws, f.flatten, f.isect_offsets, render, alphas,
                              last_ids)
        ctx.cfg, ctx.M = cfg, f.M
        if cfg["ed"]:      # expected depth: D / clamp(alpha, 1e-10) (gsplat "ED")
            out = torch.empty_like(render)
            L.check(lib.bds_expected_depth_fwd(H * W, L.ptr(render), L.ptr(alphas), L.ptr(out), st), "bds_expected_depth_fwd")
        else:
            out = render[..., :3] if cfg["channels"] == 3 else render
        ctx.mark_non_differentiable(radii, depths, conics)
        if opac_eff is not None:
            ctx.mark_non_differentiable(opac_eff)
        # undefined output gradients stay None: the reference never puts a loss on meta["means2d"], and a materialised [1,N,2] zero
        # tensor would cost a fill, an index_select and an add over the records in every backward
        ctx.set_materialize_grads(False)
        return out, alphas, means2d, radii, depths, conics, opac_eff

    @staticmethod
    def backward(ctx, v_out, v_alphas, v_means2d_ext, *_):
        cfg, want_pose = ctx.cfg, bool(ctx.needs_input_grad[5])
        # dense outputs: means 3 | quats 4 | scales 3 | opacities 1 | colours 3 | grad2d 2 | absgrad2d 2
        outs, _, slots = _view_backward(ctx, ctx.saved_tensors, v_out, None, v_alphas, v_means2d_ext, want_pose, (3, 4, 3, 1, 3, 2, 2),
                                        L.PROJ_ACTIVATED)
        v_means, v_quats, v_scales, v_opac, v_colors = outs[:5]
        g = ctx.needs_input_grad
        return (v_means if g[0] else None, v_quats if g[1] else None, v_scales if g[2] else None, v_opac if g[3] else None,
                v_colors.view(cfg["colors_shape"]) if g[4] else None, slots.sum(0) if want_pose else None, None, None)


class _RasterizeRawView(torch.autograd.Function):
    """rasterization() for one camera over a class's RAW parameters (``lazy_gaussians``: the reference's unmodified call sequence
    with ``marshalling.install``): what ``_RasterizeView`` does, with sigmoid / exp / quaternion normalisation inside the projection
    kernel (bds_project_view_fwd), the SH colours (+0.5, clamp) evaluated by the record pack for the VISIBLE Gaussians only, straight
    from the class's two SH parameters (bds_splat_pack_sh with coeffs_rest: no concatenation, no dense SH pass over all N), and the backward
    list-driven into the raw parameters' gradients (bds_sh_view_bwd_list with v_coeffs_rest, bds_project_view_bwd_list).  The reference's NaN /
    Inf check (vanilla.py:407-412) is one streaming launch whose flag word arrives with the list counts."""

    @staticmethod
    def forward(ctx, means, quats, log_scales, logits, dc, rest, viewmat, Kmat, cfg):
        L.require_gpu(means, quats, log_scales, logits, dc, rest, viewmat, Kmat)
        means, quats, log_scales, logits, dc, rest, viewmat, Kmat = map(L.f32c, (means, quats, log_scales, logits, dc, rest, viewmat, Kmat))
        lib, st = L.lib(), L.stream()
        dev = means.device
        W, H, N = cfg["width"], cfg["height"], means.shape[0]
        fcfg = dict(width=W, height=H, K=Kmat, cam_pos=cfg["cam_pos"], sh_degree=cfg["sh_degree"], near_plane=cfg["near_plane"],
                    far_plane=cfg["far_plane"], radius_clip=cfg["radius_clip"], eps2d=cfg["eps2d"], tile_cull=cfg["cull"],
                    list_tile=_LIST_TILE, antialiased=cfg["aa"])
        flags = None
        if cfg["check_finite"]:
            # in FRONT of the projection: the flag's copy to the host is then older than the event the one wait of this view waits for.
            # On the raw values, by what makes each tensor's ACTIVATION non-finite (the reference checks the activated tensors,
            # vanilla.py:393-395,407-412): a log-scale whose exp overflows (NaN, +Inf, >= 88.72284; -Inf gives 0), a quaternion with a
            # NaN / Inf component or all zeros (0 / 0), a NaN logit (sigmoid maps +-Inf to 0 / 1); means and SH coefficients as they are
            flags = _finite_words(dev)
            ts = (means, quats, log_scales, logits, dc, rest)
            ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            cnts = (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts])
            kinds = (ctypes.c_int * len(ts))(0, 2, 1, 3, 0, 0)
            L.check(lib.bds_nonfinite_flags(len(ts), ptrs, cnts, kinds, flags[0].data_ptr(), flags[1].data_ptr(), st), "bds_nonfinite_flags")
        f = _view_front(fcfg, means, quats, log_scales, logits.reshape(N), (dc, rest), viewmat, lambda: _image_buffers(W, H, dev))
        if flags is not None and int(flags[1][0]):
            bad = [n for i, n in enumerate(("means", "quats", "scales", "opacities", "features_dc", "features_rest")) if int(flags[1][0]) >> i & 1]
            raise ValueError(f"NaN / Inf detected in gaussian {', '.join(bad)} at step {cfg['step']}")
        rec, render, alphas, last_ids = _composite(f, f.opac, f.pre)
        ctx.save_for_backward(f.means, f.quats, f.scales, f.opac, viewmat, Kmat, rec, f.vis_ids, f.ws, f.flatten, f.isect_offsets, render, alphas,
                              last_ids, f.sh_rgb, f.cam_pos)
        ctx.cfg, ctx.M, ctx.shapes = cfg, f.M, (tuple(log_scales.shape), tuple(cfg["logits_shape"]), tuple(dc.shape), tuple(rest.shape))
        opac_out = f.opac_row if cfg["aa"] else f.opac      # (meta["opacities"]: what the compositor used -- antialiased: opacity * comp)
        ctx.mark_non_differentiable(f.radii, f.depths, f.conics, opac_out)
        ctx.set_materialize_grads(False)
        if cfg.get("split"):       # rgb and depth as two outputs (SplitRender): 4-channel modes only
            rgb, depth = torch.empty(H, W, 3, device=dev), torch.empty(H, W, 1, device=dev)
            L.check(lib.bds_expected_depth_split_fwd(H * W, int(cfg["ed"]), L.ptr(render), L.ptr(alphas), L.ptr(rgb), L.ptr(depth), st),
                    "bds_expected_depth_split_fwd")
            return rgb, depth, alphas, f.means2d, f.radii, f.depths, f.conics, opac_out
        if cfg["ed"]:
            out = torch.empty_like(render)
            L.check(lib.bds_expected_depth_fwd(H * W, L.ptr(render), L.ptr(alphas), L.ptr(out), st), "bds_expected_depth_fwd")
        else:
            out = render[..., :3] if cfg["channels"] == 3 else render
        return out, None, alphas, f.means2d, f.radii, f.depths, f.conics, opac_out

    @staticmethod
    def backward(ctx, v_out, v_depth, v_alphas, v_means2d_ext, *_):
        saved = ctx.saved_tensors
        means, vis_ids, sh_rgb, cam_pos = saved[0], saved[7], saved[14], saved[15]
        cfg, want_pose = ctx.cfg, bool(ctx.needs_input_grad[6])
        ls_shape, lg_shape, dc_shape, rest_shape = ctx.shapes
        K = 1 + rest_shape[1]
        widths = (3, 4, 3, 1, 3, 3 * (K - 1), 2, 2)   # means | quats | log_scales | logits | dc | rest | grad2d | absgrad2d
        outs, v_rec, slots = _view_backward(ctx, saved, v_out, v_depth, v_alphas, v_means2d_ext, want_pose, widths, 0)
        v_means, v_quats, v_ls, v_logits, v_dc, v_rest = outs[:6]
        with L.timed("sh_bwd"):
            L.check(L.lib().bds_sh_view_bwd_list(vis_ids.numel(), None, L.ptr(vis_ids), K, cfg["sh_degree"], L.ptr(means), L.ptr(cam_pos),
                                                 L.ptr(sh_rgb), 1, L.ptr(v_rec), L.ptr(v_dc), L.ptr(v_rest), None, 0, L.stream()),
                    "bds_sh_view_bwd_list")
        g = ctx.needs_input_grad
        return (v_means if g[0] else None, v_quats if g[1] else None, v_ls.view(ls_shape) if g[2] else None,
                v_logits.view(lg_shape) if g[3] else None, v_dc.view(dc_shape) if g[4] else None, v_rest.view(rest_shape) if g[5] else None,
                slots.sum(0) if want_pose else None, None, None)


class _SceneTable:
    """The segment table of include/bds.h "the scene view" as the host arrays its two entries take: rows, kinds, K and active degree
    per segment, and the forward's pointer pair (raw: ``_features_dc`` / ``_features_rest``; dense: the activated colours)."""

    def __init__(self, segs, colors, rests):
        n = self.n = len(segs)
        self.rows = (ctypes.c_int64 * n)(*[s["n"] for s in segs])
        self.kinds = (ctypes.c_int * n)(*[int(s["raw"]) for s in segs])      # BDS_SCENE_DENSE 0 / BDS_SCENE_RAW 1
        self.Ks = (ctypes.c_int * n)(*[s["K"] for s in segs])
        self.degs = (ctypes.c_int * n)(*[s["deg"] for s in segs])
        self._keep = (colors, rests)
        self.p0, self.p1 = self.pointers(colors, rests)

    def pointers(self, a, b):
        n = self.n
        return ((ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in a]),
                (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in b]))

    def head(self):
        return self.n, self.rows, self.kinds, self.Ks, self.degs

    def forward_args(self):
        return (*self.head(), self.p0, self.p1)


_RAW_FIELDS = ("means", "quats", "scales", "opacities", "features_dc", "features_rest")


class _RasterizeSceneView(torch.autograd.Function):
    """rasterization() for one camera over SEVERAL Gaussian classes (``lazy_gaussians.lazy_scene``: the reference's scene graph,
    models/trainers/base.py:355-366, with ``marshalling.install(cls, scene=True)``): the classes' rows lie one behind the other in one
    row range [0, N).  A RAW segment hands over a class's six raw parameters -- activations inside its own projection launch
    (bds_project_view_fwd into rows [start, start + n) of the [N] arrays), SH colours by the record pack for its VISIBLE rows only,
    straight from its two SH parameters at its own degree (bds_scene_pack) -- a DENSE segment a class's five activated tensors, taken
    as they are (bds_project_fwd into its rows).  The tile stage and the compositors are ``_RasterizeView``'s, on global row ids.
    Backward: the list-driven projection backward in its ACTIVATED form over all rows, then bds_scene_sh_bwd: SH backward into each raw
    segment's own gradient arrays and the exp / sigmoid chain of the raw rows.  Every segment's gradients are slices of the dense
    arrays.  Only the means and quaternions are concatenated (28 bytes per row: the list-driven kernels gather them by global id);
    no SH coefficient is concatenated, evaluated for or written back to a culled row.  NaN / Inf: one bds_nonfinite_flags launch
    per raw segment in front of the projection, read with the one wait of the view (dense segments arrive checked by their class).
    ``tensors``: per segment in order, raw (means, quats, log_scales, logits, features_dc, features_rest), dense (means, quats,
    scales, opacities, colors)."""

    @staticmethod
    def forward(ctx, viewmat, Kmat, cfg, *tensors):
        L.require_gpu(viewmat, Kmat, *tensors)
        viewmat, Kmat = L.f32c(viewmat), L.f32c(Kmat)
        lib, st = L.lib(), L.stream()
        dev = viewmat.device
        W, H, N, aa, segs = cfg["width"], cfg["height"], cfg["N"], cfg["aa"], cfg["segments"]
        per, i = [], 0
        for s in segs:
            k = 6 if s["raw"] else 5
            per.append([L.f32c(t) for t in tensors[i:i + k]])
            i += k
        means, quats = torch.cat([p[0] for p in per], 0), torch.cat([p[1] for p in per], 0)      # [N,3], [N,4]: global rows
        scales, opac = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
        opac_eff = torch.empty(N, device=dev) if aa else None
        radii = torch.empty(1, N, device=dev, dtype=torch.int32)
        means2d, depths, conics = torch.empty(1, N, 2, device=dev), torch.empty(1, N, device=dev), torch.empty(1, N, 3, device=dev)
        checked = []
        if cfg["check_finite"]:      # in front of the projection, by the kinds of _RasterizeRawView; one flag word per raw segment
            words = _finite_words(dev, 8)
            for s, p in zip(segs, per):
                if not (s["raw"] and s["n"] > 0):
                    continue
                slot = len(checked)
                ptrs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in p])
                cnts = (ctypes.c_int64 * 6)(*[t.numel() for t in p])
                kinds = (ctypes.c_int * 6)(0, 2, 1, 3, 0, 0)
                L.check(lib.bds_nonfinite_flags(6, ptrs, cnts, kinds, words[0][slot:].data_ptr(), words[1][slot:].data_ptr(), st),
                        "bds_nonfinite_flags")
                checked.append((slot, s))

        def at(t, row, width):      # address of global row `row` of a [N, width] array
            return None if t is None else t.data_ptr() + 4 * row * width

        with L.timed("project_fwd"):
            for s, p in zip(segs, per):
                n, r0 = s["n"], s["start"]
                if n == 0:
                    continue
                outs = (at(radii, r0, 1), at(means2d, r0, 2), at(depths, r0, 1), at(conics, r0, 3))
                if s["raw"]:
                    L.check(lib.bds_project_view_fwd(L.PROJ_ANTIALIASED if aa else 0, n, L.ptr(p[0]), L.ptr(p[1]), L.ptr(p[2]), L.ptr(p[3]),
                                                     L.ptr(viewmat), L.ptr(Kmat), W, H, cfg["eps2d"], cfg["near_plane"], cfg["far_plane"],
                                                     cfg["radius_clip"], at(scales, r0, 3), at(opac, r0, 1), at(opac_eff, r0, 1), *outs,
                                                     None, None, 0, None, st), "bds_project_view_fwd")
                else:
                    scales[r0:r0 + n].copy_(p[2])
                    opac[r0:r0 + n].copy_(p[3].reshape(n))
                    L.check(lib.bds_project_fwd(1, n, L.ptr(p[0]), L.ptr(p[1]), L.ptr(p[2]), L.ptr(p[3]) if aa else None, L.ptr(viewmat),
                                                L.ptr(Kmat), W, H, cfg["eps2d"], cfg["near_plane"], cfg["far_plane"], cfg["radius_clip"],
                                                *outs, None, at(opac_eff, r0, 1), st), "bds_project_fwd")
        opac_c = opac_eff if aa else opac      # what the tile stage and the compositor read
        ls = _lists_begin(means2d, radii, depths, (L.ptr(conics), L.ptr(opac_c)) if cfg["cull"] else None, W, H, _LIST_TILE)
        images = _image_buffers(W, H, dev)      # (while the two counts travel to the host)
        _lists_finish(ls)
        for slot, s in checked:      # (the flag words' copies are older than the event that wait waited for)
            word = int(words[1][slot])
            if word:
                bad = [n for i, n in enumerate(_RAW_FIELDS) if word >> i & 1]
                raise ValueError(f"NaN / Inf detected in gaussian {', '.join(bad)} at step {s['step']}")
        f = _Front()
        f.flatten, f.vis_ids, f.M, f.n_vis, f.m_dev, f.nvis_dev, f.rec_buf = ls.flatten, ls.vis_ids, ls.M, ls.n_vis, ls.m_dev, ls.nvis_dev, ls.rec_buf
        f.cfg, f.W, f.H, f.list_tile, f.tw, f.th = cfg, W, H, _LIST_TILE, math.ceil(W / TILE_SIZE), math.ceil(H / TILE_SIZE)
        f.means, f.means2d, f.depths, f.conics, f.radii, f.isect_offsets = means, means2d, depths, conics, radii, ls.isect_offsets
        f.opac = f.opac_row = opac_c
        f.colors, f.cam_pos = None, cfg["cam_pos"]
        f.scene = _SceneTable(segs, [p[4] for p in per], [p[5] if s["raw"] else None for s, p in zip(segs, per)])
        rec, render, alphas, last_ids = _composite(f, f.opac, images)
        ctx.save_for_backward(means, quats, scales, opac, viewmat, Kmat, rec, f.vis_ids, ls.ws, f.flatten, f.isect_offsets, render, alphas,
                              last_ids, f.sh_rgb, f.cam_pos)
        ctx.cfg, ctx.M = cfg, f.M
        ctx.shapes = [tuple(tuple(t.shape) for t in p) for p in per]
        ctx.mark_non_differentiable(radii, depths, conics, opac_c)
        ctx.set_materialize_grads(False)
        if cfg.get("split"):       # rgb and depth as two outputs (SplitRender): 4-channel modes only
            rgb, depth = torch.empty(H, W, 3, device=dev), torch.empty(H, W, 1, device=dev)
            L.check(lib.bds_expected_depth_split_fwd(H * W, int(cfg["ed"]), L.ptr(render), L.ptr(alphas), L.ptr(rgb), L.ptr(depth), st),
                    "bds_expected_depth_split_fwd")
            return rgb, depth, alphas, means2d, radii, depths, conics, opac_c
        if cfg["ed"]:
            out = torch.empty_like(render)
            L.check(lib.bds_expected_depth_fwd(H * W, L.ptr(render), L.ptr(alphas), L.ptr(out), st), "bds_expected_depth_fwd")
        else:
            out = render[..., :3] if cfg["channels"] == 3 else render
        return out, None, alphas, means2d, radii, depths, conics, opac_c

    @staticmethod
    def backward(ctx, v_out, v_depth, v_alphas, v_means2d_ext, *_):
        saved = ctx.saved_tensors
        means, scales, opac, vis_ids, sh_rgb, cam_pos = saved[0], saved[2], saved[3], saved[7], saved[14], saved[15]
        cfg, want_pose, segs = ctx.cfg, bool(ctx.needs_input_grad[0]), ctx.cfg["segments"]
        # dense outputs over the global rows: means 3 | quats 4 | activated scales 3 | activated opacities 1 | colours 3 | grad2d 2 | absgrad2d 2
        outs, v_rec, slots = _view_backward(ctx, saved, v_out, v_depth, v_alphas, v_means2d_ext, want_pose, (3, 4, 3, 1, 3, 2, 2),
                                            L.PROJ_ACTIVATED)
        v_means, v_quats, v_scales, v_opac, v_colors = outs[:5]
        # the raw segments' SH gradients: their own arrays (ONE zero fill), rows of culled Gaussians stay zero
        sizes = [(s["n"] * 3, s["n"] * (s["K"] - 1) * 3) if s["raw"] else (0, 0) for s in segs]
        pool = torch.zeros(sum(a + b for a, b in sizes), device=means.device)
        v_dc, v_rest, o = [], [], 0
        for (a, b), s in zip(sizes, segs):
            v_dc.append(pool[o:o + a] if s["raw"] else None)
            v_rest.append(pool[o + a:o + a + b] if s["raw"] else None)
            o += a + b
        table = _SceneTable(segs, v_dc, v_rest)
        with L.timed("sh_bwd"):
            L.check(L.lib().bds_scene_sh_bwd(vis_ids.numel(), None, L.ptr(vis_ids), *table.forward_args(), L.ptr(means), L.ptr(cam_pos),
                                             L.ptr(sh_rgb), L.ptr(v_rec), L.ptr(scales), L.ptr(opac), L.ptr(v_scales), L.ptr(v_opac),
                                             L.stream()), "bds_scene_sh_bwd")
        g = ctx.needs_input_grad
        grads, i = [slots.sum(0) if want_pose else None, None, None], 3
        for s, shapes, dc, rest in zip(segs, ctx.shapes, v_dc, v_rest):
            a, b = s["start"], s["start"] + s["n"]
            seg = [v_means[a:b], v_quats[a:b], v_scales[a:b], v_opac[a:b]] + ([dc, rest] if s["raw"] else [v_colors[a:b]])
            for t, shape in zip(seg, shapes):
                grads.append(t.view(shape) if g[i] else None)
                i += 1
        return tuple(grads)


def _view_backward(ctx, saved, v_out, v_depth, v_alphas, v_means2d_ext, want_pose: bool, widths, flags: int):
    """The backward both one-view nodes share: expected depth -> ``fused_view._composite_backward`` (host-count form, + a loss on
    meta["means2d"]) -> ONE zero fill of the dense outputs, ``widths`` floats per Gaussian (the four parameter gradients first, grad2d |
    absgrad2d last) -> ``fused_view._project_backward`` (``flags``; ACTIVATED scatters the colour gradient to the fifth output), which
    gives the means2d carrier .absgrad with cfg["absgrad"] and .grad when it retains it.  Returns (dense outputs, gradient records,
    camera-pose slots or None)."""
    means, quats, scales, opac, viewmat, Kmat, rec, vis_ids, _ws, flatten, isect_offsets, render, alphas, last_ids = saved[:14]
    cfg, lib, st = ctx.cfg, L.lib(), L.stream()
    W, H, N = cfg["width"], cfg["height"], means.shape[0]
    v_render, v_alphas_t = torch.empty_like(render), torch.empty_like(alphas)
    if cfg.get("split"):
        L.check(lib.bds_expected_depth_split_bwd(H * W, int(cfg["ed"]), L.ptr(render), L.ptr(alphas),
                                                 None if v_out is None else L.ptr(L.f32c(v_out)), None if v_depth is None else L.ptr(L.f32c(v_depth)),
                                                 None if v_alphas is None else L.ptr(L.f32c(v_alphas)), L.ptr(v_render), L.ptr(v_alphas_t), st),
                "bds_expected_depth_split_bwd")
    else:
        L.check(lib.bds_expected_depth_bwd(H * W, cfg["channels"], int(cfg["ed"]), L.ptr(render), L.ptr(alphas),
                                           None if v_out is None else L.ptr(L.f32c(v_out)), None if v_alphas is None else L.ptr(L.f32c(v_alphas)),
                                           L.ptr(v_render), L.ptr(v_alphas_t), st), "bds_expected_depth_bwd")
    v_rec_all, v_rec = _composite_backward(cfg, (rec, flatten, isect_offsets, alphas, last_ids), vis_ids, ctx.M, _LIST_TILE,
                                           absgrad=cfg["absgrad"], want_pose=want_pose, v_render=v_render, v_alphas=v_alphas_t,
                                           v_means2d_ext=v_means2d_ext)
    dense = torch.zeros(N * sum(widths), device=means.device)      # ONE zero fill for all dense outputs
    outs, o = [], 0
    for w in widths:
        outs.append(dense[o:o + N * w].view(N, w) if w != 1 else dense[o:o + N])
        o += N * w
    slots = v_rec_all[v_rec.shape[0]:].view(L.POSE_GRAD_SLOTS, 4, 4) if want_pose else None
    _project_backward(cfg, flags | (L.PROJ_ANTIALIASED if cfg["aa"] else 0), None, vis_ids, (means, quats, scales, opac, viewmat, Kmat), v_rec,
                      outs[:4], g2d=outs[-2], ag2d=outs[-1] if cfg["absgrad"] else None,
                      v_colors=outs[4] if flags & L.PROJ_ACTIVATED else None, slots=slots)
    return outs, v_rec, slots


_FINITE_WORDS: Dict[tuple, tuple] = {}


def _finite_words(dev, n: int = 1):
    """(device words, page-locked words) of bds_nonfinite_flags, one pair per device (a view waits for its counts before the next one);
    ``n`` words: one per launch of a view that checks several classes."""
    w = _FINITE_WORDS.get((dev, n))
    if w is None:
        w = _FINITE_WORDS[(dev, n)] = (torch.zeros(n, device=dev, dtype=torch.int32), torch.zeros(n, dtype=torch.int32).pin_memory())
    return w


def _as_int(v) -> int:
    # the reference passes 0-d (GPU) int64 tensors for width/height
    # (/root/reference/project/datasets/base/pixel_source.py:653-654, tools/train.py:262-264)
    if torch.is_tensor(v):
        return int(v.item())
    return int(v)


def rasterization(
    means: Tensor,  # [N, 3]
    quats: Tensor,  # [N, 4]
    scales: Tensor,  # [N, 3]
    opacities: Tensor,  # [N]
    colors: Tensor,  # [(C,) N, D] or [(C,) N, K, 3]
    viewmats: Tensor,  # [C, 4, 4]
    Ks: Tensor,  # [C, 3, 3]
    width,
    height,
    near_plane: float = 0.01,
    far_plane: float = 1e10,
    radius_clip: float = 0.0,
    eps2d: float = 0.3,
    sh_degree: Optional[int] = None,
    packed: bool = True,
    tile_size: int = 16,
    backgrounds: Optional[Tensor] = None,
    render_mode: str = "RGB",
    sparse_grad: bool = False,
    absgrad: bool = False,
    rasterize_mode: str = "classic",
    channel_chunk: int = 32,
    distributed: bool = False,
    covars: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Dict]:
    """Returns (render_colors [C,H,W,D], render_alphas [C,H,W,1], meta).

    ``packed`` / ``sparse_grad`` / ``channel_chunk`` only select memory layouts inside gsplat; results
    are identical, so they are accepted and ignored (the dense layout is used: one camera per step on
    the reference's path).  ``distributed`` (gsplat's Gaussian-sharded mode) and ``covars`` are not
    used by the reference and raise."""
    if distributed:
        raise NotImplementedError("distributed=True (Gaussian-sharded rendering) is not on the reference's path; "
                                  "multi-GPU here shards views, see bilateral_driving_amd.dist")
    if covars is not None:
        raise NotImplementedError("covars= is not on the reference's path (quats/scales are passed)")
    assert render_mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED"), render_mode
    assert rasterize_mode in ("classic", "antialiased"), rasterize_mode
    assert tile_size >= TILE_SIZE and tile_size % TILE_SIZE == 0, (
        f"tile_size={tile_size}: a multiple of {TILE_SIZE} is required (lists of larger tiles are filtered per 16-px compositing tile)")
    src = lazy_source(means, quats, scales, opacities, colors)     # marshalling.install: a class's raw parameters behind placeholders
    raw_ok = (src is not None and _ONE_VIEW_NODE and viewmats.shape[0] == 1 and sh_degree is None and backgrounds is None
              and render_mode in ("RGB", "RGB+ED") and means.shape[0] > 0 and src.features_rest.shape[1] >= 1)
    # several classes, some of them behind placeholders (marshalling.install(cls, scene=True)): under the same conditions, one node
    scene = None if raw_ok else lazy_scene(means, quats, scales, opacities, colors)
    scene_ok = (scene is not None and _ONE_VIEW_NODE and viewmats.shape[0] == 1 and sh_degree is None and backgrounds is None
                and render_mode in ("RGB", "RGB+ED") and means.shape[0] > 0)
    if not raw_ok and not scene_ok:
        means, quats, scales, opacities, colors = materialised((means, quats, scales, opacities, colors))
    N = means.shape[0]
    C = viewmats.shape[0]
    assert means.shape == (N, 3), means.shape
    assert quats.shape == (N, 4), quats.shape
    assert scales.shape == (N, 3), scales.shape
    assert opacities.shape == (N,), opacities.shape
    assert viewmats.shape == (C, 4, 4), viewmats.shape
    assert Ks.shape == (C, 3, 3), Ks.shape
    width, height = _as_int(width), _as_int(height)

    if sh_degree is None:
        # post-activation colours [N, D] or [C, N, D]
        assert (colors.dim() == 2 and colors.shape[0] == N) or (colors.dim() == 3 and colors.shape[:2] == (C, N)), colors.shape
    else:
        assert (colors.dim() == 3 and colors.shape[0] == N and colors.shape[2] == 3) or (
            colors.dim() == 4 and colors.shape[:2] == (C, N) and colors.shape[3] == 3), colors.shape
        assert (sh_degree + 1) ** 2 <= colors.shape[-2], colors.shape

    def _meta(radii, means2d, depths, conics, opacities, lists=(None, None, None, None)):     # (lists None: materialised on first access)
        tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = lists
        return _Meta({"camera_ids": None, "gaussian_ids": None, "radii": radii, "means2d": means2d, "depths": depths, "conics": conics,
                      "opacities": opacities, "tile_width": math.ceil(width / float(tile_size)),
                      "tile_height": math.ceil(height / float(tile_size)), "tiles_per_gauss": tiles_per_gauss, "isect_ids": isect_ids,
                      "flatten_ids": flatten_ids, "isect_offsets": isect_offsets, "width": width, "height": height,
                      "tile_size": tile_size, "n_cameras": C, "_cull": _TILE_CULLING})

    def _one_view_cfg(**own):      # what the two one-view nodes' cfg share
        return dict(width=width, height=height, eps2d=float(eps2d), near_plane=float(near_plane), far_plane=float(far_plane),
                    radius_clip=float(radius_clip), ed=render_mode == "RGB+ED", channels=3 if render_mode == "RGB" else 4,
                    absgrad=bool(absgrad), cull=_TILE_CULLING, aa=rasterize_mode == "antialiased", **own)

    if raw_ok:
        cfg = _one_view_cfg(sh_degree=src.sh_degree, cam_pos=L.f32c(src.cam_pos.detach().reshape(3)), logits_shape=tuple(src.logits.shape),
                           step=src.step, check_finite=_CHECK_FINITE, split=_SPLIT_RENDER and render_mode != "RGB")
        out, depth1, alphas, means2d, radii, depths, conics, opac = _RasterizeRawView.apply(
            src.means, src.quats, src.log_scales, src.logits, src.features_dc, src.features_rest, viewmats[0], Ks[0], cfg)
        if depth1 is not None:      # the render as a placeholder over the node's two image outputs (SplitRender)
            out = SplitRender(out[None], depth1[None], first=(out, depth1))
        cfg["_means2d_ref"] = weakref.ref(means2d)      # the backward attaches .absgrad (and .grad, when retained) to THIS tensor object
        return out, alphas, _meta(radii, means2d, depths, conics, opac.detach()[None, :])

    if scene_ok:
        segs, tensors = [], []
        for s in scene:
            if s.raw:
                r = s.src
                segs.append(dict(raw=True, start=s.start, n=s.n, K=1 + r.features_rest.shape[1], deg=r.sh_degree, step=r.step))
                tensors += [r.means, r.quats, r.log_scales, r.logits, r.features_dc, r.features_rest]
            else:
                segs.append(dict(raw=False, start=s.start, n=s.n, K=1, deg=0, step=-1))
                tensors += list(s.dense)
        first = next(s.src for s in scene if s.raw)
        cfg = _one_view_cfg(N=N, segments=segs, cam_pos=L.f32c(first.cam_pos.detach().reshape(3)), check_finite=_CHECK_FINITE,
                           split=_SPLIT_RENDER and render_mode != "RGB")
        out, depth1, alphas, means2d, radii, depths, conics, opac = _RasterizeSceneView.apply(viewmats[0], Ks[0], cfg, *tensors)
        if depth1 is not None:
            out = SplitRender(out[None], depth1[None], first=(out, depth1))
        cfg["_means2d_ref"] = weakref.ref(means2d)
        return out, alphas, _meta(radii, means2d, depths, conics, opac.detach()[None, :])

    if (_ONE_VIEW_NODE and C == 1 and N > 0 and sh_degree is None and colors.shape[-1] == 3 and backgrounds is None
            and render_mode in ("RGB", "RGB+ED")):
        cfg = _one_view_cfg(colors_shape=tuple(colors.shape))
        out, alphas, means2d, radii, depths, conics, opac_eff = _RasterizeView.apply(means, quats, scales, opacities, colors, viewmats[0], Ks[0],
                                                                                     cfg)
        cfg["_means2d_ref"] = weakref.ref(means2d)
        return out, alphas, _meta(radii, means2d, depths, conics, opacities.detach()[None, :] if opac_eff is None else opac_eff)

    radii, means2d, depths, conics, compensations = fully_fused_projection(
        means, quats, scales, viewmats, Ks, width, height, eps2d=eps2d, near_plane=near_plane, far_plane=far_plane,
        radius_clip=radius_clip, calc_compensations=(rasterize_mode == "antialiased"))
    opac = opacities[None, :].expand(C, N)
    if compensations is not None:
        opac = opac * compensations

    if sh_degree is None:
        col = colors if colors.dim() == 3 else colors[None].expand(C, N, colors.shape[-1])
    else:
        camtoworlds = torch.linalg.inv(viewmats)
        dirs = means[None, :, :] - camtoworlds[:, None, :3, 3]  # [C, N, 3]
        shs = colors if colors.dim() == 4 else colors[None].expand(C, N, colors.shape[-2], 3)
        col = spherical_harmonics(sh_degree, dirs, shs, masks=radii > 0)
        col = torch.clamp_min(col + 0.5, 0.0)

    if render_mode in ("RGB+D", "RGB+ED"):
        col = torch.cat([col, depths[..., None]], dim=-1)
        if backgrounds is not None:
            backgrounds = torch.cat([backgrounds, torch.zeros(C, 1, device=backgrounds.device)], dim=-1)
    elif render_mode in ("D", "ED"):
        col = depths[..., None]
        if backgrounds is not None:
            backgrounds = torch.zeros(C, 1, device=backgrounds.device)

    tile_width, tile_height = math.ceil(width / float(tile_size)), math.ceil(height / float(tile_size))
    tiles_per_gauss, isect_ids, flatten_ids, isect_offsets = isect_tiles(means2d, radii, depths, tile_size, tile_width,
                                                                         tile_height, want_isect_ids=False,
                                                                         conics=conics if _TILE_CULLING else None,
                                                                         opacities=opac.contiguous() if _TILE_CULLING else None)
    render_colors, render_alphas = rasterize_to_pixels(means2d, conics, col.contiguous(), opac.contiguous(), width, height,
                                                       tile_size, isect_offsets, flatten_ids, backgrounds=backgrounds,
                                                       absgrad=absgrad)
    if render_mode in ("ED", "RGB+ED"):
        render_colors = torch.cat(
            [render_colors[..., :-1], render_colors[..., -1:] / render_alphas.clamp(min=1e-10)], dim=-1)

    return render_colors, render_alphas, _meta(radii, means2d, depths, conics, opac, (tiles_per_gauss, isect_ids, flatten_ids, isect_offsets))
