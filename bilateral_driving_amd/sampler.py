"""The error-driven image sampler on the device (csrc/error_buffer.hip through ``bds_error_maps``): the per-image error maps, the
per-image mean errors and the weighted draw of the next training image.

Reference: every ``cache_buffer_freq`` steps (tools/train.py:322-337) ``render_images`` renders every image at 1 / ``buffer_downscale``
and copies about twenty arrays per view to numpy (models/video_utils.py:184-260); ``ScenePixelSource.update_image_error_maps``
(datasets/base/pixel_source.py:948-983) re-stacks the lists per camera on the host, ``CameraData.update_image_error_maps`` (:431-449)
forms ``abs(gt - pred).mean(-1)``, multiplies by 5 where ``Dynamic_opacity > 0.1``, copies the maps to the device and takes one mean per
image.  Every training step, ``propose_training_image`` (:909-936) gathers the buffer, rebuilds ``error_weight`` on the host, uploads
it, multiplies and calls ``torch.multinomial(...).item()``: several launches, one copy and one blocking read-back per step for a buffer
that changes every 2000 steps.

* ``error_maps(pred, gt, dyn, maps, slots, stats, img_ids, ws=None)``: the maps and (mean, min, max) of B views in one call, no wait.
* ``ErrorSweep(pixel_source)``: the streaming form.  ``add(results, image_infos, cam_infos)`` takes one rendered view's device tensors
  and enqueues one call; ``finish()`` sets every camera's ``image_error_maps``, ``pixel_source.image_error_buffer`` and
  ``image_error_buffered``, keeps the per-image minima and maxima, reads the statistics back once and keeps them for the draw.
* ``update_image_error_maps(pixel_source, render_results)``: the reference's name and argument (the dict of numpy lists that
  ``render_images`` returns), for the unmodified ``train.py``: per camera one upload and one batched call.
* ``cache_image_errors(trainer, dataset)``: train.py:327-337 without the host round trip.
* ``get_image_error_video(camera_data)``: pixel_source.py:404-429, normalised with the kept minimum and maximum.
* ``DrawTable`` and ``propose_training_image(pixel_source, candidate_indices)``: the weighted draw from a host table that is rebuilt
  when the buffer or the candidate list changes.  Per step: no launch, no copy, no read-back.
* ``install(CameraData, ScenePixelSource)`` sets ``get_image_error_video`` on the first and ``update_image_error_maps`` and
  ``propose_training_image`` on the second; ``uninstall`` puts the former back.  An object whose tensors live on the CPU keeps the
  class's own methods.

The pixel formula (csrc/error_buffer_math.h): e = ((|g0 - c0| + |g1 - c1|) + |g2 - c2|) / 3 with c = clamp(p, 0, 1), times 5 where
dyn > 0.1f.  The clamp is the one ``render_images`` applies to every ``*rgb*`` result (video_utils.py:185-187): ``ErrorSweep`` takes
the unclamped render, and on the clamped arrays of ``render_results`` it changes nothing.

Deviations.  The draw has ``torch.multinomial``'s distribution (inverse CDF over the same weights) but not its random stream: it takes
one ``random.random()`` where the reference consumes torch's generator.  The means are sums in float64 in a fixed order, rounded to
float32 once; torch's are float32 sums in its own order.  ``image_error_buffer`` slots are addressed by ``img_idx`` in the streaming
form, not by the order of the rendered list; the two agree for the full image set that ``train.py`` passes.  A buffer that is changed
in place (not replaced) after a table was built is not noticed.

Read-backs: one per ``finish()`` (the statistics, [num_imgs,3] float32).  ``add`` reads nothing back when ``cam_infos`` carries
``cam_name`` (the reference's always does) or a host ``cam_id``; a ``cam_id`` that only exists on the device is read to pick the camera.

Not included: the multi-GPU split of the sweep, ``render_images`` itself, the mp4 encoder.  The videos' frames -- ``dataset.layout``,
the depth colours and the 8-bit quantiser -- are video.py's."""
from __future__ import annotations

import bisect
import math
import random
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam
from .metrics import grown
from .pixels import _dispatch

MAX_ROWS = 2 ** 31 - 1      # include/bds.h: B h w of one call
UNSET = -1.0                # a statistics row that no view has written yet: an error is never negative


def _f32_out(t: Tensor, what: str) -> None:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor (the call writes into it)")


def _ids(t: Tensor, B: int, what: str) -> Tensor:
    if not isinstance(t, Tensor) or t.dtype != torch.int64 or t.numel() != B:
        raise ValueError(f"{what} must be an int64 tensor of {B} values")
    return t.reshape(-1).contiguous()


@torch.no_grad()
def error_maps(pred: Tensor, gt: Tensor, dyn: Optional[Tensor], maps: Tensor, slots: Tensor, stats: Tensor, img_ids: Tensor,
               ws: Optional[Tensor] = None) -> Tensor:
    """``pred``, ``gt`` [B,h,w,3] (or [h,w,3]) and ``dyn`` [B,h,w] or None, float32 on the device; ``slots``, ``img_ids`` [B] int64 on
    the device.  Writes view b's map into ``maps[slots[b]]`` (``maps`` [F,h,w] float32) and (mean, min, max) of it into
    ``stats[img_ids[b]]`` (``stats`` [num_imgs,3] float32); other rows keep their bits.  The slots of one call must differ, and so must
    the ids.  Returns the workspace it used (``ws`` where that was large enough).  No host wait.  BdsError for a CPU tensor, ValueError
    for a shape that does not fit."""
    if pred.dim() == 3:
        pred, gt, dyn = pred[None], gt[None], None if dyn is None else dyn[None]
    if pred.dim() != 4 or pred.shape[-1] != 3:
        raise ValueError(f"pred must be [B,h,w,3] or [h,w,3], got {tuple(pred.shape)}")
    if gt.shape != pred.shape:
        raise ValueError(f"gt {tuple(gt.shape)} must have pred's shape {tuple(pred.shape)}")
    B, h, w = (int(s) for s in pred.shape[:3])
    if dyn is not None and tuple(dyn.shape) != (B, h, w):
        raise ValueError(f"dyn must be [B,h,w] = {(B, h, w)}, got {tuple(dyn.shape)}")
    if maps.dim() != 3 or tuple(maps.shape[1:]) != (h, w):
        raise ValueError(f"maps must be [F,h,w] with (h, w) = {(h, w)}, got {tuple(maps.shape)}")
    if stats.dim() != 2 or stats.shape[1] != 3:
        raise ValueError(f"stats must be [num_imgs,3], got {tuple(stats.shape)}")
    if B * h * w > MAX_ROWS:
        raise ValueError(f"one call takes B*h*w <= {MAX_ROWS}, got B={B}, h={h}, w={w}")
    _f32_out(maps, "maps")
    _f32_out(stats, "stats")
    slots, img_ids = _ids(slots, B, "slots"), _ids(img_ids, B, "img_ids")
    L.require_gpu(pred, gt, dyn, maps, slots, stats, img_ids, ws)
    pred, gt, dyn = L.f32c(pred.detach()), L.f32c(gt.detach()), L.f32c(None if dyn is None else dyn.detach())
    lib = L.lib()
    ws = grown(ws, int(lib.bds_error_maps_workspace_bytes(B, h, w)), pred.device)
    L.check(lib.bds_error_maps(B, h, w, L.ptr(pred), L.ptr(gt), L.ptr(dyn), L.ptr(slots), L.ptr(img_ids), L.ptr(maps), int(maps.shape[0]),
                               L.ptr(stats), int(stats.shape[0]), L.ptr(ws), ws.numel(), L.stream()), "bds_error_maps")
    return ws


# ----------------------------------------------------------------------------------------------------------------------------------
# the buffer update
# ----------------------------------------------------------------------------------------------------------------------------------
def _cameras(pixel_source) -> Dict[object, object]:
    """{cam_id: camera} in ``camera_list``'s order."""
    return {cam_id: pixel_source.camera_data[cam_id] for cam_id in pixel_source.camera_list}


def _device_of(pixel_source):
    for cam in _cameras(pixel_source).values():
        for t in (getattr(cam, "image_error_maps", None), getattr(cam, "cam_to_worlds", None)):
            if isinstance(t, Tensor):
                return t.device
    return torch.device(pixel_source.device)


def _first(v, dev) -> Tensor:
    """An index as a 1-element int64 device tensor: a device tensor's first element as a view of it (no launch, no read-back), a host
    value through one small copy."""
    if isinstance(v, Tensor) and v.is_cuda and v.dtype == torch.int64 and v.numel() > 0 and v.is_contiguous():
        return v.reshape(-1)[:1]
    if isinstance(v, Tensor):
        return v.reshape(-1)[:1].to(device=dev, dtype=torch.int64)
    return torch.tensor([int(v)], dtype=torch.int64).to(dev)


def _commit(pixel_source, staged: Mapping[object, Tensor], stats: Tensor, rows: Mapping[object, Tensor], complete: bool = False) -> None:
    """Hands a finished update over: ``staged`` {cam_id: [num_frames,h,w]}, ``stats`` [num_imgs,3] on the device, ``rows`` {cam_id: the
    camera's image ids, int64 on the device}.  ``complete``: ValueError, with nothing handed over, when a row of ``stats`` is ``UNSET``."""
    host = stats.cpu().numpy()                                  # the update's one read-back
    if complete and bool((host[:, 0] == UNSET).any()):          # (a frame given twice leaves another one's row unset)
        raise ValueError("the sweep left images without an error: a frame was given twice and another one never")
    for cam_id, cam in _cameras(pixel_source).items():
        r = stats[rows[cam_id]]
        cam.image_error_maps = staged[cam_id]
        if r.shape[0]:
            cam._bds_error_range = (staged[cam_id], r[:, 1].min(), r[:, 2].max())      # (torch's min / max: a NaN stays)
    pixel_source.image_error_buffer = stats[:, 0].contiguous()
    pixel_source.image_error_buffered = True
    pixel_source.image_error_stats = stats                     # [num_imgs,3]: mean, min, max per image
    pixel_source._bds_buffer_host = (pixel_source.image_error_buffer, host[:, 0].copy())
    pixel_source._bds_draw_tables = []


class ErrorSweep:
    """One update of the error buffer, view by view: ``add`` per rendered view (one call into the library each, nothing read back),
    then ``finish()``.  The maps are staged: a sweep that ``finish()`` refuses leaves the pixel source as it was.  ``add`` must be called
    on ONE stream: the views share a workspace, which the launches of one stream use in order."""

    def __init__(self, pixel_source):
        self.source = pixel_source
        self.cams = _cameras(pixel_source)
        self.by_name = {cam.cam_name: cam_id for cam_id, cam in self.cams.items() if getattr(cam, "cam_name", None) is not None}
        self.device = _device_of(pixel_source)
        self.num_imgs = int(pixel_source.num_imgs)
        self.stats = torch.full((self.num_imgs, 3), UNSET, dtype=torch.float32, device=self.device)
        self.staged: Dict[object, Tensor] = {}
        self.count = {cam_id: 0 for cam_id in self.cams}
        self._ws = None
        self._stream = None

    def _camera(self, cam_infos):
        name = cam_infos.get("cam_name")
        if name in self.by_name:
            return self.by_name[name]
        cam_id = cam_infos["cam_id"]
        cam_id = int(cam_id.reshape(-1)[0]) if isinstance(cam_id, Tensor) else int(np.asarray(cam_id).reshape(-1)[0])
        if cam_id not in self.cams:
            raise ValueError(f"cam_id {cam_id} names no camera of the pixel source ({sorted(self.cams)})")
        return cam_id

    @torch.no_grad()
    def add(self, results: Mapping[str, Tensor], image_infos: Mapping[str, Tensor], cam_infos: Mapping[str, object]) -> None:
        """``results["rgb"]`` [h,w,3], unclamped, and ``results.get("Dynamic_opacity")`` [h,w,1] or [h,w]; ``image_infos["pixels"]``
        [h,w,3], ``image_infos["img_idx"]`` and ``image_infos["frame_idx"]`` (any shape, the first element counts);
        ``cam_infos["cam_name"]`` or ``cam_infos["cam_id"]``."""
        rgb, gt = results["rgb"], image_infos["pixels"]
        L.require_gpu(rgb, gt, self.stats)
        cam_id = self._camera(cam_infos)
        cam = self.cams[cam_id]
        if rgb.dim() != 3 or rgb.shape[-1] != 3 or rgb.shape != gt.shape:
            raise ValueError(f"rgb {tuple(rgb.shape)} and pixels {tuple(gt.shape)} must be one [h,w,3]")
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        want = (int(cam.num_frames),) + tuple(int(s) for s in cam.image_error_maps.shape[1:])
        if (h, w) != want[1:]:
            raise ValueError(f"camera {cam_id}: a view of {(h, w)} does not fit its error maps {want}")
        dyn = results.get("Dynamic_opacity")
        if dyn is not None:
            if dyn.numel() != h * w:
                raise ValueError(f"Dynamic_opacity {tuple(dyn.shape)} must hold {(h, w)}")
            dyn = dyn.reshape(1, h, w)
        stream = L.stream()
        if self._stream is None:
            self._stream = stream
        elif stream != self._stream:
            raise L.BdsError("ErrorSweep.add was called on another stream than before: the views share one workspace")
        if cam_id not in self.staged:
            self.staged[cam_id] = torch.empty(want, dtype=torch.float32, device=self.device)
        self._ws = error_maps(rgb[None], gt[None], dyn, self.staged[cam_id], _first(image_infos["frame_idx"], self.device), self.stats,
                              _first(image_infos["img_idx"], self.device), self._ws)
        self.count[cam_id] += 1

    def finish(self) -> None:
        """Raises ValueError when a camera did not receive every one of its frames exactly once (the reference's
        ``assert image_error_maps.shape == self.image_error_maps.shape``); the pixel source is then unchanged."""
        for cam_id, cam in self.cams.items():
            if self.count[cam_id] != int(cam.num_frames):
                raise ValueError(f"camera {cam_id} received {self.count[cam_id]} views for its {int(cam.num_frames)} frames")
        ids = torch.arange(self.num_imgs, device=self.device)
        num_cams = int(self.source.num_cams)
        rows = {cam_id: ids[ids % num_cams == int(cam.unique_cam_idx)] for cam_id, cam in self.cams.items()}      # parse_img_idx, :808-809
        _commit(self.source, self.staged, self.stats, rows, complete=True)


@torch.no_grad()
def update_image_error_maps(self, render_results: Mapping[str, Sequence]) -> None:
    """pixel_source.py:948-983 on a ``ScenePixelSource`` whose tensors live on the device, for the dict of numpy lists that
    ``render_images`` returns: per camera one upload of the stacked arrays and one batched call.  As the reference, a camera's views
    are the entries of its ``cam_name``, in the list's order; their buffer slots are the positions whose ``cam_ids`` entry is the
    camera's ``cam_id``; images that no camera names get 0.  ValueError where the reference's shape assertion fails."""
    dev = _device_of(self)
    L.require_gpu(torch.empty(0, device=dev))
    num_imgs = int(self.num_imgs)
    stats = torch.zeros(num_imgs, 3, dtype=torch.float32, device=dev)
    image_cam_id = np.stack([np.asarray(c) for c in render_results["cam_ids"]], axis=0).reshape(-1)
    staged, rows, ws = {}, {}, None
    for cam_id, cam in _cameras(self).items():
        at = [i for i, name in enumerate(render_results["cam_names"]) if name == cam.cam_name]
        ids = np.flatnonzero(image_cam_id == cam_id).astype(np.int64)
        want = tuple(int(s) for s in cam.image_error_maps.shape)
        B, h, w = want
        gt = np.stack([np.asarray(render_results["gt_rgbs"][i], np.float32) for i in at], axis=0) if at else np.zeros((0, h, w, 3), np.float32)
        pred = np.stack([np.asarray(render_results["rgbs"][i], np.float32) for i in at], axis=0) if at else np.zeros((0, h, w, 3), np.float32)
        if gt.shape != want + (3,) or pred.shape != want + (3,) or len(ids) != B or (len(ids) and int(ids.max()) >= num_imgs):
            raise ValueError(f"camera {cam_id}: {len(at)} views of {tuple(pred.shape[1:3])} for error maps {want} and {len(ids)} buffer slots")
        dyn = None
        if len(render_results.get("Dynamic_opacities", ())) > 0:
            dyn = np.stack([np.asarray(render_results["Dynamic_opacities"][i], np.float32) for i in at], axis=0).reshape(B, h, w)
        # one buffer, one copy: {slots, ids} int64, then the float32 arrays, each from a 16-byte boundary
        n = B * h * w
        off, sizes = [16 * ((2 * 8 * B + 15) // 16)], [12 * n, 12 * n] + ([4 * n] if dyn is not None else [])
        for s in sizes:
            off.append(off[-1] + 16 * ((s + 15) // 16))
        buf = np.zeros(off[-1], np.uint8)
        words = buf[:16 * B].view(np.int64)
        words[:B], words[B:] = np.arange(B), ids
        for o, s, a in zip(off, sizes, [pred, gt] + ([dyn] if dyn is not None else [])):
            buf[o:o + s] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        d = torch.from_numpy(buf).to(dev)
        on_dev = [d[o:o + s].view(torch.float32) for o, s in zip(off, sizes)]
        idx = d[:16 * B].view(torch.int64)
        staged[cam_id] = torch.empty(want, dtype=torch.float32, device=dev)
        ws = error_maps(on_dev[0].view(B, h, w, 3), on_dev[1].view(B, h, w, 3), on_dev[2].view(B, h, w) if dyn is not None else None,
                        staged[cam_id], idx[:B], stats, idx[B:], ws)
        rows[cam_id] = idx[B:]
    _commit(self, staged, stats, rows)


@torch.no_grad()
def cache_image_errors(trainer, dataset) -> None:
    """tools/train.py:327-337 with the views left on the device: ``trainer.set_eval()``, the downscale factor set to
    1 / ``buffer_downscale``, every image of ``dataset.full_image_set`` fetched and rendered as ``render_images`` does
    (models/video_utils.py:169-182) and handed to an ``ErrorSweep``, the factor reset, ``finish()``."""
    source = dataset.pixel_source
    trainer.set_eval()
    source.update_downscale_factor(1 / source.buffer_downscale)
    try:
        sweep = ErrorSweep(source)
        split = dataset.full_image_set
        camera_downscale = trainer._get_downscale_factor()
        for i in range(len(split)):
            image_infos, cam_infos = split.get_image(i, camera_downscale)
            image_infos = {k: v.cuda(non_blocking=True) if isinstance(v, Tensor) else v for k, v in image_infos.items()}
            cam_infos = {k: v.cuda(non_blocking=True) if isinstance(v, Tensor) else v for k, v in cam_infos.items()}
            sweep.add(trainer(image_infos, cam_infos), image_infos, cam_infos)
    finally:
        source.reset_downscale_factor()
    sweep.finish()


@torch.no_grad()
def get_image_error_video(self) -> List[np.ndarray]:
    """pixel_source.py:404-429 on a ``CameraData``: the maps normalised to [0, 1] with the reference's expression, as a list of
    [H // buffer_downscale, W // buffer_downscale] arrays.  The minimum and maximum are the ones the last update kept (the extremes of
    the per-image ones); maps that did not come from such an update are searched as the reference does."""
    maps = self.image_error_maps
    kept = getattr(self, "_bds_error_range", None)
    if kept is not None and kept[0] is maps:
        lo, hi = kept[1], kept[2]
    else:
        lo, hi = maps.min(), maps.max()
    image_error_maps = (maps - lo) / (hi - lo)
    loss_maps = image_error_maps.detach().cpu().numpy().reshape(self.num_frames, self.HEIGHT // self.buffer_downscale,
                                                                self.WIDTH // self.buffer_downscale)
    return [loss_maps[i] for i in range(self.num_frames)]


# ----------------------------------------------------------------------------------------------------------------------------------
# the draw
# ----------------------------------------------------------------------------------------------------------------------------------
class DrawTable:
    """The weights that the reference hands to ``torch.multinomial`` (pixel_source.py:915-927) for one buffer and one candidate list,
    in float64 on the host, with their running sum.  ``buffer``: the per-image mean errors as host values ([num_imgs]: numpy, list or
    CPU tensor).  RuntimeError where ``torch.multinomial`` raises: a negative or NaN weight, or a sum that is not positive and finite."""

    def __init__(self, buffer, candidate_indices, num_imgs: int, num_cams: int, start_enhance_weight=1):
        self.candidates = list(candidate_indices)
        at = np.asarray([int(c) for c in self.candidates], np.int64)
        buffer = buffer.detach().numpy() if isinstance(buffer, Tensor) else np.asarray(buffer)
        w = buffer.astype(np.float64).reshape(-1)[at]
        if start_enhance_weight > 1:
            # increase the error of the first 10% frames: the expression of :919-924, evaluated once per table
            frame_num = int(num_imgs / num_cams)
            error_weight = torch.cat((
                torch.linspace(start_enhance_weight, 1, int(frame_num * 0.1)),
                torch.ones(frame_num - int(frame_num * 0.1))
            ))
            error_weight = error_weight[..., None].repeat(1, num_cams).reshape(-1)
            w = w * error_weight.double().numpy()[at]
        if len(w) == 0 or bool(np.isnan(w).any()) or bool((w < 0).any()):
            raise RuntimeError("the draw's weights hold a NaN or a negative entry, or there is no candidate")
        self.weights = w
        self.running = np.cumsum(w).tolist()      # (sequential, in float64)
        self.total = self.running[-1]
        if not (self.total > 0.0 and math.isfinite(self.total)):
            raise RuntimeError(f"the draw's weights sum to {self.total!r}, not to a positive finite number")
        self.last = int(np.flatnonzero(w)[-1])

    def position(self, u: float) -> int:
        """The first position whose running sum exceeds ``u * total`` (``u`` in [0, 1)), at most the last one of non-zero weight: a
        candidate of zero weight is never drawn."""
        return min(bisect.bisect_right(self.running, u * self.total), self.last)

    def draw(self, u: float):
        return self.candidates[self.position(u)]


MAX_TABLES = 4      # candidate lists kept per buffer (train.py draws from one)


def _host_buffer(pixel_source) -> np.ndarray:
    """The buffer's host copy: the one the update kept, else (a buffer set by someone else) read back once and kept."""
    kept = getattr(pixel_source, "_bds_buffer_host", None)
    buf = pixel_source.image_error_buffer
    if kept is None or kept[0] is not buf:
        kept = (buf, buf.detach().cpu().numpy().astype(np.float32))
        pixel_source._bds_buffer_host = kept
        pixel_source._bds_draw_tables = []
    return kept[1]


def draw_table(pixel_source, candidate_indices) -> DrawTable:
    """The pixel source's table for ``candidate_indices``: the cached one while the buffer is the same object and the list has the same
    contents, else a new one."""
    host = _host_buffer(pixel_source)
    weight = pixel_source.data_cfg.sampler.get('start_enhance_weight', 1)
    tables = pixel_source._bds_draw_tables
    cands = candidate_indices if isinstance(candidate_indices, list) else [int(c) for c in candidate_indices]
    for kept_weight, table in tables:
        if kept_weight == weight and table.candidates == cands:
            return table
    table = DrawTable(host, list(cands), int(pixel_source.num_imgs), int(pixel_source.num_cams), weight)
    tables.append((weight, table))
    del tables[:-MAX_TABLES]
    return table


def propose_training_image(self, candidate_indices=None):
    """pixel_source.py:909-936 on a ``ScenePixelSource``: with probability ``buffer_ratio``, once the buffer is filled, a candidate
    drawn by its mean error (times the first frames' weight), else ``random.choice``.  The weighted branch takes one more
    ``random.random()``."""
    if random.random() < self.buffer_ratio and self.image_error_buffered:
        # sample according to the image error buffer
        return draw_table(self, candidate_indices).draw(random.random())
    # random sample one from candidate_indices
    return random.choice(candidate_indices)


_SEAM = Seam()


def install(camera_data_class=None, scene_pixel_source_class=None) -> None:
    """Sets ``get_image_error_video`` on ``camera_data_class`` (the reference's ``CameraData``) and ``update_image_error_maps`` and
    ``propose_training_image`` on ``scene_pixel_source_class`` (its ``ScenePixelSource``).  An object whose tensors live on the CPU
    keeps the class's own method, defined on the class or inherited."""
    for target, fns in ((camera_data_class, {"get_image_error_video": get_image_error_video}),
                        (scene_pixel_source_class, {"update_image_error_maps": update_image_error_maps,
                                                    "propose_training_image": propose_training_image})):
        if target is not None:
            _SEAM.install(target, {name: _dispatch(fn, target, name, _SEAM) for name, fn in fns.items()})


def uninstall(*targets) -> None:
    """Puts back what ``install`` replaced (no target given: on every installed one)."""
    _SEAM.uninstall(*targets)
