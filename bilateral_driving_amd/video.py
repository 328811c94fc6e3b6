"""The evaluation video frames on the device (csrc/video.hip through ``bds_video_frame``): the depth colours, the dataset layouts, the
vertical stack of the keys and the 8-bit quantiser, one launch per finished frame.

Reference: ``render`` copies every rendered view to the host as about twenty float32 arrays (models/video_utils.py:184-262);
``save_concatenated_videos`` (:703-768) and ``save_seperate_videos`` (:771-857) then, per timestep and key, run ``depth_visualizer`` on
every depth map (utils/visualization.py:491-497), tile the cameras with ``layout_*`` (:41-341) into a zeroed float32 canvas, crop it,
concatenate the keys and quantise with ``to8b`` (:19-22), all in numpy.  Here the frame is a table of rectangles over the device tensors
and one kernel writes the uint8 canvas; only that canvas, 3 bytes per pixel, crosses to the host.

* ``plan_layout(dataset_type, cam_names, sizes)``: host logic, cached: the six layouts as rectangles of the cropped canvas.
* ``to8b(x)``, ``depth_visualizer(frame, opacity)``, ``over_green(rgb, opacity)``, ``lidar_on_image(pixels, depth_map)``: the
  reference's names (the last two its expressions of :201-227 and :265-271) on device tensors, each a one-panel frame.
* ``FrameComposer(dataset_type, keys)``: ``frame(render_results, cam_names, first)`` is the merged uint8 canvas of one timestep in one
  launch, ``key_frame(key, ...)`` one key's.
* ``save_concatenated_videos`` and ``save_seperate_videos``: the reference's names, arguments and returns, over ``render_results`` whose
  lists hold device tensors (a numpy array is uploaded); one ``.cpu()`` of the uint8 canvas per written frame.
* ``install(models.video_utils)`` sets the two ``save_*`` functions on the reference's module; ``uninstall`` puts the former back.

The key rules are the reference's: a key with ``mask`` in it shows the ``opacities`` list of the same prefix as grey; a key with
``depth`` takes its weight from the matching ``opacities`` list, ``median_depths`` falling back to ``opacities``, and is skipped where
that list is missing; any other key is an [h,w,3] image; a key whose list is absent or empty is skipped.  The ``mask`` rule comes first,
so ``gt_sky_masks`` looks for ``gt_sky_opacitiess`` and is skipped, as in the reference.

Layout quirks kept: nuplan crops ``min:max+1``, the other five ``min:max`` and so drop the last filled row and column; waymo
bottom-aligns a shorter side camera; argoverse shifts the rear cameras by half a height and shows the first ``landscape_height``
rows of the centre camera; a camera name that the layout does not know is ignored; where two panels cover one pixel (a name given
twice) the later one wins, as the reference's successive assignments do.  ValueError where the reference raises one: no
``front_camera`` for waymo, no panel filled, an image that does not fit its slot.

Deviations.  A NaN quantises to 0 (numpy's cast of a NaN is unspecified).  A depth pixel may show a neighbouring entry of the colour
table where the float64 value 256 s lies within 2^-10 of an integer (the device's logf and numpy's differ in the last place).
An image that numpy would broadcast into its slot (one pixel high or wide) is refused.  float64 arrays are shown as float32, which is
what the layouts' canvas makes of them.

Not included: ``render()``'s own per-key host lists, ``error_maps`` of ``render`` (a squared-error normalisation that differs from the
sampler's maps), ``dump_3d_bbox_on_image``, the mp4 encoder (``writer_factory``, default ``imageio.get_writer``)."""
from __future__ import annotations

import functools
import logging
import os
from typing import Callable, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from ._patch import Seam

logger = logging.getLogger()

RGB, GRAY, DEPTH, OVER_GREEN, LIDAR_ON_IMAGE = range(5)      # include/bds.h BDS_VIDEO_*
SRC0_BYTES, SRC1_BYTES = 1, 2
MAX_EXTENT = 2 ** 31 - 1                                     # Hc Wc 3 of one canvas, h w 3 of one source


# ----------------------------------------------------------------------------------------------------------------------------------
# the layouts
# ----------------------------------------------------------------------------------------------------------------------------------
class Rect(NamedTuple):
    """Image ``index`` of the camera list at (``y``, ``x``) of the cropped canvas, ``h`` x ``w`` pixels from source row ``row0``."""
    index: int
    y: int
    x: int
    h: int
    w: int
    row0: int


class Plan(NamedTuple):
    height: int
    width: int
    rects: Tuple[Rect, ...]      # in ``cam_names`` order: where two overlap, the later one is on top


_GRIDS = {
    "nuscenes": (("CAM_FRONT_LEFT", "CAM_FRONT", "CAM_FRONT_RIGHT"), ("CAM_BACK_LEFT", "CAM_BACK", "CAM_BACK_RIGHT")),
    "pandaset": (("front_left_camera", "front_camera", "front_right_camera"), ("left_camera", "back_camera", "right_camera")),
    "nuplan": (("CAM_L0", "CAM_F0", "CAM_R0"), ("CAM_L1", None, "CAM_R1"), ("CAM_L2", "CAM_B0", "CAM_R2")),
}
_WAYMO = ("left_camera", "front_left_camera", "front_camera", "front_right_camera", "right_camera")


def _slots(dataset_type: str, cam_names: Sequence[str], sizes: Sequence[Tuple[int, int]]):
    """(canvas height, canvas width, [(index, row slice, column slice, source rows shown)], keep the last filled row and column)."""
    s = slice
    known = [(i, n) for i, n in enumerate(cam_names)]
    if dataset_type == "waymo":
        if "front_camera" not in cam_names:
            raise ValueError("'front_camera' is not in list")
        lh, lw = sizes[cam_names.index("front_camera")]
        slots = []
        for i, n in known:
            if n in _WAYMO:
                c = _WAYMO.index(n)
                rows = s(lh - sizes[i][0], None) if n in ("left_camera", "right_camera") else s(None)
                slots.append((i, rows, s(c * lw, (c + 1) * lw if c < 4 else None), sizes[i][0]))
        return lh, 5 * lw, slots, False
    if dataset_type in _GRIDS:
        grid = _GRIDS[dataset_type]
        if dataset_type == "nuplan":
            lh, lw = sizes[0]
        else:
            lw, lh = max(sizes[0]), min(sizes[0])
        R, C = len(grid), len(grid[0])
        at = {n: (r, c) for r, row in enumerate(grid) for c, n in enumerate(row) if n is not None}
        slots = []
        for i, n in known:
            if n in at:
                r, c = at[n]
                slots.append((i, s(r * lh, (r + 1) * lh if r < R - 1 else None), s(c * lw, (c + 1) * lw if c < C - 1 else None), sizes[i][0]))
        return R * lh, C * lw, slots, dataset_type == "nuplan"
    if dataset_type == "kitti":
        lh, lw = sizes[0]
        slots = []
        for i, n in known:
            if n == "CAM_LEFT":
                slots.append((i, s(None), s(None, sizes[i][1]), sizes[i][0]))
            elif n == "CAM_RIGHT":
                slots.append((i, s(None), s(sizes[i][1], None), sizes[i][0]))
        return lh, 2 * lw, slots, False
    if dataset_type == "argoverse":
        lw, lh = max(sizes[0]), min(sizes[0])
        place = {"ring_front_left": (s(None, lh), s(None, lw)), "ring_front_center": (s(None, lh), s(lw, lw + lh)),
                 "ring_front_right": (s(None, lh), s(lw + lh, None)), "ring_side_left": (s(lh, 2 * lh), s(None, lw)),
                 "ring_side_right": (s(lh, 2 * lh), s(lw + lh, None)),
                 "ring_rear_left": (s(2 * lh, 3 * lh), s(int(0.5 * lh), int(lw + 0.5 * lh))),
                 "ring_rear_right": (s(2 * lh, 3 * lh), s(int(lw + 0.5 * lh), int(2 * lw + 0.5 * lh)))}
        slots = []
        for i, n in known:
            if n in place:
                shown = min(lh, sizes[i][0]) if n == "ring_front_center" else sizes[i][0]      # img[:landscape_height, :]
                slots.append((i, place[n][0], place[n][1], shown))
        return 3 * lh, 2 * lw + lh, slots, False
    raise ValueError(f"dataset_type {dataset_type} not supported")


@functools.lru_cache(maxsize=512)
def _plan(dataset_type: str, cam_names: Tuple[str, ...], sizes: Tuple[Tuple[int, int], ...]) -> Plan:
    if len(sizes) < len(cam_names):
        raise IndexError(f"{len(cam_names)} camera names for {len(sizes)} images")
    Hc, Wc, slots, keep_last = _slots(dataset_type, cam_names, sizes)
    boxes = []
    for i, rows, cols, shown in slots:
        y0, y1, _ = rows.indices(Hc)
        x0, x1, _ = cols.indices(Wc)
        if (max(y1 - y0, 0), max(x1 - x0, 0)) != (shown, sizes[i][1]):
            raise ValueError(f"could not place image {i} ({cam_names[i]}) of {sizes[i]} into a slot of {(max(y1 - y0, 0), max(x1 - x0, 0))}")
        if y1 > y0 and x1 > x0:
            boxes.append((i, y0, y1, x0, x1))
    if not boxes:
        raise ValueError("no camera of the list fills a panel of the layout")
    last = 1 if keep_last else 0
    top, left = min(b[1] for b in boxes), min(b[3] for b in boxes)
    bottom, right = max(b[2] for b in boxes) - 1 + last, max(b[4] for b in boxes) - 1 + last      # the crop's end, exclusive
    rects = tuple(Rect(i, y0 - top, x0 - left, max(min(y1, bottom) - y0, 0), max(min(x1, right) - x0, 0), 0) for i, y0, y1, x0, x1 in boxes)
    return Plan(bottom - top, right - left, rects)


def plan_layout(dataset_type: str, cam_names: Sequence[str], sizes: Sequence[Tuple[int, int]]) -> Plan:
    """``layout_<dataset_type>(imgs, cam_names)`` of utils/visualization.py:41-341 for images of ``sizes`` [(h, w)] as rectangles of
    the cropped canvas.  Cached per (type, names, sizes).  ValueError where the reference raises one, IndexError for fewer images than
    names."""
    return _plan(str(dataset_type), tuple(cam_names), tuple((int(h), int(w)) for h, w in sizes))


# ----------------------------------------------------------------------------------------------------------------------------------
# one launch
# ----------------------------------------------------------------------------------------------------------------------------------
class Panel(NamedTuple):
    kind: int
    src0: Tensor               # [h,w,3] float32 (RGB, OVER_GREEN, LIDAR_ON_IMAGE), [h,w] float32 or bytes (GRAY), [h,w] float32 (DEPTH)
    src1: Optional[Tensor]     # [h,w]: DEPTH's weight (float32, bytes or None), OVER_GREEN's opacity, LIDAR_ON_IMAGE's depth map
    rect: Rect


_BYTES = (torch.uint8, torch.bool)


def _source(x, device, channels: int, bytes_ok: bool = False) -> Tensor:
    """``x`` (a tensor, or a numpy array that is uploaded) as a contiguous [h,w,3] or [h,w] tensor the kernel reads: float32, or bytes
    where ``bytes_ok``.  [h,w,1] counts as [h,w]."""
    if not isinstance(x, Tensor):
        a = np.asarray(x)
        if a.dtype == np.float64 or not (a.dtype == np.float32 or (bytes_ok and a.dtype in (np.bool_, np.uint8))):
            a = a.astype(np.float32)
        x = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    x = x.detach()
    if channels == 1 and x.dim() == 3 and x.shape[-1] == 1:
        x = x[..., 0]
    if x.dim() != (3 if channels == 3 else 2) or (channels == 3 and x.shape[-1] != 3):
        raise ValueError(f"expected {'[h,w,3]' if channels == 3 else '[h,w] or [h,w,1]'}, got {tuple(x.shape)}")
    if x.dtype in _BYTES and bytes_ok:
        return (x.view(torch.uint8) if x.dtype == torch.bool else x).contiguous()
    return L.f32c(x)


def _panel(kind: int, a, b, device, rect: Optional[Rect] = None, index: int = 0) -> Panel:
    src0 = _source(a, device, 1 if kind in (GRAY, DEPTH) else 3, bytes_ok=kind == GRAY)
    src1 = None
    if kind in (OVER_GREEN, LIDAR_ON_IMAGE) or (kind == DEPTH and b is not None):
        if b is None:
            raise ValueError("the panel's second source is missing")
        src1 = _source(b, device, 1, bytes_ok=kind == DEPTH)
        if tuple(src1.shape) != tuple(src0.shape[:2]):
            raise ValueError(f"the panel's sources differ in size: {tuple(src0.shape[:2])} and {tuple(src1.shape)}")
    h, w = int(src0.shape[0]), int(src0.shape[1])
    return Panel(kind, src0, src1, Rect(index, 0, 0, h, w, 0) if rect is None else rect)


def _launch(panels: Sequence[Panel], Hc: int, Wc: int, device) -> Tensor:
    """The canvas [Hc,Wc,3] uint8 of ``panels``: one call into the library, no host wait.  BdsError for a CPU tensor."""
    if Hc * Wc * 3 > MAX_EXTENT:
        raise ValueError(f"one canvas holds Hc*Wc*3 <= {MAX_EXTENT} bytes, got {Hc} x {Wc}")
    tensors = [t for p in panels for t in (p.src0, p.src1)]
    L.require_gpu(*tensors)
    if tensors:
        device = tensors[0].device
    canvas = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=device)
    L.require_gpu(canvas)
    table = (L.BdsVideoPanel * max(len(panels), 1))()
    for t, p in zip(table, panels):
        t.src0, t.src1 = L.ptr(p.src0), L.ptr(p.src1)
        t.kind = p.kind
        t.flags = (SRC0_BYTES if p.src0.dtype == torch.uint8 else 0) | (SRC1_BYTES if p.src1 is not None and p.src1.dtype == torch.uint8 else 0)
        t.src_h, t.src_w, t.src_row0 = int(p.src0.shape[0]), int(p.src0.shape[1]), p.rect.row0
        t.dst_y, t.dst_x, t.dst_h, t.dst_w = p.rect.y, p.rect.x, p.rect.h, p.rect.w
    L.check(L.lib().bds_video_frame(len(panels), table, Hc, Wc, L.ptr(canvas), L.stream()), "bds_video_frame")
    return canvas


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


def _one(kind: int, a, b=None) -> Tensor:
    device = next((t.device for t in (a, b) if isinstance(t, Tensor)), None) or _default_device()
    p = _panel(kind, a, b, device)
    return _launch([p], p.rect.h, p.rect.w, device)


@torch.no_grad()
def to8b(x) -> Tensor:
    """visualization.py:19-22 on a device tensor [h,w,3], [h,w] or [h,w,1]: ``(255 * clip(x, 0, 1))`` truncated to uint8, in ``x``'s
    shape.  A NaN gives 0."""
    if getattr(x, "ndim", 0) == 3 and x.shape[-1] == 3:
        return _one(RGB, x)
    return _one(GRAY, x)[..., 0].reshape(tuple(x.shape))


@torch.no_grad()
def depth_visualizer(frame, opacity=None) -> Tensor:
    """``to8b(depth_visualizer(frame, opacity))`` of visualization.py:491-497 as [h,w,3] uint8: turbo over -log(depth + 1e-6) scaled
    between lo = 4 and hi = 120, times the opacity (float32 or bool; None: 1)."""
    return _one(DEPTH, frame, opacity)


@torch.no_grad()
def over_green(rgb, opacity) -> Tensor:
    """The per-class composite of video_utils.py:201-227 behind the clamp of :185-187, quantised: [h,w,3] uint8."""
    return _one(OVER_GREEN, rgb, opacity)


@torch.no_grad()
def lidar_on_image(pixels, depth_map) -> Tensor:
    """video_utils.py:265-271, quantised: the lidar depth's colour where the map is > 0, else the pixel; [h,w,3] uint8."""
    return _one(LIDAR_ON_IMAGE, pixels, depth_map)


# ----------------------------------------------------------------------------------------------------------------------------------
# the keys
# ----------------------------------------------------------------------------------------------------------------------------------
def _present(render_results: Mapping[str, Sequence], key: str) -> bool:
    return key in render_results and len(render_results[key]) != 0


def key_sources(render_results: Mapping[str, Sequence], key: str, at: slice) -> Optional[List[tuple]]:
    """One key of the views ``at`` as the reference prepares it for the layout (video_utils.py:723-756): [(kind, first source, second
    source or None)] per camera, or None where the reference skips the key."""
    if "mask" in key:
        new_key = key.replace("mask", "opacities")
        if not _present(render_results, new_key):
            return None
        return [(GRAY, f, None) for f in render_results[new_key][at]]
    if not _present(render_results, key):
        return None
    frames = render_results[key][at]
    if "depth" in key:
        name = key.replace("depths", "opacities")
        if name not in render_results:
            if "median" not in key:
                return None
            name = key.replace("median_depths", "opacities")      # (KeyError where that is missing too, as the reference)
        return [(DEPTH, f, o) for f, o in zip(frames, render_results[name][at])]
    return [(RGB, f, None) for f in frames]


def _size(x) -> Tuple[int, int]:
    return int(x.shape[0]), int(x.shape[1])


class FrameComposer:
    """The frames of one dataset type's videos.  ``keys``: the rows of a merged frame, top to bottom."""

    def __init__(self, dataset_type: str, keys: Sequence[str] = ("gt_rgbs", "rgbs", "depths"), device=None):
        self.dataset_type, self.keys, self.device = str(dataset_type), list(keys), device

    def _device(self, sources) -> torch.device:
        if self.device is not None:
            return torch.device(self.device)
        return next((t.device for s in sources for t in s[1:] if isinstance(t, Tensor)), None) or _default_device()

    def _key(self, key: str, render_results, cam_names: Sequence[str], first: int):
        """(plan, sources) of one key, or None where it is skipped."""
        sources = key_sources(render_results, key, slice(first, first + len(cam_names)))
        if sources is None:
            return None
        if len(sources) == 0:
            raise IndexError("list index out of range")      # (the reference's imgs[0])
        return plan_layout(self.dataset_type, cam_names, [_size(s[1]) for s in sources]), sources

    def _panels(self, plan: Plan, sources, device, top: int) -> List[Panel]:
        return [_panel(sources[r.index][0], sources[r.index][1], sources[r.index][2], device, r._replace(y=r.y + top))
                for r in plan.rects if r.h > 0 and r.w > 0]

    @torch.no_grad()
    def key_frame(self, key: str, render_results, cam_names: Sequence[str], first: int = 0) -> Optional[Tensor]:
        """One key's canvas [Hc,Wc,3] uint8 of the views ``first .. first + len(cam_names)`` of the lists, or None where the key is
        skipped."""
        got = self._key(key, render_results, list(cam_names), first)
        if got is None:
            return None
        plan, sources = got
        device = self._device(sources)
        return _launch(self._panels(plan, sources, device, 0), plan.height, plan.width, device)

    @torch.no_grad()
    def frame(self, render_results, cam_names: Sequence[str], first: int = 0) -> Tensor:
        """The merged canvas of one timestep: the keys' canvases stacked vertically as ``np.concatenate(merged_list, axis=0)`` does, in
        one launch.  ValueError where no key is left or the keys' canvases differ in width."""
        rows = [r for r in (self._key(k, render_results, list(cam_names), first) for k in self.keys) if r is not None]
        if not rows:
            raise ValueError("need at least one array to concatenate")
        width = rows[0][0].width
        if any(plan.width != width for plan, _ in rows):
            raise ValueError(f"the keys' canvases differ in width: {[plan.width for plan, _ in rows]}")
        device = self._device([s for _, sources in rows for s in sources])
        panels, top = [], 0
        for plan, sources in rows:
            panels += self._panels(plan, sources, device, top)
            top += plan.height
        return _launch(panels, top, width, device)


def _dataset_type(layout: Union[str, Callable]) -> str:
    """The dataset type of the reference's ``layout`` argument: one of its ``layout_<type>`` functions, or the type's name."""
    name = layout if isinstance(layout, str) else getattr(layout, "__name__", "")
    name = name[len("layout_"):] if name.startswith("layout_") else name
    if name not in ("waymo", "pandaset", "argoverse", "nuscenes", "kitti", "nuplan"):
        raise ValueError(f"layout {layout!r} is none of the reference's layout_<dataset type> functions")
    return name


def _get_writer(writer_factory):
    if writer_factory is not None:
        return writer_factory
    import imageio
    return imageio.get_writer


def _host(canvas: Tensor) -> np.ndarray:
    return canvas.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------------------
# the reference's two functions
# ----------------------------------------------------------------------------------------------------------------------------------
def _open(get_writer, path: str, num_timestamps: int, fps: int):
    """A writer for ``path``: a single timestep is an image and takes no frame rate."""
    return get_writer(path, mode="I") if num_timestamps == 1 else get_writer(path, mode="I", fps=fps)


def _keyed(path: str, key: str, tail: Optional[str] = None) -> str:
    """``path`` with ``_<key>`` in front of its ``.mp4`` or ``.png`` suffix; ``tail``: what then stands in place of ``.mp4``."""
    path = path.replace(".mp4", f"_{key}.mp4").replace(".png", f"_{key}.png")
    return path if tail is None else path.replace(".mp4", tail)


@torch.no_grad()
def save_concatenated_videos(render_results, save_pth: str, layout, num_timestamps: int, keys: List[str] = ["gt_rgbs", "rgbs", "depths"],
                             num_cams: int = 3, save_images: bool = False, fps: int = 10, verbose: bool = True, writer_factory=None):
    """video_utils.py:703-768: one merged frame per timestep, written to ``save_pth``; returns ``{"concatenated_frame": the middle
    timestep's frame}`` (uint8 numpy; the only frame where there is one timestep).  ``layout``: the reference's ``layout_<type>``
    function or the type's name.  ``save_images`` is accepted and, as in the reference, unused."""
    composer = FrameComposer(_dataset_type(layout), keys)
    writer = _open(_get_writer(writer_factory), save_pth, num_timestamps, fps)
    middle = 0 if num_timestamps == 1 else num_timestamps // 2
    kept = None
    for step in range(num_timestamps):
        first = step * num_cams
        frame = _host(composer.frame(render_results, render_results["cam_names"][first:first + num_cams], first))
        writer.append_data(frame)
        if step == middle:
            kept = frame
    writer.close()
    if verbose:
        logger.info(f"saved video to {save_pth}")
    return {"concatenated_frame": kept}


@torch.no_grad()
def save_seperate_videos(render_results, save_pth: str, layout, num_timestamps: int, keys: List[str] = ["gt_rgbs", "rgbs", "depths"],
                         num_cams: int = 3, fps: int = 10, verbose: bool = False, save_images: bool = False, writer_factory=None,
                         image_writer=None):
    """video_utils.py:771-857: one video per key at ``save_pth`` with ``_<key>`` before its suffix; returns {key: the middle
    timestep's frame}.  As in the reference a writer is created for every key, and the writer of a key whose list is absent or empty
    (other than a ``mask`` key) is left as it was opened.  ``save_images``: per camera the raw depth maps as ``.npy`` and every key's
    quantised image as PNG (``image_writer``, default ``imageio.imwrite``)."""
    dataset_type = _dataset_type(layout)
    get_writer = _get_writer(writer_factory)
    kept = {}
    for key in keys:
        path = _keyed(save_pth, key)
        writer = _open(get_writer, path, num_timestamps, fps)
        if "mask" not in key and not _present(render_results, key):
            continue
        composer = FrameComposer(dataset_type, [key])
        for step in range(num_timestamps):
            first = step * num_cams
            canvas = composer.key_frame(key, render_results, render_results["cam_names"][first:first + num_cams], first)
            if canvas is None:
                continue
            if save_images:
                _save_images(render_results, key, slice(first, first + num_cams), save_pth, step, image_writer)
            frame = _host(canvas)
            writer.append_data(frame)
            if step == num_timestamps // 2:
                kept[key] = frame
        writer.close()
        if verbose:
            logger.info(f"saved video to {path}")
    return kept


def _save_images(render_results, key: str, at: slice, save_pth: str, step: int, image_writer) -> None:
    """video_utils.py:825-845: one key's views of one timestep as files ``<step>_<camera>``, three digits each: the raw depth maps
    as [h,w] ``.npy`` under ``<video>_np/``, every view's quantised image as PNG under ``<video>/``."""
    if image_writer is None:
        import imageio
        image_writer = imageio.imwrite
    if "depth" in key and "mask" not in key:
        os.makedirs(_keyed(save_pth, key, "_np"), exist_ok=True)
        for cam, depth in enumerate(render_results[key][at]):
            raw = depth.detach().cpu().numpy() if isinstance(depth, Tensor) else np.asarray(depth)
            raw = raw[..., 0] if raw.ndim == 3 and raw.shape[-1] == 1 else raw      # (the reference's lists hold squeezed maps)
            np.save(_keyed(save_pth, key, f"_np/{step:03d}_{cam:03d}.npy"), raw)
    os.makedirs(_keyed(save_pth, key, ""), exist_ok=True)
    for cam, (kind, a, b) in enumerate(key_sources(render_results, key, at)):
        image_writer(_keyed(save_pth, key, f"/{step:03d}_{cam:03d}.png"), _host(_one(kind, a, b)))


# ----------------------------------------------------------------------------------------------------------------------------------
# the seam
# ----------------------------------------------------------------------------------------------------------------------------------
_SEAM = Seam()


def install(video_utils_module) -> None:
    """Sets ``save_concatenated_videos`` and ``save_seperate_videos`` on the reference's ``models.video_utils``, whose ``save_videos``
    then reaches them.  Lists of numpy arrays that the unmodified ``render`` produced still work: they are uploaded."""
    _SEAM.install(video_utils_module, {"save_concatenated_videos": save_concatenated_videos, "save_seperate_videos": save_seperate_videos})


def uninstall(*targets) -> None:
    """Puts back what ``install`` replaced (no target given: on every installed one)."""
    _SEAM.uninstall(*targets)
