"""Evaluation image metrics as one fused HIP pass (csrc/metrics.hip through ``bds_image_metrics``).

Reference: ``render_images`` scores every frame on the host (models/video_utils.py:273-361): the render and the ground truth are
copied over, ``skimage.metrics.structural_similarity`` runs on the full image up to five times (once for the scalar, four times with
``full=True`` to index the same map with the sky, dynamic, human and vehicle masks), ``compute_psnr`` (:29-44) up to five times over
boolean-indexed copies, and every value is an ``.item()``.

* ``image_metrics(rgb, gt, masks, ...)``: PSNR, SSIM and both under up to four masks, as float64 device tensors, in two launches and
  without a host wait.  The SSIM is skimage's (7x7 uniform window, sample covariance, reflected borders, cropped mean) -- NOT the
  training loss's (``losses.ssim``: 11x11 Gaussian window, VALID region); the two differ in the third decimal.
* ``compute_psnr(prediction, target)``: the reference's name and signature, a float.
* ``frame_metrics(rgb, image_infos)``: lines 273-361 under the reference's key names, floats, one read-back.
* ``MetricAccumulator``: a split's frames into one device buffer, read once by ``results()``: the reference's ``results_dict`` entries
  (``non_zero_mean`` :26-27, :542-552).

LPIPS is not covered; the geometry block (Chamfer, depth error) lives in ``geometry.py``."""
from __future__ import annotations

import math
from typing import Dict, Iterable, Mapping, Optional

import torch
from torch import Tensor

from . import _lib as L

ROW = 14             # include/bds.h BDS_IMAGE_METRICS_ROW: psnr, ssim, (psnr, ssim) x 4 slots, valid x 4 slots
SLOTS = 4
MIN_SIDE = 7         # the window; skimage raises below it too
MAX_SIDE = 1 << 19   # include/bds.h: the largest extent bds_image_metrics takes
# (results key prefix, image_infos key, score the complement): video_utils.py:291-361
FRAME_MASKS = (("occupied", "sky_masks", True), ("masked", "dynamic_masks", False), ("human", "human_masks", False),
               ("vehicle", "vehicle_masks", False))
RESULT_KEYS = ("psnr", "ssim") + tuple(f"{p}_{m}" for p, _, _ in FRAME_MASKS for m in ("psnr", "ssim"))


def _image(t: Tensor, what: str) -> Tensor:
    if t.dim() != 3 or t.shape[-1] != 3:
        raise ValueError(f"{what} must be [H,W,3], got {tuple(t.shape)}")
    return t.detach().contiguous().float()


def _mask_kind(m: Tensor) -> int:
    return 1 if m.dtype == torch.float32 else (0 if m.dtype in (torch.bool, torch.uint8) else -1)


def grown(ws: Optional[Tensor], need: int, device) -> Tensor:
    """``ws`` where it holds ``need`` bytes, else a new uint8 buffer that does (never empty: the entries take no NULL workspace)."""
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    return ws


def _launch(rgb: Tensor, gt: Tensor, masks: list, invert_bits: int, row: Tensor, ssim_map: Optional[Tensor],
            ws: Optional[Tensor] = None) -> None:
    """``masks``: up to four [H,W] tensors or None per slot; ``row``: [ROW] float64, contiguous."""
    H, W = rgb.shape[:2]
    for m in masks:
        if m is not None and tuple(m.shape) != (H, W):
            raise ValueError(f"mask must be [H,W] = {(H, W)}, got {tuple(m.shape)}")
    L.require_gpu(rgb, gt, row, ssim_map, *masks)
    kinds = {_mask_kind(m) for m in masks if m is not None}
    if len(kinds) > 1 or -1 in kinds:       # mixed or other element types: one byte per pixel, non-zero = true
        masks = [None if m is None else (m if _mask_kind(m) == 0 else (m != 0)) for m in masks]
        kinds = {0}
    held = [None if m is None else m.detach().contiguous() for m in masks]      # (alive until the launches are enqueued)
    ptrs = [L.ptr(m) for m in held] + [None] * (SLOTS - len(held))
    lib = L.lib()
    ws = grown(ws, int(lib.bds_image_metrics_workspace_bytes(H, W)), rgb.device)
    L.check(lib.bds_image_metrics(H, W, L.ptr(rgb), L.ptr(gt), *ptrs, invert_bits, kinds.pop() if kinds else 0, L.ptr(ssim_map),
                                  L.ptr(row), L.ptr(ws), ws.numel(), L.stream()), "bds_image_metrics")


@torch.no_grad()
def image_metrics(rgb: Tensor, gt: Tensor, masks: Optional[Mapping[str, Tensor]] = None, return_map: bool = False,
                  invert: Iterable[str] = ()) -> Dict[str, Tensor]:
    """``rgb``, ``gt`` [H,W,3]; ``masks``: up to four names -> [H,W] bool, uint8 or float tensors (non-zero = true); a name in
    ``invert`` scores the pixels where its mask is false.  Returns 0-dim float64 device tensors ``psnr``, ``ssim`` and per mask
    ``<name>_psnr``, ``<name>_ssim`` (NaN for an empty mask) and ``<name>_valid`` (1.0 / 0.0); with ``return_map`` also ``ssim_map``
    [H,W,3] float32, skimage's ``full=True``.  A masked SSIM is the mean of the uncropped map over the mask, as ``S[mask].mean()``."""
    rgb, gt = _image(rgb, "rgb"), _image(gt, "gt")
    if rgb.shape != gt.shape:
        raise ValueError(f"rgb {tuple(rgb.shape)} and gt {tuple(gt.shape)} must have the same shape")
    if min(rgb.shape[:2]) < MIN_SIDE:
        raise ValueError(f"the {MIN_SIDE}x{MIN_SIDE} window exceeds the image extent {tuple(rgb.shape[:2])}")
    masks = dict(masks or {})
    if len(masks) > SLOTS:
        raise ValueError(f"at most {SLOTS} masks per call, got {len(masks)}")
    invert = set(invert)
    if not invert <= set(masks):
        raise ValueError(f"invert names no mask: {sorted(invert - set(masks))}")
    row = torch.empty(ROW, dtype=torch.float64, device=rgb.device)
    smap = torch.empty_like(rgb) if return_map else None
    bits = sum(1 << s for s, name in enumerate(masks) if name in invert)
    _launch(rgb, gt, list(masks.values()), bits, row, smap)
    out = {"psnr": row[0], "ssim": row[1]}
    for s, name in enumerate(masks):
        out[f"{name}_psnr"], out[f"{name}_ssim"], out[f"{name}_valid"] = row[2 + 2 * s], row[3 + 2 * s], row[2 + 2 * SLOTS + s]
    if return_map:
        out["ssim_map"] = smap
    return out


def compute_psnr(prediction: Tensor, target: Tensor) -> float:
    """video_utils.py:29-44: ``-10 log10(mse)`` over all elements of two tensors of one shape (an image, or ``image[mask]``).  It goes
    through the frame pass (there is no separate PSNR kernel): a tensor that is not an [H,W,3] image the pass takes is laid out as a
    zero-padded [h,w,3] one, which limits it to 2^19 * 4096 * 3 elements."""
    if not isinstance(prediction, Tensor):
        prediction = torch.as_tensor(prediction, dtype=torch.float32)
    if not isinstance(target, Tensor):
        target = torch.as_tensor(target, dtype=torch.float32).to(prediction.device)
    if prediction.shape != target.shape or prediction.numel() == 0:
        raise ValueError(f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)} must have one non-empty shape")
    L.require_gpu(prediction, target)
    p, t = prediction.detach().float(), target.detach().float()
    n = p.numel()
    if p.dim() != 3 or p.shape[-1] != 3 or min(p.shape[:2]) < MIN_SIDE or max(p.shape[:2]) > MAX_SIDE:
        # the squared error does not depend on the elements' arrangement: [h,w,3] with zero padding, which adds nothing to it
        w = MIN_SIDE if n <= MIN_SIDE * 3 * 4096 else 4096
        h = max(-(-n // (w * 3)), MIN_SIDE)
        if h > MAX_SIDE:
            raise ValueError(f"compute_psnr takes at most {MAX_SIDE * 4096 * 3} elements, got {n}")
        p, t = (torch.nn.functional.pad(x.reshape(-1), (0, h * w * 3 - n)).reshape(h, w, 3) for x in (p, t))
    row = torch.empty(ROW, dtype=torch.float64, device=p.device)
    _launch(p.contiguous(), t.contiguous(), [], 0, row, None)
    return float(row[0].item()) - 10.0 * math.log10(p.numel() / n)      # (the kernel divided by the padded count)


def _frame_inputs(rgb: Tensor, image_infos: Mapping[str, Tensor]):
    """get_numpy's squeeze on the render, the ground truth and the masks present; (rgb, gt, [mask or None] * 4, invert bits)."""
    rgb, gt = rgb.squeeze(), image_infos["pixels"].squeeze()
    masks = [image_infos[key].squeeze() if key in image_infos else None for _, key, _ in FRAME_MASKS]
    bits = sum(1 << s for s, (_, _, inv) in enumerate(FRAME_MASKS) if inv and masks[s] is not None)
    rgb, gt = _image(rgb, "rgb"), _image(gt, "image_infos['pixels']")
    if rgb.shape != gt.shape:
        raise ValueError(f"rgb {tuple(rgb.shape)} and pixels {tuple(gt.shape)} must have the same shape")
    if min(rgb.shape[:2]) < MIN_SIDE:
        raise ValueError(f"the {MIN_SIDE}x{MIN_SIDE} window exceeds the image extent {tuple(rgb.shape[:2])}")
    return rgb, gt, masks, bits


def _row_to_dict(vals, present) -> Dict[str, float]:
    out = {"psnr": vals[0], "ssim": vals[1]}
    for s, (prefix, _, _) in enumerate(FRAME_MASKS):
        if present[s] and vals[2 + 2 * SLOTS + s] > 0:
            out[f"{prefix}_psnr"], out[f"{prefix}_ssim"] = vals[2 + 2 * s], vals[3 + 2 * s]
    return out


@torch.no_grad()
def frame_metrics(rgb: Tensor, image_infos: Mapping[str, Tensor]) -> Dict[str, float]:
    """One frame's values of video_utils.py:273-361 as floats: ``psnr``, ``ssim`` and, for every mask key of ``image_infos`` that is
    present and scores at least one pixel, ``occupied_*`` (~sky_masks), ``masked_*`` (dynamic_masks), ``human_*``, ``vehicle_*``."""
    rgb, gt, masks, bits = _frame_inputs(rgb, image_infos)
    row = torch.empty(ROW, dtype=torch.float64, device=rgb.device)
    _launch(rgb, gt, masks, bits, row, None)
    return _row_to_dict(row.cpu().tolist(), [m is not None for m in masks])


def non_zero_mean(x) -> float:
    return sum(x) / len(x) if len(x) > 0 else -1        # video_utils.py:26-27


class RowAccumulator:
    """What ``MetricAccumulator`` and ``geometry.GeometryAccumulator`` share: a preallocated [num_frames, ROW] float64 device buffer
    with one row per frame, and one grow-only workspace for the frames' launches."""
    ROW = 0                     # floats per frame
    WORKSPACE_BYTES = ""        # the C entry that sizes the workspace of an [H,W] frame

    def __init__(self, num_frames: int, device=None):
        """``device``: the GPU every frame lives on (default: the current one).  ``add`` must be called on ONE stream: the frames share
        a workspace, which the launches of one stream use in order."""
        dev = torch.device(device if device is not None else "cuda")
        self.rows = torch.empty(num_frames, self.ROW, dtype=torch.float64, device=dev)
        self.count = 0
        self._ws = None
        self._stream = None

    def __len__(self) -> int:
        return self.count

    def _require_room(self) -> None:
        if self.count >= self.rows.shape[0]:
            raise IndexError(f"{type(self).__name__} holds {self.rows.shape[0]} frames")

    def _next(self, H: int, W: int, *frame: Tensor):
        """(the row of the next frame, the workspace) for a launch over the [H,W] tensors ``frame``; the caller counts the frame."""
        L.require_gpu(*frame, self.rows)           # (one device: the frame's and the buffer's)
        stream = L.stream()
        if self._stream is None:
            self._stream = stream
        elif stream != self._stream:
            raise L.BdsError(f"{type(self).__name__}.add was called on another stream than before: the frames share one workspace")
        self._ws = grown(self._ws, int(getattr(L.lib(), self.WORKSPACE_BYTES)(H, W)), frame[0].device)
        return self.rows[self.count], self._ws


class MetricAccumulator(RowAccumulator):
    """The scores of a split: ``add(rgb, image_infos)`` writes the next frame's row into a preallocated [num_frames, ROW] device
    buffer (no host wait); ``results()`` reads the buffer once and returns ``results_dict``'s entries (video_utils.py:542-552): per
    key the mean over the frames that produced it, -1 where none did."""
    ROW, WORKSPACE_BYTES = ROW, "bds_image_metrics_workspace_bytes"

    def __init__(self, num_frames: int, device=None):
        super().__init__(num_frames, device)
        self.present = []        # per frame: which mask keys image_infos had (host knowledge, no read-back)

    @torch.no_grad()
    def add(self, rgb: Tensor, image_infos: Mapping[str, Tensor]) -> None:
        self._require_room()
        rgb, gt, masks, bits = _frame_inputs(rgb, image_infos)
        row, ws = self._next(*rgb.shape[:2], rgb, gt)
        _launch(rgb, gt, masks, bits, row, None, ws)
        self.present.append([m is not None for m in masks])
        self.count += 1

    def per_frame(self):
        """[{key: float}] of the frames added so far, the keys ``frame_metrics`` gives (one read-back)."""
        vals = self.rows[:self.count].cpu().tolist()
        return [_row_to_dict(v, p) for v, p in zip(vals, self.present)]

    def results(self) -> Dict[str, float]:
        frames = self.per_frame()
        return {k: non_zero_mean([f[k] for f in frames if k in f]) for k in RESULT_KEYS}
