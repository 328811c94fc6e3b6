"""Numpy restatement of the evaluation video frames (bilateral_driving_amd/video.py, csrc/video.hip) and the inputs that the golden
generator (scripts/gen_golden_video.py), the CPU tests and the GPU tests share.  Test infrastructure: nothing here is loaded by the
product, and nothing here reads the reference tree.

The restatement follows the reference's expressions (utils/visualization.py:19-22, 41-341, 412-497; models/video_utils.py:201-227,
265-271, 703-857) in two modes: ``np.float32`` rounds every operation to float32 as csrc/video_math.h does, ``np.float64`` evaluates the
same formula in float64 from the float32 inputs.  tests/test_video_cpu.py pins it to the reference's recorded results
(tests/golden/video_frames.npz).

The depth rule (``depth_rule``).  The device's logf and numpy's differ in the last place, so a depth pixel may differ from the float64
restatement, but only by exactly one table index and only where the float64 value t = 256 s lies within 2^-10 of an integer: about six
float32 roundings on magnitudes <= 13.8, divided by 3.4 and multiplied by 256, move t by at most 3.7e-4 < 2^-10.  At most 0.1 % of a
case's depth pixels may differ (none in a case of fewer than 1000); every other pixel is bit-equal."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "video_frames.npz")
BAND = 2.0 ** -10
MAX_SHARE = 1e-3
LO, HI = -np.log(4.0 + 1e-6), -np.log(120 + 1e-6)      # depth_visualizer's lo = 4 and hi = 120 behind its curve, in float64
GREEN = np.float32([0.0, 177.0, 64.0]) / np.float32(255.0)
BAD = -1

# ---- the layouts' cameras: every camera, a three-camera subset, one camera ------------------------------------------------------------
CAMS = {
    "waymo": ["left_camera", "front_left_camera", "front_camera", "front_right_camera", "right_camera"],
    "pandaset": ["front_left_camera", "front_camera", "front_right_camera", "left_camera", "back_camera", "right_camera"],
    "argoverse": ["ring_front_left", "ring_front_center", "ring_front_right", "ring_side_left", "ring_side_right", "ring_rear_left",
                  "ring_rear_right"],
    "nuscenes": ["CAM_FRONT_LEFT", "CAM_FRONT", "CAM_FRONT_RIGHT", "CAM_BACK_LEFT", "CAM_BACK", "CAM_BACK_RIGHT"],
    "kitti": ["CAM_LEFT", "CAM_RIGHT"],
    "nuplan": ["CAM_L0", "CAM_F0", "CAM_R0", "CAM_L1", "CAM_R1", "CAM_L2", "CAM_B0", "CAM_R2"],
}
SUBSETS = {
    "waymo": (["front_camera", "front_left_camera", "front_right_camera"], ["front_camera"]),
    "pandaset": (["front_camera", "left_camera", "right_camera"], ["back_camera"]),
    "argoverse": (["ring_front_left", "ring_rear_left", "ring_rear_right"], ["ring_side_right"]),
    "nuscenes": (["CAM_FRONT", "CAM_BACK_LEFT", "CAM_BACK_RIGHT"], ["CAM_BACK"]),
    "kitti": (["CAM_RIGHT", "CAM_LEFT", "CAM_UNKNOWN"], ["CAM_RIGHT"]),
    "nuplan": (["CAM_F0", "CAM_L1", "CAM_B0"], ["CAM_R1"]),
}
H, W = 4, 6                   # the layouts' images
WAYMO_SIDE_H = 3              # a shorter waymo side camera: bottom-aligned
MERGED_KEYS = ["gt_rgbs", "rgbs", "depths", "Dynamic_depths", "RigidNodes_mask", "gt_sky_masks"]
MERGED = {"waymo": ["front_left_camera", "front_camera", "front_right_camera"], "nuscenes": CAMS["nuscenes"]}
MERGED_T = 3
ERRORS = (("waymo", ["left_camera", "right_camera"], [(4, 6), (4, 6)]),          # no front camera: list.index raises
          ("nuscenes", ["CAM_SIDE"], [(4, 6)]),                                  # no panel filled
          ("nuscenes", ["CAM_FRONT", "CAM_BACK"], [(4, 6), (5, 6)]),             # an image that does not fit its slot
          ("kitti", ["CAM_LEFT", "CAM_RIGHT"], [(4, 6), (4, 7)]),
          ("argoverse", ["ring_front_left", "ring_front_center"], [(4, 6), (3, 4)]))


def size_of(dataset_type, name, short_sides=False):
    """(h, w) of camera ``name``'s image in the layout cases: argoverse's centre camera is portrait, waymo's side cameras may be short."""
    if dataset_type == "argoverse" and name == "ring_front_center":
        return (W, H)
    if dataset_type == "waymo" and short_sides and name in ("left_camera", "right_camera"):
        return (WAYMO_SIDE_H, W)
    return (H, W)


def layout_cases():
    """[(label, dataset type, camera names, sizes)] of the recorded layout canvases."""
    out = []
    for t, full in CAMS.items():
        three, one = SUBSETS[t]
        for tag, names in (("full", full), ("three", three), ("one", one)):
            out.append((f"{t}_{tag}", t, list(names), [size_of(t, n) for n in names]))
    out.append(("waymo_short", "waymo", list(CAMS["waymo"]), [size_of("waymo", n, True) for n in CAMS["waymo"]]))
    out.append(("argoverse_rear", "argoverse", ["ring_rear_left", "ring_rear_right"], [(H, W), (H, W)]))
    out.append(("argoverse_rear_swapped", "argoverse", ["ring_rear_right", "ring_rear_left"], [(H, W), (H, W)]))
    out.append(("nuscenes_twice", "nuscenes", ["CAM_FRONT", "CAM_BACK", "CAM_FRONT"], [(H, W)] * 3))      # one slot twice: the later image wins
    return out


def constant_images(sizes):
    """One float32 [h,w,3] image per size, each filled with a constant of its own that no other image and no channel shares."""
    return [np.broadcast_to(np.float32([(3 * i + 1) / 32, (3 * i + 2) / 32, (3 * i + 3) / 32]), (h, w, 3)).copy() for i, (h, w) in enumerate(sizes)]


# ---- the formulas ---------------------------------------------------------------------------------------------------------------------
def to8b(x):
    """``to8b`` on the layouts' float32 canvas; a NaN gives 0 (the device's choice: numpy's cast of a NaN is unspecified)."""
    x = np.asarray(x).astype(np.float32)
    c = np.where(x > 0, np.minimum(x, np.float32(1)), np.float32(0))
    return (np.float32(255) * c).astype(np.uint8)


def depth_t(depth, weight, dtype):
    """t = 256 s of visualize_cmap for ``depth_visualizer`` (NaN where matplotlib shows "bad")."""
    depth = np.asarray(depth, np.float32)
    weight = np.ones(depth.shape, np.float32) if weight is None else np.asarray(weight).astype(np.float32)
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            v = -np.log(depth + np.float32(1e-6))
            s = (v - np.float32(min(LO, HI))) / np.float32(abs(HI - LO))
        else:
            v = -np.log(depth.astype(np.float64) + 1e-6)
            s = (v - min(LO, HI)) / abs(HI - LO)
        s = np.where(s > 0, np.minimum(s, dtype(1)), dtype(0)).astype(dtype)      # clip, then nan_to_num
        return (s * weight.astype(dtype)) * dtype(256)


def depth_index(depth, weight, dtype):
    t = depth_t(depth, weight, dtype)
    with np.errstate(all="ignore"):
        idx = np.where(t < 0, 0, np.where(t >= 255, 255, np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0))).astype(np.int32)
    return np.where(np.isnan(t), BAD, idx).astype(np.int32)


TURBO8 = None      # the generator sets matplotlib's table here while the golden does not exist yet


def turbo8():
    """matplotlib's ``turbo`` quantised by ``to8b``, [256,3] uint8: the golden's record of it."""
    return golden()["turbo8"] if TURBO8 is None else TURBO8


def turbo(index):
    """The table's colours [...,3] uint8 of ``index`` (BAD: black)."""
    index = np.asarray(index)
    return np.where((index == BAD)[..., None], np.uint8(0), turbo8()[np.clip(index, 0, 255)])


def depth_image(depth, weight, dtype=np.float64):
    return turbo(depth_index(depth, weight, dtype))


def over_green(rgb, op, dtype=np.float32):
    """video_utils.py:201-227 behind the clamp of :185-187, before the quantiser; ``op`` [h,w] or [h,w,1]."""
    rgb, op = np.asarray(rgb, np.float32).astype(dtype), np.asarray(op, np.float32).astype(dtype).reshape(rgb.shape[:2] + (1,))
    with np.errstate(all="ignore"):
        return (np.clip(rgb, 0, 1) * op + GREEN.astype(dtype) * (dtype(1) - op)).astype(dtype)


def lidar_on_image(pixels, depth_map, dtype=np.float64):
    """video_utils.py:265-271, quantised: the depth's colour where the map is > 0, else the pixel."""
    pixels, depth_map = np.asarray(pixels, np.float32), np.asarray(depth_map, np.float32)
    with np.errstate(all="ignore"):
        mask = depth_map > 0
    return np.where(mask[..., None], depth_image(depth_map, mask, dtype), to8b(pixels))


def _rule(got, want, shown, t, idx):
    """The depth rule of this module's docstring on one canvas: ``want`` the float64 restatement's colours, ``shown`` the pixels that
    show a depth, ``t`` and ``idx`` their float64 256 s and table index.  Outside ``shown`` every pixel is bit-equal.  Returns the
    number of differing pixels, at most 0.1 % of the shown ones (rounded down: none in a case of fewer than 1000)."""
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape, got.dtype)
    differs = np.any(got != want, axis=-1)
    assert not bool((differs & ~shown).any()), np.argwhere(differs & ~shown)[:4]
    near = np.abs(t - np.round(t)) <= BAND
    for y, x in zip(*np.nonzero(differs)):
        assert near[y, x] and idx[y, x] != BAD, (y, x, t[y, x], got[y, x])
        around = [turbo(np.int32(j)) for j in (int(idx[y, x]) - 1, int(idx[y, x]) + 1) if 0 <= j <= 255]
        assert any(np.array_equal(got[y, x], c) for c in around), (y, x, t[y, x], got[y, x])
    count = int(differs.sum())
    assert count <= int(MAX_SHARE * int(shown.sum())), (count, int(shown.sum()))
    return count


def depth_rule(got, depth, weight, shown=None):
    """``got`` [h,w,3] uint8 against the float64 restatement of ``depth_visualizer(depth, weight)`` under the rule in this module's
    docstring; ``shown`` [h,w] bool: the pixels that show the depth (default: all; the others are not compared).  Returns the number
    of differing pixels."""
    t = depth_t(depth, weight, np.float64)
    idx = depth_index(depth, weight, np.float64)
    shown = np.ones(idx.shape, bool) if shown is None else shown
    want = turbo(idx)
    return _rule(np.where(shown[..., None], got, want), want, shown, t, idx)


# ---- the layouts ----------------------------------------------------------------------------------------------------------------------
def _slots(dataset_type, imgs, cam_names):
    """(canvas height, canvas width, [(image index, rows of the canvas, columns of the canvas, image rows shown or None)], whether the
    crop keeps the last filled row and column) as utils/visualization.py:41-341 assigns them."""
    if dataset_type == "waymo":
        front = imgs[cam_names.index("front_camera")]
        lh, lw = front.shape[0], front.shape[1]
    elif dataset_type in ("kitti", "nuplan"):
        lh, lw = imgs[0].shape[0], imgs[0].shape[1]
    else:
        lw, lh = max(imgs[0].shape[:2]), min(imgs[0].shape[:2])
    s = slice
    if dataset_type == "waymo":
        col = {"left_camera": 0, "front_left_camera": 1, "front_camera": 2, "front_right_camera": 3, "right_camera": 4}
        place = {n: ((lambda img: s(lh - img.shape[0], None)) if n in ("left_camera", "right_camera") else (lambda img: s(None)),
                     (lambda img, c=c: s(c * lw, (c + 1) * lw if c < 4 else None)), None) for n, c in col.items()}
        Hc, Wc, keep_last = lh, 5 * lw, False
    elif dataset_type in ("nuscenes", "pandaset"):
        grid = ([["CAM_FRONT_LEFT", "CAM_FRONT", "CAM_FRONT_RIGHT"], ["CAM_BACK_LEFT", "CAM_BACK", "CAM_BACK_RIGHT"]] if dataset_type == "nuscenes"
                else [["front_left_camera", "front_camera", "front_right_camera"], ["left_camera", "back_camera", "right_camera"]])
        place = {n: ((lambda img, r=r: s(None, lh) if r == 0 else s(lh, None)),
                     (lambda img, c=c: s(c * lw, (c + 1) * lw if c < 2 else None)), None) for r, row in enumerate(grid) for c, n in enumerate(row)}
        Hc, Wc, keep_last = 2 * lh, 3 * lw, False
    elif dataset_type == "kitti":
        place = {"CAM_LEFT": ((lambda img: s(None)), (lambda img: s(None, img.shape[1])), None),
                 "CAM_RIGHT": ((lambda img: s(None)), (lambda img: s(img.shape[1], None)), None)}
        Hc, Wc, keep_last = lh, 2 * lw, False
    elif dataset_type == "nuplan":
        at = {"CAM_L0": (0, 0), "CAM_F0": (0, 1), "CAM_R0": (0, 2), "CAM_L1": (1, 0), "CAM_R1": (1, 2), "CAM_L2": (2, 0), "CAM_B0": (2, 1),
              "CAM_R2": (2, 2)}
        place = {n: ((lambda img, r=r: s(r * lh, (r + 1) * lh if r < 2 else None)),
                     (lambda img, c=c: s(c * lw, (c + 1) * lw if c < 2 else None)), None) for n, (r, c) in at.items()}
        Hc, Wc, keep_last = 3 * lh, 3 * lw, True
    elif dataset_type == "argoverse":
        half = int(0.5 * lh)
        place = {"ring_front_left": ((lambda img: s(None, lh)), (lambda img: s(None, lw)), None),
                 "ring_front_center": ((lambda img: s(None, lh)), (lambda img: s(lw, lw + lh)), lh),
                 "ring_front_right": ((lambda img: s(None, lh)), (lambda img: s(lw + lh, None)), None),
                 "ring_side_left": ((lambda img: s(lh, 2 * lh)), (lambda img: s(None, lw)), None),
                 "ring_side_right": ((lambda img: s(lh, 2 * lh)), (lambda img: s(lw + lh, None)), None),
                 "ring_rear_left": ((lambda img: s(2 * lh, 3 * lh)), (lambda img: s(half, int(lw + 0.5 * lh))), None),
                 "ring_rear_right": ((lambda img: s(2 * lh, 3 * lh)), (lambda img: s(int(lw + 0.5 * lh), int(2 * lw + 0.5 * lh))), None)}
        Hc, Wc, keep_last = 3 * lh, 2 * lw + lh, False
    else:
        raise ValueError(f"dataset_type {dataset_type} not supported")
    return Hc, Wc, place, keep_last


def layout(dataset_type, imgs, cam_names, dtype=np.float32):
    """``layout_<dataset_type>(imgs, cam_names)``: the float32 canvas (``dtype``: the restatement's own side channels), cropped.  ValueError where the reference raises one (numpy's
    "could not broadcast", ``list.index``, the minimum of an empty array), IndexError for fewer images than names."""
    cam_names = list(cam_names)
    Hc, Wc, place, keep_last = _slots(dataset_type, imgs, cam_names)
    canvas = np.zeros((Hc, Wc, imgs[0].shape[-1]), dtype)
    filled = np.zeros((Hc, Wc), np.uint8)
    for idx, name in enumerate(cam_names):
        img = imgs[idx]
        if name not in place:
            continue
        rows, cols, shown = place[name]
        canvas[rows(img), cols(img)] = img if shown is None else img[:shown, :]
        filled[rows(img), cols(img)] = 1
    ys, xs = np.where(filled)
    last = 1 if keep_last else 0
    return canvas[ys.min():ys.max() + last, xs.min():xs.max() + last]


# ---- the key loop of save_concatenated_videos / save_seperate_videos ----------------------------------------------------------------------
def key_frames(render_results, key, i, num_cams):
    """One key of one timestep as the reference prepares it for the layout (video_utils.py:723-756): a list of
    ("rgb", image) / ("gray", map) / ("depth", depth, opacity) per camera, or None where the reference skips the key."""
    at = slice(i * num_cams, (i + 1) * num_cams)
    if "mask" in key:
        new_key = key.replace("mask", "opacities")
        if new_key not in render_results or len(render_results[new_key]) == 0:
            return None
        return [("gray", f) for f in render_results[new_key][at]]
    if key not in render_results or len(render_results[key]) == 0:
        return None
    frames = render_results[key][at]
    if "depth" in key:
        name = key.replace("depths", "opacities")
        if name not in render_results:
            if "median" not in key:
                return None
            name = key.replace("median_depths", "opacities")
        return [("depth", f, o) for f, o in zip(frames, render_results[name][at])]
    return [("rgb", f) for f in frames]


def _panel_images(entries, dtype):
    """Per camera the quantised colours [h,w,3] uint8 and, in float64, the depth's 256 s and table index (None for other kinds)."""
    colours, depths = [], []
    for e in entries:
        shape = np.asarray(e[1]).shape[:2]
        depths.append(None)
        if e[0] == "rgb":
            colours.append(to8b(e[1]))
        elif e[0] == "gray":
            g = np.asarray(e[1]).reshape(shape)
            colours.append(to8b(np.stack([g, g, g], -1)))
        else:
            d, o = np.asarray(e[1]).reshape(shape), np.asarray(e[2]).reshape(shape)
            colours.append(depth_image(d, o, dtype))
            depths[-1] = (depth_t(d, o, np.float64), depth_index(d, o, np.float64))
    return colours, depths


def _tile_u8(dataset_type, imgs_u8, cam_names):
    """The layout of quantised images: the bytes travel through the float32 canvas as exact integers (an unfilled pixel stays 0)."""
    return layout(dataset_type, [im.astype(np.float32) for im in imgs_u8], cam_names).astype(np.uint8)


def key_canvas(dataset_type, render_results, key, i, num_cams, dtype=np.float64):
    """(canvas [Hc,Wc,3] uint8, depth pixels [Hc,Wc] bool, their float64 256 s, their float64 table index) of one key, or None.
    Quantising before the layout equals the reference's quantising after it: the layout only copies.  The three side channels are
    tiled through the same layout in float64."""
    entries = key_frames(render_results, key, i, num_cams)
    if entries is None:
        return None
    cam_names = list(render_results["cam_names"][i * num_cams:(i + 1) * num_cams])
    colours, depths = _panel_images(entries, dtype)

    def tiled(pick, fill):
        maps = [np.full(c.shape[:2], fill, np.float64) if d is None else pick(d) for c, d in zip(colours, depths)]
        return layout(dataset_type, [m.astype(np.float64)[..., None] for m in maps], cam_names, np.float64)[..., 0]
    shown = tiled(lambda d: np.ones(d[0].shape), 0.0) > 0
    t = tiled(lambda d: np.nan_to_num(d[0], nan=0.5, posinf=0.5, neginf=0.5), 0.5)      # (a "bad" pixel is never near an integer)
    idx = tiled(lambda d: d[1], BAD).astype(np.int32)
    return _tile_u8(dataset_type, colours, cam_names), shown, t, idx


def merged_frame(dataset_type, render_results, keys, i, num_cams, dtype=np.float64):
    """The frame of timestep ``i`` of ``save_concatenated_videos`` with ``key_canvas``'s side channels, stacked like the keys."""
    parts = [p for p in (key_canvas(dataset_type, render_results, k, i, num_cams, dtype) for k in keys) if p is not None]
    return tuple(np.concatenate([p[j] for p in parts], axis=0) for j in range(4))


def frame_rule(got, frame):
    """A merged frame ``got`` against ``frame`` = ``merged_frame(...)`` or ``key_canvas(...)``: bit-equal outside the depth pixels, the
    depth rule -- band, one table index, at most 0.1 % -- inside.  Returns the number of differing pixels."""
    return _rule(got, *frame)


# ---- the shared inputs ------------------------------------------------------------------------------------------------------------------
def depth_case(h=17, w=23, seed=5):
    """(depth [h,w] float32 log-uniform in [2, 200] holding 0, a negative value, NaN, 4, 120 and 1e10; opacity [h,w] float32 uniform in
    [0, 1] holding 0 and 1; a bool weight [h,w])."""
    rng = np.random.default_rng(seed)
    depth = np.exp(rng.uniform(np.log(2.0), np.log(200.0), (h, w))).astype(np.float32)
    opacity = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    special = np.float32([0.0, -3.0, np.nan, 4.0, 120.0, 1e10])
    n = min(len(special), depth.size)
    depth.reshape(-1)[:n] = special[:n]
    if opacity.size > 8:
        opacity.reshape(-1)[:n] = 1.0                     # the special depths at full weight ...
        opacity.reshape(-1)[-2:] = (0.0, 1.0)
    return depth, opacity, rng.uniform(0, 1, (h, w)) > 0.3


def rgb_case(h, w, seed=6):
    """(rgb [h,w,3] float32 spanning [-0.2, 1.3] with the quantiser's edges, an opacity [h,w], a lidar depth map [h,w] that is 0 on
    most pixels)."""
    rng = np.random.default_rng(seed + 100 * h + w)
    rgb = rng.uniform(-0.2, 1.3, (h, w, 3)).astype(np.float32)
    one = np.float32(1)
    edge = np.float32([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 1 / 255, 254.999 / 255, 0.5, np.nan])
    n = min(len(edge), rgb.size)
    rgb.reshape(-1)[:n] = edge[:n]
    op = rng.uniform(0, 1, (h, w)).astype(np.float32)
    lidar = np.where(rng.uniform(0, 1, (h, w)) < 0.25, np.exp(rng.uniform(np.log(2.0), np.log(150.0), (h, w))), 0.0).astype(np.float32)
    lidar.reshape(-1)[-1] = -1.0
    return rgb, op, lidar


def render_results(dataset_type, cam_names, T=MERGED_T, h=H, w=W, seed=9, short_sides=False):
    """The dict of numpy lists that the reference's ``render`` returns, for T timesteps of ``cam_names``: per view float32 ``rgbs``,
    ``gt_rgbs`` [h,w,3], ``depths``, ``opacities``, ``Dynamic_depths``, ``Dynamic_opacities``, ``RigidNodes_opacities``,
    ``gt_sky_masks`` [h,w], and ``cam_names``."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("rgbs", "gt_rgbs", "depths", "opacities", "Dynamic_depths", "Dynamic_opacities", "RigidNodes_opacities",
                           "gt_sky_masks", "cam_names")}
    for _ in range(T):
        for name in cam_names:
            hh = WAYMO_SIDE_H * h // H if (short_sides and name in ("left_camera", "right_camera")) else h
            out["rgbs"].append(rng.uniform(0, 1, (hh, w, 3)).astype(np.float32))
            out["gt_rgbs"].append(rng.uniform(0, 1, (hh, w, 3)).astype(np.float32))
            for k in ("depths", "Dynamic_depths"):
                out[k].append(np.exp(rng.uniform(np.log(2.0), np.log(200.0), (hh, w))).astype(np.float32))
            for k in ("opacities", "Dynamic_opacities", "RigidNodes_opacities"):
                out[k].append(rng.uniform(0, 1, (hh, w)).astype(np.float32))
            out["gt_sky_masks"].append((rng.uniform(0, 1, (hh, w)) > 0.5).astype(np.float32))
            out["cam_names"].append(name)
    return out


class RecordingWriter:
    """Stands in for imageio's writer: keeps what it is given."""

    def __init__(self, log, path, **kw):
        self.path, self.kw, self.frames, self.closed = path, kw, [], False
        log.append(self)

    def append_data(self, frame):
        self.frames.append(np.array(frame, copy=True))

    def close(self):
        self.closed = True


def writer_factory(log):
    return lambda path, **kw: RecordingWriter(log, path, **kw)


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}
