"""Numpy restatement of a view's input preparation (bilateral_driving_amd/pixels.py, csrc/pixels.hip): CameraData.get_image
(datasets/base/pixel_source.py:477-657, get_rays :38-75) and ScenePixelSource.prepare_novel_view_render_data (:1070-1132).

Every function takes a ``dtype``: ``np.float64`` is the exact reading of the float32 inputs, ``np.float32`` evaluates the same
expression with every operation rounded to float32 on its own (numpy never fuses a multiply and an add), which is what the kernels and
the host shim compute.  ``pixel_coords``, ``origins``, the fills, the masks and the intrinsics are bit-equal to torch's in the float32
mode; ``viewdirs``, ``direction_norm`` and the resized image are held to MEASURED bounds: ``bound(f32, f64)`` is four times the
distance of the float32 framework expression from float64 on the same inputs, at least 1e-6 absolute (a kernel may order a sum
otherwise than torch does, and the reference's own float32 stands that far from the exact value).

Also here: the golden file's cases (tests/golden/get_image.npz, scripts/gen_golden_get_image.py) and the bare objects the tests hand
to ``pixels.get_image`` / ``pixels.prepare_novel_view_render_data``."""
import math
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "get_image.npz")
FACTORS = (1.0, 0.5, 0.25)
GOLDEN_H, GOLDEN_W, GOLDEN_FRAMES, GOLDEN_POSES = 12, 20, 3, 3
MASKS = ("egocar_mask", "sky_masks", "dynamic_masks", "human_masks", "vehicle_masks")                 # the object's attributes
MASK_KEYS = ("egocar_masks", "sky_masks", "dynamic_masks", "human_masks", "vehicle_masks")           # image_infos' keys
FLOOR = 1e-6


def bound(f32, f64) -> float:
    """4 x the distance of a float32 evaluation from float64, at least FLOOR."""
    return max(4.0 * float(np.max(np.abs(np.asarray(f32, np.float64) - np.asarray(f64, np.float64)), initial=0.0)), FLOOR)


def output_size(H, W, factor):
    return int(math.floor(float(H) * factor)), int(math.floor(float(W) * factor))


# ---- rays and fields ------------------------------------------------------------------------------------------------------------------
def scaled_intrinsics(K, scale, dtype=np.float32):
    out = np.asarray(K, dtype) * dtype(scale)
    out[..., 2, 2] = 1.0
    return out


def rays(c2w, K, scale, H, W, dtype=np.float64):
    """-> origins [H,W,3], viewdirs [H,W,3], direction_norm [H,W,1], pixel_coords [H,W,2] of one view."""
    c2w, Ks = np.asarray(c2w, dtype), scaled_intrinsics(K, scale, dtype)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = x.astype(dtype), y.astype(dtype)
    dx = ((x - Ks[0, 2]) + dtype(0.5)) / Ks[0, 0]
    dy = ((y - Ks[1, 2]) + dtype(0.5)) / Ks[1, 1]
    R = c2w[:3, :3]
    d = np.stack([(dx * R[i, 0] + dy * R[i, 1]) + R[i, 2] for i in range(3)], axis=-1)
    n = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])[..., None]
    viewdirs = d / (n + dtype(1e-8))
    origins = np.broadcast_to(c2w[:3, 3], (H, W, 3)).copy()
    coords = np.stack([y / dtype(H), x / dtype(W)], axis=-1)
    return origins, viewdirs, n, coords


# ---- the resizes ------------------------------------------------------------------------------------------------------------------------
def cubic(x, dtype):
    A = dtype(-0.5)
    x = np.abs(x)
    near = ((A + dtype(2)) * x - (A + dtype(3))) * x * x + dtype(1)
    far = ((A * x - dtype(5) * A) * x + dtype(8) * A) * x - dtype(4) * A
    return np.where(x < 1, near, np.where(x < 2, far, dtype(0))).astype(dtype)


def axis_scale(factor, dtype):
    return dtype(1.0 / factor)      # torch: the double quotient, converted to the computation's type


def aa_window(i, scale, n_in, dtype):
    """(lo, normalised weights) of output i on an axis of n_in samples."""
    support = dtype(2) * scale
    c = scale * (dtype(i) + dtype(0.5))
    lo = max(0, int((c - support) + dtype(0.5)))
    n = min(n_in, int((c + support) + dtype(0.5))) - lo
    w = cubic(((np.arange(lo, lo + n).astype(dtype) - c) + dtype(0.5)) / scale, dtype)
    total = dtype(0)
    for v in w:      # the sum in tap order
        total = dtype(total + v)
    return lo, (w / total).astype(dtype)


def resize_axis(a, factor, axis, dtype):
    a = np.moveaxis(np.asarray(a, dtype), axis, 0)
    n_in = a.shape[0]
    n_out = int(math.floor(float(n_in) * factor))
    scale = axis_scale(factor, dtype)
    out = np.zeros((n_out,) + a.shape[1:], dtype)
    for i in range(n_out):
        lo, w = aa_window(i, scale, n_in, dtype)
        acc = np.zeros(a.shape[1:], dtype)
        for j, wj in enumerate(w):      # tap by tap, every product and sum rounded
            acc = (acc + wj * a[lo + j]).astype(dtype)
        out[i] = acc
    return np.moveaxis(out, 0, axis)


def resize_aa(img, factor, dtype=np.float64):
    """[H,W,3] -> [floor(H factor), floor(W factor), 3]: width first, then height."""
    return resize_axis(resize_axis(img, factor, 1, dtype), factor, 0, dtype)


def nearest_index(n_out, n_in, factor):
    scale = np.float32(1.0 / factor)
    return np.minimum(np.floor(np.arange(n_out).astype(np.float32) * scale).astype(np.int64), n_in - 1)


def resize_nearest(mask, factor):
    H, W = mask.shape
    Ho, Wo = output_size(H, W, factor)
    return mask[nearest_index(Ho, H, factor)][:, nearest_index(Wo, W, factor)]


def downsample_sparse(depth, factor):
    from tests import lidar_ref64
    return lidar_ref64.downsample(depth, factor, np.float32)[0]


# ---- get_image and the novel views ------------------------------------------------------------------------------------------------------
def get_image(cam, frame, factor, dtype=np.float64):
    """``cam``: dict of numpy arrays under the object's attribute names.  -> (image_infos, cam_infos) as numpy."""
    rgb = cam["images"][frame]
    H, W = rgb.shape[:2]
    if factor != 1.0:
        rgb = resize_aa(rgb, factor, dtype)
        H, W = rgb.shape[:2]
    origins, viewdirs, norm, coords = rays(cam["cam_to_worlds"][frame], cam["intrinsics"][frame], factor, H, W, dtype)
    info = {"origins": origins, "viewdirs": viewdirs, "direction_norm": norm, "pixel_coords": coords,
            "normed_time": np.full((H, W), cam["normalized_time"][frame], np.float32),
            "img_idx": np.full((H, W), cam["unique_img_idx"][frame], np.int64), "frame_idx": np.full((H, W), frame, np.int64), "pixels": rgb}
    for attr, key in zip(MASKS, MASK_KEYS):
        m = cam[attr] if attr == "egocar_mask" else cam[attr][frame]
        info[key] = m if factor == 1.0 else resize_nearest(m, factor)
    d = cam["lidar_depth_maps"][frame]
    info["lidar_depth_map"] = d if factor == 1.0 else downsample_sparse(d, factor)
    cams = {"cam_id": np.full((H, W), int(cam["cam_id"]), np.int64), "camera_to_world": cam["cam_to_worlds"][frame],
            "height": np.int64(H), "width": np.int64(W), "intrinsics": scaled_intrinsics(cam["intrinsics"][frame], factor, np.float32)}
    return info, cams


def novel_frames(num_frames, n):
    import torch
    return torch.linspace(0, num_frames - 1, n).round().long().numpy(), torch.linspace(0, 1, n).numpy()


def novel_views(cam, traj, num_frames, dtype=np.float64):
    H, W = cam["images"].shape[1:3]
    frames, times = novel_frames(num_frames, len(traj))
    out = []
    for i, c2w in enumerate(traj):
        origins, viewdirs, norm, coords = rays(c2w, cam["intrinsics"][0], 1.0, H, W, dtype)
        out.append({"origins": origins, "viewdirs": viewdirs, "direction_norm": norm, "pixel_coords": coords,
                    "img_idx": np.full((H, W), i, np.int64), "frame_idx": np.full((H, W), frames[i], np.int64),
                    "normed_time": np.full((H, W), times[i], np.float32)})
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def random_pose(g, far=0.0):
    """A camera-to-world matrix with a general rotation; ``far``: metres from the origin."""
    q = g.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = g.uniform(-30, 30, 3) + far * np.array([0.6, -0.64, 0.48])
    return M.astype(np.float32)


def random_intrinsics(g, H, W):
    K = np.eye(3)
    K[0, 0], K[1, 1] = g.uniform(0.7, 1.3, 2) * W
    K[0, 2], K[1, 2] = W / 2 + g.uniform(-2, 2), H / 2 + g.uniform(-2, 2)
    return K.astype(np.float32)


def view_case(seed, B, H, W, far=0.0):
    g = np.random.default_rng(seed)
    return {"c2w": np.stack([random_pose(g, far) for _ in range(B)]), "K": np.stack([random_intrinsics(g, max(H, 2), max(W, 2)) for _ in range(B)]),
            "time": g.uniform(0, 1, B).astype(np.float32), "img": g.integers(0, 5000, B), "frame": g.integers(0, 300, B),
            "cam": g.integers(0, 6, B)}


def image_case(kind, H, W, seed=0):
    g = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return g.uniform(0, 1, (H, W, 3)).astype(np.float32)
    if kind == "step":
        img = np.zeros((H, W, 3), np.float32)
        img[:, W // 2:] = 1.0
        img[H // 3:, :, 1] = 0.25
        return img
    if kind == "constant":
        return np.full((H, W, 3), np.float32(0.7), np.float32)
    raise KeyError(kind)


def mask_case(n, H, W, seed=0):
    g = np.random.default_rng(2000 + seed)
    return [(g.uniform(0, 1, (H, W)) < 0.4).astype(np.float32) * g.uniform(0.5, 1.0, (H, W)).astype(np.float32) for _ in range(n)]


def golden_inputs(seed=7):
    """The camera the golden file records: 3 frames of 12 x 20, all five masks, a sparse lidar map, normalized time."""
    g = np.random.default_rng(seed)
    F, H, W = GOLDEN_FRAMES, GOLDEN_H, GOLDEN_W
    depth = g.uniform(2, 60, (F, H, W)).astype(np.float32) * (g.uniform(0, 1, (F, H, W)) < 0.3)
    cam = {"images": g.uniform(0, 1, (F, H, W, 3)).astype(np.float32),
           "cam_to_worlds": np.stack([random_pose(g) for _ in range(F)]), "intrinsics": np.stack([random_intrinsics(g, H, W) for _ in range(F)]),
           "egocar_mask": (g.uniform(0, 1, (H, W)) < 0.2).astype(np.float32), "lidar_depth_maps": depth.astype(np.float32),
           "normalized_time": np.linspace(0, 1, F).astype(np.float32), "unique_img_idx": np.array([4, 9, 14], np.int64),
           "cam_id": np.int64(2)}
    for attr in MASKS[1:]:
        cam[attr] = (g.uniform(0, 1, (F, H, W)) < 0.35).astype(np.float32)
    traj = np.stack([random_pose(g) for _ in range(GOLDEN_POSES)])
    return cam, traj


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_camera():
    z = golden()
    return {k[4:]: z[k] for k in z if k.startswith("cam_")}, z["traj"]


class BareCamera:
    """What ``get_image`` reads of a CameraData, tensors on ``device``."""

    def __init__(self, cam, factor, device, cam_name="front_camera"):
        import torch
        for k, v in cam.items():
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(v)).to(device) if k not in ("cam_id", "normalized_time", "unique_img_idx")
                    else v)
        # the reference's CameraData keeps these on the host
        self.normalized_time, self.unique_img_idx = torch.from_numpy(cam["normalized_time"]), torch.from_numpy(cam["unique_img_idx"])
        self.cam_id = int(cam["cam_id"])
        self.HEIGHT, self.WIDTH = (int(s) for s in cam["images"].shape[1:3])
        self.downscale_factor, self.device, self.cam_name = factor, device, cam_name


def bare_pixel_source(cam, device, num_frames, second=None):
    cams = {0: BareCamera(cam, 1.0, device)}
    if second is not None:
        cams[1] = BareCamera(second, 1.0, device)
    return types.SimpleNamespace(camera_data=cams, num_frames=num_frames, device=device)
