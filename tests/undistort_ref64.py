"""A numpy restatement of the lens undistortion (``bds_undistort``, ``undistort.optimal_new_camera_matrix``), written from the
algorithm's statement in include/bds.h and not from the product's code: the map in float64 with every operation on its own, the taps
on the 1/32-pixel grid with integer weights and integer rounding, a constant 0 border.  numpy's float64 operations are IEEE and
unfused, ``np.rint`` rounds half to even, and ``>>`` / ``&`` on negative int64 floor and give the non-negative rest.

Also the fixed cases the CPU and GPU tests share (shape, camera matrix, coefficient sets) and the classification of a map's pixels."""
import numpy as np

F, H, W = 3, 37, 53
K = np.array([[40.0, 0.0, 26.1], [0.0, 41.5, 18.3], [0.0, 0.0, 1.0]])
NEW_K_SHIFT = np.array([[30.0, 0.0, 35.0], [0.0, 30.0, 25.0], [0.0, 0.0, 1.0]])
COEFFS = {"zero": (0.0, 0.0, 0.0, 0.0, 0.0), "barrel": (-0.32, 0.11, 0.004, -0.003, -0.02), "pincushion": (0.25, 0.08, -0.006, 0.005, 0.01)}
CASES = {"zero": ("zero", None), "barrel": ("barrel", None), "pincushion": ("pincushion", None), "pin+shift": ("pincushion", NEW_K_SHIFT)}
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def case(name):
    """(K, dist [5], new K or None)"""
    coeffs, new_K = CASES[name]
    return K, np.array(COEFFS[coeffs], np.float64), new_K


def source_map(h, w, Kmat, dist, new_K=None):
    """(u, v) [h,w] float64: where output pixel (row i, column j) reads the source."""
    Kmat = np.asarray(Kmat, np.float64)
    k1, k2, p1, p2, k3 = (np.float64(d) for d in dist)
    ir = np.linalg.inv(Kmat if new_K is None else np.asarray(new_K, np.float64)).reshape(9)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    _x = j * ir[0] + i * ir[1] + ir[2]
    _y = j * ir[3] + i * ir[4] + ir[5]
    _w = j * ir[6] + i * ir[7] + ir[8]
    x, y = _x / _w, _y / _w
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
    return Kmat[0, 0] * xd + Kmat[0, 2], Kmat[1, 1] * yd + Kmat[1, 2]


def fixed(t):
    """rint(32 t) saturated to int32, as int64"""
    with np.errstate(invalid="ignore"):
        s = np.rint(np.asarray(t, np.float64) * 32)
    s = np.where(np.isnan(s), INT32_MIN, s)
    return np.clip(s, INT32_MIN, INT32_MAX).astype(np.int64)


def taps(u, v):
    """sx, sy, ax, ay (int64) and the four weights w00, w01, w10, w11"""
    iu, iv = fixed(u), fixed(v)
    sx, sy, ax, ay = iu >> 5, iv >> 5, iu & 31, iv & 31
    return sx, sy, ax, ay, ((32 - ay) * (32 - ax) * 32, (32 - ay) * ax * 32, ay * (32 - ax) * 32, ay * ax * 32)


def remap(img, u, v):
    """``img`` [h,w] or [h,w,c] uint8 -> uint8 of the map's shape (+ channels)"""
    img = np.asarray(img)
    chan = img[..., None] if img.ndim == 2 else img
    h, w = chan.shape[:2]
    sx, sy, _, _, ws = taps(u, v)
    acc = np.zeros(u.shape + (chan.shape[2],), np.int64)
    for (dy, dx), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), ws):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        val = chan[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64) * ok[..., None]
        acc += val * wt[..., None]
    out = (acc + 16384) >> 15
    gone = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    out[gone] = 0
    assert out.min() >= 0 and out.max() <= 255
    out = out.astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


def undistort(frames, Ks, dists, new_Ks=None, kind="uint8"):
    """``frames`` [F,h,w] or [F,h,w,3] uint8 with per-frame (or single) K, dist, new K -> the three output forms."""
    frames = np.asarray(frames)
    n = frames.shape[0]
    Ks = np.broadcast_to(np.asarray(Ks, np.float64), (n, 3, 3))
    dists = np.broadcast_to(np.asarray(dists, np.float64), (n, 5))
    out = []
    for f in range(n):
        nk = None if new_Ks is None else (new_Ks[f] if np.ndim(new_Ks) == 3 or isinstance(new_Ks, (list, tuple)) else new_Ks)
        u, v = source_map(frames.shape[1], frames.shape[2], Ks[f], dists[f], nk)
        out.append(remap(frames[f], u, v))
    out = np.stack(out)
    if kind == "uint8":
        return out
    if kind == "unit":
        return out.astype(np.float32) / np.float32(255)
    assert kind == "mask"
    return (out > 0).astype(np.float32)


def classify(u, v, h, w):
    """Counts of a map's pixel classes: fully outside, partial (inside the window test, at least one tap outside), the four edges,
    and the distance of 32 u, 32 v from a rounding tie."""
    sx, sy, ax, ay, _ = taps(u, v)
    gone = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
    tap_out = (sx < 0) | (sx + 1 >= w) | (sy < 0) | (sy + 1 >= h)
    live = ~gone
    frac = np.concatenate([(u * 32 - np.floor(u * 32)).ravel(), (v * 32 - np.floor(v * 32)).ravel()])
    return {"outside": int(gone.sum()), "partial": int((live & tap_out).sum()), "left": int((live & (sx == -1)).sum()),
            "top": int((live & (sy == -1)).sum()), "right": int((live & (sx == w - 1)).sum()), "bottom": int((live & (sy == h - 1)).sum()),
            "tie_margin": float(np.abs(frac - 0.5).min()), "min_source": float(min(u.min(), v.min())),
            "negative_fixed": int(((fixed(u) < 0) | (fixed(v) < 0)).sum())}


def frames_case(channels, seed=5):
    """[F,H,W] or [F,H,W,3] uint8 noise with some exact zeros (the masks' ``> 0``) and 255s"""
    g = np.random.default_rng(seed)
    shape = (F, H, W) if channels == 1 else (F, H, W, 3)
    img = g.integers(0, 256, shape, dtype=np.uint8)
    img[g.random(shape) < 0.3] = 0
    img[g.random(shape) < 0.05] = 255
    return img


# ---- getOptimalNewCameraMatrix ------------------------------------------------------------------------------------------------------------
def undistort_points(pu, pv, Kmat, dist, iterations=5):
    k1, k2, p1, p2, k3 = (np.float64(d) for d in dist)
    x0, y0 = (pu - Kmat[0, 2]) / Kmat[0, 0], (pv - Kmat[1, 2]) / Kmat[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        icd = 1 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def grid_points(w, h):
    """the 81 image points, [9,9] each, row = y index"""
    return np.meshgrid(np.arange(9) * (w - 1) / 8.0, np.arange(9) * (h - 1) / 8.0)


def optimal_new_camera_matrix(Kmat, dist, size, alpha=1.0):
    Kmat = np.asarray(Kmat, np.float64)
    w, h = size
    pu, pv = grid_points(w, h)
    x, y = undistort_points(pu, pv, Kmat, dist)
    outer = (x.min(), y.min(), x.max() - x.min(), y.max() - y.min())
    ix0, ix1 = max(x[r, 0] for r in range(9)), min(x[r, 8] for r in range(9))
    iy0, iy1 = max(y[0, c] for c in range(9)), min(y[8, c] for c in range(9))
    inner = (ix0, iy0, ix1 - ix0, iy1 - iy0)
    M = np.eye(3)
    for axis, n in ((0, w), (1, h)):
        f0 = (n - 1) / inner[2 + axis]
        f1 = (n - 1) / outer[2 + axis]
        c0, c1 = -f0 * inner[axis], -f1 * outer[axis]
        M[axis, axis] = (1 - alpha) * f0 + alpha * f1
        M[axis, 2] = (1 - alpha) * c0 + alpha * c1
    return M


def redistortion_residual(Kmat, dist, size):
    """The largest distance, in pixels, between the 81 grid points and their undistorted coordinates pushed through the forward
    model again: how far the five fixed iterations are from the model's inverse."""
    Kmat = np.asarray(Kmat, np.float64)
    k1, k2, p1, p2, k3 = dist
    pu, pv = grid_points(*size)
    x, y = undistort_points(pu, pv, Kmat, dist)
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * (2 * x * y) + p2 * (r2 + 2 * x * x)
    yd = y * kr + p1 * (r2 + 2 * y * y) + p2 * (2 * x * y)
    return float(np.hypot(Kmat[0, 0] * xd + Kmat[0, 2] - pu, Kmat[1, 1] * yd + Kmat[1, 2] - pv).max())


# ---- a bare camera for the loaders ------------------------------------------------------------------------------------------------------
def write_camera_files(tmp_path, F=2, h=20, w=26):
    """tiny PNGs written with PIL, larger than the load size so that the resize filters run"""
    from PIL import Image
    g = np.random.default_rng(3)
    paths = {k: [] for k in ("img", "dynamic_mask", "human_mask", "vehicle_mask", "sky_mask")}
    for f in range(F):
        for k in paths:
            name = str(tmp_path / f"{k}_{f}.png")
            if k == "img":
                Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(name)
            else:
                Image.fromarray(((g.random((h, w)) < 0.4) * 255).astype(np.uint8)).save(name)
            paths[k].append(name)
    return paths


class BareLoaderCamera:
    """What the four loaders read of a CameraData."""

    def __init__(self, paths, device, undistort):
        import torch
        self.img_filepaths = np.array(paths["img"])
        for k in ("dynamic_mask", "human_mask", "vehicle_mask", "sky_mask"):
            setattr(self, f"{k}_filepaths", np.array(paths[k]))
        F = len(paths["img"])
        self.load_size, self.undistort, self.device = [14, 19], undistort, device
        self.dataset_name, self.cam_id = "no_such_dataset", 0
        self.intrinsics = torch.tensor([[15.0, 0, 9.2], [0, 15.5, 6.8], [0, 0, 1]]).expand(F, 3, 3).clone()
        self.distortions = torch.tensor([[-0.2, 0.05, 0.002, -0.001, 0.0], [0.15, 0.02, -0.003, 0.002, 0.01]])[:F].clone()
