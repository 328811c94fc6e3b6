"""Restatement of the reference's geometry scoring (models/video_utils.py:363-536 over utils/chamfer_distance.py:34-75) for the tests of
bilateral_driving_amd/geometry.py, in numpy.  pytorch3d is not installed, so ``knn_points(norm=2, K=1).dists`` is restated from its
documented behaviour: per point the SQUARED Euclidean distance to the nearest point of the other cloud (``norm=1``: the sum of absolute
differences), here by brute force over all pairs from the coordinate differences.

    hit = gt > 0 and not egocar;  valid = hit and 0.01 < gt < 80 and 1e-4 < pred < 80      (float32 comparisons, as torch's)
    pixel (v,u), depth z -> ((u - cx) z / fx, (v - cy) z / fy, z, 1) through camera_to_world
    trimmed mean at q: the mean of sorted[:int(n * q)];  median_squared: sorted(err^2)[(n - 1) // 2]
    a class: the valid pixels where its mask is non-zero; background: those of none of the four; an absent mask is all-false

Everything after the validity test is taken in float64 (the reference of the tests) or in float32 (the precision the reference itself
runs at: its distance from float64 sets the tests' bounds, ``bound()``)."""
import functools
import math

import numpy as np

CLASSES = ("sky", "dynamic", "human", "vehicle", "background")
MASK_KEYS = ("sky_masks", "dynamic_masks", "human_masks", "vehicle_masks")
QS = (("", 1.0), ("_99", 0.99), ("_97", 0.97), ("_95", 0.95))
FRAME_KEYS = ("chamfer", "chamfer_99", "chamfer_97", "chamfer_95", "depth_err", "depth_err_rmse_99", "depth_err_rmse_97",
              "depth_err_rmse_95", "depth_err_median_squared")
SCALARS = FRAME_KEYS + tuple(f"chamfer_{c}" for c in CLASSES) + tuple(f"{a}{t}" for a in ("cham_pred", "cham_gt", "abs_err") for t, _ in QS)
# What a float32 implementation may differ by where the float32 restatement happens to be exact or nearly so.  MEASURED with the host
# shim over CASES (tests/test_geometry_cpu.py prints the figures; its docstring records them), not chosen in advance.
FLOOR = 1e-6


def valid_mask(pred, gt, egocar=None):
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    hit = gt > 0
    if egocar is not None:
        hit &= ~(np.asarray(egocar) != 0)
    return hit & (gt > np.float32(0.01)) & (gt < np.float32(80.0)) & (pred > np.float32(0.0001)) & (pred < np.float32(80.0))


def unproject(depth, K, c2w, mask, dtype):
    """depth_map_to_point_cloud (chamfer_distance.py:54-75) with every operation in ``dtype``: [n,3] in row-major pixel order."""
    v, u = np.nonzero(mask)
    z = np.asarray(depth, dtype)[v, u]
    K, c2w = np.asarray(K, dtype), np.asarray(c2w, dtype)
    x = (u.astype(dtype) - K[0, 2]) * z / K[0, 0]
    y = (v.astype(dtype) - K[1, 2]) * z / K[1, 1]
    hom = np.stack([x, y, z, np.ones_like(z)], 1)
    out = (c2w @ hom.T).T[:, :3]
    assert out.dtype == dtype
    return np.ascontiguousarray(out)


def nearest(x, y, norm=2):
    """Per point of x its distance (see the module docstring) to the nearest point of y, in the arrays' dtype; +inf for an empty y."""
    out = np.full(len(x), np.inf, x.dtype)
    if len(y) == 0:
        return out
    for i in range(0, len(x), 256):
        d = x[i:i + 256, None, :] - y[None, :, :]
        out[i:i + 256] = ((d * d) if norm == 2 else np.abs(d)).sum(-1).min(1)
    return out


def _mean(a):
    return float(a.mean()) if len(a) else math.nan


def frame(pred, gt, K, c2w, masks=None, egocar=None, dtype=np.float64):
    """One frame: every name of ``SCALARS`` (NaN where the reference's expression gives NaN), ``valid`` (n), ``<class>_valid``, and the
    arrays ``dist_pred``, ``dist_gt``, ``points_pred``, ``points_gt``.  ``pred``, ``gt``: float32 [H,W]; ``masks``: {key of MASK_KEYS:
    [H,W], non-zero = true}."""
    masks = masks or {}
    valid = valid_mask(pred, gt, egocar)
    P, G = unproject(pred, K, c2w, valid, dtype), unproject(gt, K, c2w, valid, dtype)
    dp, dg = nearest(P, G), nearest(G, P)
    err = np.abs(np.asarray(pred, dtype)[valid] - np.asarray(gt, dtype)[valid])
    n = int(valid.sum())
    out = {"valid": n, "dist_pred": dp, "dist_gt": dg, "points_pred": P, "points_gt": G}
    sp, sg, se = np.sort(dp), np.sort(dg), np.sort(err)
    for tag, q in QS:
        k = n if q == 1.0 else int(n * q)
        out[f"cham_pred{tag}"], out[f"cham_gt{tag}"], out[f"abs_err{tag}"] = _mean(sp[:k]), _mean(sg[:k]), _mean(se[:k])
        out[f"chamfer{tag}"] = out[f"cham_pred{tag}"] + out[f"cham_gt{tag}"]
        out["depth_err" if q == 1.0 else f"depth_err_rmse{tag}"] = float(np.sqrt(np.square(se[:k]).mean())) if k else math.nan
    out["depth_err_median_squared"] = float(np.sort(np.square(err))[(n - 1) // 2]) if n else math.nan
    inside = {c: (np.asarray(masks[k]) != 0) if k in masks else np.zeros(valid.shape, bool) for c, k in zip(CLASSES, MASK_KEYS)}
    inside["background"] = ~(inside["sky"] | inside["dynamic"] | inside["human"] | inside["vehicle"])
    for c in CLASSES:
        sel = inside[c][valid]
        out[f"{c}_valid"] = int(sel.sum())
        out[f"chamfer_{c}"] = _mean(nearest(P[sel], G[sel])) + _mean(nearest(G[sel], P[sel]))
    return out


def reference_frame(f):
    """``frame``'s values as the reference's per-frame lists receive them: the whole-frame keys always, a class only when not NaN."""
    out = {k: f[k] for k in FRAME_KEYS}
    out.update({f"chamfer_{c}": f[f"chamfer_{c}"] for c in CLASSES if not math.isnan(f[f"chamfer_{c}"])})
    return out


def non_zero_mean(x):
    return sum(x) / len(x) if len(x) > 0 else -1


def results(frames):
    """results_dict's geometry entries (video_utils.py:558-573) from ``reference_frame`` dicts."""
    out = {}
    for k in FRAME_KEYS + tuple(f"chamfer_{c}" for c in CLASSES):
        out[f"avg_{k}" if k.startswith("chamfer") else k] = non_zero_mean([f[k] for f in frames if k in f])
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def camera(H, W, translation=(5.0, -3.0, 1.5)):
    """(K [3,3], c2w [4,4]) float32: a pinhole whose principal point is off the pixel grid, yawed and pitched, at ``translation``."""
    K = np.array([[0.8 * W, 0, 0.5 * W - 0.25], [0, 0.8 * W, 0.5 * H + 0.125], [0, 0, 1]], np.float32)
    a, b = 0.3, 0.1
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Ry @ Rx, translation
    return K, c2w.astype(np.float32)


def make_frame(H, W, n, seed=0, empty=(), one=(), egocar=False, absent=()):
    """(pred, gt, masks, egocar mask or None): exactly ``n`` valid pixels (lidar returns at ``n`` random pixels, 2 .. 55 m; the render
    within 2 % of them plus a few far misses), ``human`` inside ``dynamic``, ``vehicle`` = the rest of ``dynamic``, ``sky`` outside it.
    ``empty``: classes without a valid pixel; ``one``: classes with exactly one (needs n >= 3); ``absent``: mask keys left out."""
    g = np.random.default_rng([seed, H, W, n])
    ego = np.zeros((H, W), bool)
    if egocar:
        ego[H - H // 5:] = True
    free = np.flatnonzero(~ego.ravel())
    hits = g.choice(free, n, replace=False)
    gt = np.zeros(H * W, np.float32)
    gt[hits] = g.uniform(2.0, 55.0, n)
    if egocar:                                   # lidar returns under the ego car, which the mask removes
        gt[np.flatnonzero(ego.ravel())[::3]] = 4.0
    pred = g.uniform(1.0, 70.0, H * W).astype(np.float32)
    pred[hits] = gt[hits] * (1 + g.normal(0, 0.02, n))
    if n >= 8:
        pred[hits[:max(n // 50, 1)]] *= 1.3      # the outliers the trims remove
    dyn = g.uniform(0, 1, H * W) < 0.35
    human = dyn & (g.uniform(0, 1, H * W) < 0.4)
    masks = {"sky_masks": ~dyn & (g.uniform(0, 1, H * W) < 0.15), "dynamic_masks": dyn, "human_masks": human, "vehicle_masks": dyn & ~human}
    key = dict(zip(CLASSES, MASK_KEYS))
    for c in tuple(empty) + tuple(one):
        masks[key[c]][hits] = False
    for i, c in enumerate(one):
        masks[key[c]][hits[i]] = True
        if c == "human":
            masks["dynamic_masks"][hits[i]] = True
    return pred.reshape(H, W), gt.reshape(H, W), {k: m.reshape(H, W) for k, m in masks.items() if k not in absent}, (ego if egocar else None)


def edge_frame():
    """8x16 pixels whose depths sit on and next to the validity limits (0.01 and 80 for the lidar, 1e-4 and 80 for the render); returns
    (pred, gt, the expected valid mask)."""
    f = np.float32
    up, down = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
    gts = [f(0.0), down(0.01), f(0.01), up(0.01), f(5.0), down(80.0), f(80.0), up(80.0)]
    preds = [f(0.0), down(1e-4), f(1e-4), up(1e-4), f(5.0), down(80.0), f(80.0), up(80.0), f(-1.0), f(np.inf), f(np.nan)]
    gt = np.zeros((8, 16), f)
    pred = np.zeros((8, 16), f)
    ok = np.zeros((8, 16), bool)
    for i, a in enumerate(gts):
        for j, b in enumerate(preds):
            gt[i, j], pred[i, j] = a, b
            ok[i, j] = i in (3, 4, 5) and j in (3, 4, 5)
    return pred, gt, ok


# name -> (H, W, n, make_frame keywords, camera translation)
CASES = {
    "n0": (24, 40, 0, {}, None), "n1": (24, 40, 1, {}, None), "n2": (24, 40, 2, {}, None), "n19": (24, 40, 19, {}, None),
    "n20": (24, 40, 20, {}, None), "n21": (24, 40, 21, {}, None),
    "n511": (40, 56, 511, {}, None), "n512": (40, 56, 512, {}, None), "n513": (40, 56, 513, {"egocar": True}, None),
    "n1700": (64, 96, 1700, {"egocar": True}, None),
    "empty_human": (33, 47, 300, {"empty": ("human",)}, None), "one_vehicle": (33, 47, 300, {"one": ("vehicle", "sky")}, None),
    "absent_vehicle": (33, 47, 300, {"absent": ("vehicle_masks",)}, None), "no_masks": (33, 47, 300, {"absent": MASK_KEYS}, None),
    "far": (33, 47, 300, {}, (1000.0, -800.0, 30.0)),
    "n513_without_egocar": (40, 56, 513, {"egocar": True}, None),      # the same frame, its egocar mask not handed over
    "edges": (8, 16, 9, None, None),                                   # edge_frame()
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs dict, float64 frame, float32 frame) of one test case; computed once, shared, never modified."""
    H, W, n, kw, t = CASES[name]
    if name == "edges":
        pred, gt, ok = edge_frame()
        masks, ego = {"dynamic_masks": ok & (np.arange(W) % 2 == 0)}, None
    else:
        pred, gt, masks, ego = make_frame(H, W, n, **kw)
    if name.endswith("_without_egocar"):
        ego, n = None, int(valid_mask(pred, gt).sum())
    K, c2w = camera(H, W) if t is None else camera(H, W, t)
    inp = {"pred": pred, "gt": gt, "K": K, "c2w": c2w, "masks": masks, "egocar": ego}
    r64, r32 = (frame(pred, gt, K, c2w, masks, ego, d) for d in (np.float64, np.float32))
    assert r64["valid"] == r32["valid"] == n
    return inp, r64, r32


def bound(r64, r32, key):
    """What a float32 implementation is held to for ``key``: twice the float32 restatement's own distance from float64 (the worst
    element for an array), plus ``FLOOR``.  Returns (bound, float32 restatement's error); a NaN in float64 must be matched by a NaN."""
    a, b = np.asarray(r64[key], np.float64), np.asarray(r32[key], np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), key
    e32 = float(np.nanmax(np.abs(a - b))) if a.size and not np.all(np.isnan(a)) else 0.0
    return 2.0 * e32 + FLOOR, e32


def error(got, r64, key):
    """|got - float64| for ``key`` (the worst element for an array); inf when a NaN stands on one side only."""
    a, b = np.asarray(got, np.float64), np.asarray(r64[key], np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return math.inf
    return float(np.nanmax(np.abs(a - b))) if a.size and not np.all(np.isnan(a)) else 0.0
