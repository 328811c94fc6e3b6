"""Float64 restatement of the pseudo-lidar generation (bilateral_driving_amd/pseudo_lidar.py, csrc/pseudo_lidar.hip), with a bound on
what float32 may change, the decided / undecided classification, and the test cases.  Test infrastructure only.

The chain.  A pixel (u, v) with depth d is valid iff d > 0 and d < max_depth; pc = ((u - cx) d / fx, (v - cy) d / fy, d); p = M [pc;1]
with M = inverse(lidar_to_world) @ cam_to_world taken in float64 from the float32 inputs; kept iff lo <= p < hi on every axis; then
in double  d3 = sqrt((x x + y y) + z z), r = sqrt(x x + y y) (1e-6 where 0), column = trunc((rad(45) - asin(y / r)) / dphi) clamped to
[0, W-1]; vertical: theta = asin(z / d3), kept iff fov_down <= theta <= fov_up, row = trunc((theta - fov_down) / dtheta) clamped;
classic: row = trunc((rad(2) - asin(z / d3)) / dtheta) clamped.  The highest linear pixel index v * width + u wins a beam; the occupied
beams of the rows with row % slice == 0 are emitted in row-major beam order.

The bounds, with u = 2^-24 and gamma_k = k u / (1 - k u).  The unprojection takes three float32 operations per coordinate: e_pc =
gamma_3 |pc| (0 for z).  A float32 dot product of three terms plus a constant, in any order, with or without fused multiply-add, is
within gamma_4 of the sum of its magnitudes.
  device route     one matrix M32 = fl(M):  e_dev = |M32| e_pc + gamma_4 (|M32| (|pc| + e_pc) + |t32|) + dM [|pc|;1], dM = |M32 - M| +
                   u |M32| + 1e-12 (the product's float64 inverse is another library's: an entry may round the other way)
  reference route  w = c2w [pc;1] in float32, then inv32 [w;1] with inv32 = torch.inverse(lidar_to_world) as this host forms it:
                   e_w = |c2w| e_pc + gamma_4 (|c2w| (|pc| + e_pc) + |t|),
                   e_ref = |inv32| e_w + gamma_4 (|inv32| (|w| + e_w) + |t_inv|) + |inv32 - inv64| [|w|;1]
A coordinate of the device lies within e_dev of the restatement, one of the reference within e_ref, the two within e_dev + e_ref of each
other.  (With world translations of +-300 m e_ref is about 1e-4 m, e_dev about 1e-5 m.)

DECIDED.  A pixel is decided when no perturbation of its coordinates by MARGIN * max(e_dev, e_ref) -- plus the double rounding of
the angle itself -- can change what happens to it: every crop face farther than that, and, inside the crop, both fov limits and every
beam edge farther than the angle that perturbation subtends (a displacement of length rho at range r turns the direction by at
most asin(rho / r); rho >= r leaves it undecided with every beam in reach).  The double arithmetic adds e_num = 8 ud / sqrt(max(1 - s^2 -
16 ud, 4 ud)) + 8 pi ud for asin(s), ud = 2^-53, and 4 ud |t| for the quotient.  A pixel with an invalid depth is always decided: that
test compares float32 values as they are.  A cloud row has exact coordinates (e = 0); only the double rounding is left.
A beam is DIRTY when an undecided pixel can reach it whose index exceeds the beam's decided winner; the others are clean, and there
the winner must be equal for any float32 evaluation."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pseudo_lidar.npz")
U, UD = 2.0 ** -24, 2.0 ** -53
MARGIN = 4.0
CAP_UNDECIDED, CAP_DIRTY = 0.01, 0.02      # of a case's live pixels / of its occupied beams
CROP = (0.0, 80.0, -50.0, 50.0, -2.5, 3.0)
SPARSE_CROP = (0.0, 120.0, -50.0, 50.0, -2.5, 1.5)
RANDOM_SEEDS = (11, 12, 17, 21, 23, 24)      # within the caps (test_pseudo_lidar_cpu asserts it); three of them have dirty beams
RANDOM_SHAPE = dict(Hi=96, Wi=160, H=16, W=32)
GOLDEN_DEPTH = {"front": dict(seed=501, Hi=48, Wi=80, H=8, W=16, yaw=0.0),
                "side": dict(seed=502, Hi=48, Wi=80, H=8, W=16, yaw=math.radians(50.0)),
                "slice": dict(seed=503, Hi=48, Wi=80, H=9, W=16, slice=2, yaw=0.1, downscale=2)}
GOLDEN_CLOUD = dict(seed=504, H=64, W=32, slice=1)


def gamma(k):
    return k * U / (1 - k * U)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def beam_constants(H, W, mode="vertical", fov=(10.0, -30.0)):
    """(rad45, dphi, theta0, fov_up, dtheta) with the reference's numpy expressions."""
    if mode == "vertical":
        up, down = np.radians(fov[0]), np.radians(fov[1])
        return np.radians(45.), np.radians(90.0 / W), down, up, (up - down) / H
    return np.radians(45.), np.radians(90.0 / W), np.radians(2.), 0.0, np.radians(0.4 * 64.0 / H)


def exact_matrix(c2w, l2w):
    """[3,4] float64: inverse(lidar_to_world) @ cam_to_world of the float32 inputs."""
    return (np.linalg.inv(np.asarray(l2w, np.float32).astype(np.float64)) @ np.asarray(c2w, np.float32).astype(np.float64))[:3]


def scaled_intrinsics(K, downscale=1):
    """fx fy cx cy / downscale in double, rounded to float32 (the reference subtracts a Python float from a float32 tensor)."""
    return (np.asarray(K, np.float32)[:4].astype(np.float64) / float(downscale)).astype(np.float32)


def unproject(depth, K, max_depth=80.0):
    """depth [Hi,Wi] float32, K the scaled intrinsics -> (pc [n,3] float64 (0 where invalid), e_pc [n,3], valid [n]), n = Hi * Wi in
    linear pixel order."""
    d32 = np.asarray(depth, np.float32)
    Hi, Wi = d32.shape
    with np.errstate(invalid="ignore"):
        valid = ((d32 > 0) & (d32 < np.float32(max_depth))).reshape(-1)
    d = np.where(valid, d32.reshape(-1).astype(np.float64), 0.0)
    v, u = np.divmod(np.arange(Hi * Wi), Wi)
    fx, fy, cx, cy = [float(k) for k in K]
    pc = np.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], 1)
    e = gamma(3) * np.abs(pc)
    e[:, 2] = 0.0
    return pc, e, valid


def route_bounds(pc, e_pc, c2w, l2w):
    """-> (p [n,3] float64, e_dev [n,3], e_ref [n,3])."""
    import torch
    c2w64, l2w64 = np.asarray(c2w, np.float32).astype(np.float64), np.asarray(l2w, np.float32).astype(np.float64)
    M = exact_matrix(c2w, l2w)
    p = pc @ M[:, :3].T + M[:, 3]
    apc = np.abs(pc)
    M32 = M.astype(np.float32).astype(np.float64)
    A = np.abs(M32[:, :3])
    dM = np.abs(M32 - M) + U * np.abs(M32) + 1e-12      # (another float64 inverse may round an entry the other way)
    e_dev = e_pc @ A.T + gamma(4) * ((apc + e_pc) @ A.T + np.abs(M32[:, 3])) + apc @ dM[:, :3].T + dM[:, 3]
    Cw = np.abs(c2w64[:3, :3])
    w = pc @ c2w64[:3, :3].T + c2w64[:3, 3]
    e_w = e_pc @ Cw.T + gamma(4) * ((apc + e_pc) @ Cw.T + np.abs(c2w64[:3, 3]))
    inv64 = np.linalg.inv(l2w64)[:3]
    inv32 = torch.inverse(torch.from_numpy(np.array(l2w, np.float32))).numpy().astype(np.float64)[:3]
    Ai, dinv = np.abs(inv32[:, :3]), np.abs(inv32 - inv64)
    aw = np.abs(w)
    e_ref = e_w @ Ai.T + gamma(4) * ((aw + e_w) @ Ai.T + np.abs(inv32[:, 3])) + aw @ dinv[:, :3].T + dinv[:, 3]
    return p, e_dev * 1.01, e_ref * 1.01


def clamp_trunc(t, n):
    with np.errstate(invalid="ignore"):
        t = np.where(t >= 0, np.minimum(t, n - 1.0), 0.0)
    return t.astype(np.int64)


def angles(p):
    """p [n,3] float64 -> (azimuth asin(y / r), elevation asin(z / d), r, d, sy, sz)."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    d, r = np.sqrt((x * x + y * y) + z * z), np.sqrt(x * x + y * y)
    d, r = np.where(d == 0, 0.000001, d), np.where(r == 0, 0.000001, r)
    sy, sz = y / r, z / d
    return np.arcsin(sy), np.arcsin(sz), r, d, sy, sz


def asin_rounding(s):
    return 8 * UD / np.sqrt(np.maximum(1 - s * s - 16 * UD, 4 * UD)) + 8 * math.pi * UD


def edge_decided(t, et, n):
    """trunc(t) clamped to [0, n-1]: the edges are the integers 1 .. n-1.  -> (decided, lo, hi): the cells t +- et can give."""
    near = np.clip(np.round(t), 1, max(n - 1, 1))
    decided = (np.abs(t - near) > et) if n > 1 else np.ones(len(t), bool)
    big = 1e9
    lo = clamp_trunc(np.clip(np.nan_to_num(t - et, nan=-big, posinf=big, neginf=-big), -big, big), n)
    hi = clamp_trunc(np.clip(np.nan_to_num(t + et, nan=big, posinf=big, neginf=-big), -big, big), n)
    return decided, lo, hi


def bin_points(p, e, alive, H, W, slice=1, mode="vertical", fov=(10.0, -30.0), crop=CROP):
    """The binning of n candidates in index order.  p [n,3] float64 (the exact coordinates), e [n,3] (how far a float32 evaluation may
    lie from them; zeros: exact), alive [n] (the candidates that reach the crop at all: a valid depth).  -> dict: cell [n] (-1 dead),
    live [n], decided [n], winner [H*W] (-1 empty), dwinner [H*W] (the highest DECIDED live index), dirty [H*W], emitted [M] (the
    indices of the occupied kept beams in beam order), cells [M] (their cells)."""
    n = len(p)
    rad45, dphi, theta0, fov_up, dtheta = beam_constants(H, W, mode, fov)
    m = MARGIN * e
    if crop is None:
        inside, crop_dec = np.ones(n, bool), np.ones(n, bool)
    else:
        lo, hi = np.asarray(crop, np.float64)[0::2], np.asarray(crop, np.float64)[1::2]
        inside = np.all((p >= lo) & (p < hi), axis=1)
        crop_dec = np.all(((np.abs(p - lo) > m) & (np.abs(p - hi) > m)) | (e == 0), axis=1)
    az, el, r, d, sy, sz = angles(p)
    rho2, rho3 = MARGIN * np.hypot(e[:, 0], e[:, 1]), MARGIN * np.sqrt((e * e).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        e_az = np.where(rho2 < r, np.arcsin(np.minimum(rho2 / r, 1.0)), np.inf) + MARGIN * asin_rounding(sy)
        e_el = np.where(rho3 < d, np.arcsin(np.minimum(rho3 / d, 1.0)), np.inf) + MARGIN * asin_rounding(sz)
    tcol = (rad45 - az) / dphi
    col = clamp_trunc(tcol, W)
    col_dec, c_lo, c_hi = edge_decided(tcol, e_az / dphi + 4 * UD * np.abs(tcol), W)
    if mode == "vertical":
        in_fov = (el >= theta0) & (el <= fov_up)
        fov_dec = (np.abs(el - theta0) > e_el) & (np.abs(el - fov_up) > e_el)
        trow = (el - theta0) / dtheta
    else:
        in_fov, fov_dec = np.ones(n, bool), np.ones(n, bool)
        trow = (theta0 - el) / dtheta
    row = clamp_trunc(trow, H)
    row_dec, r_lo, r_hi = edge_decided(trow, e_el / dtheta + 4 * UD * np.abs(trow), H)
    live = alive & inside & in_fov
    decided = ~alive | (crop_dec & (~inside | (fov_dec & (~in_fov | (col_dec & row_dec)))))
    cell = np.where(live, row * W + col, -1)
    idx = np.arange(n)
    winner, dwinner = np.full(H * W, -1, np.int64), np.full(H * W, -1, np.int64)
    np.maximum.at(winner, cell[live], idx[live])
    dl = live & decided
    np.maximum.at(dwinner, cell[dl], idx[dl])
    dirty = np.zeros((H, W), bool)
    dw = dwinner.reshape(H, W)
    for i in np.nonzero(~decided)[0]:
        sub = dirty[r_lo[i]:r_hi[i] + 1, c_lo[i]:c_hi[i] + 1]
        sub |= dw[r_lo[i]:r_hi[i] + 1, c_lo[i]:c_hi[i] + 1] < i
    dirty = dirty.reshape(-1)
    kept = ((np.arange(H * W) // W) % slice == 0)
    cells = np.nonzero(kept & (winner >= 0))[0]
    return {"cell": cell, "live": live, "decided": decided, "winner": winner, "dwinner": dwinner, "dirty": dirty, "kept": kept,
            "emitted": winner[cells], "cells": cells, "H": H, "W": W}


def depth_reference(case, routes="both"):
    """The whole of depth_map_to_lidar_points for one camera of a case.  -> bin_points' dict plus p [n,3], e_dev, e_ref, valid.
    routes: "both" -- decided under the reference's route and the device's (what a recorded result needs); "device" -- under the
    device's alone (what a comparison of the device, or of the host shim, with this restatement needs)."""
    K = scaled_intrinsics(case["K"], case.get("downscale", 1))
    pc, e_pc, valid = unproject(case["depth"], K, case.get("max_depth", 80.0))
    p, e_dev, e_ref = route_bounds(pc, e_pc, case["c2w"], case["l2w"])
    ref = bin_points(p, np.maximum(e_dev, e_ref) if routes == "both" else e_dev, valid, case["H"], case["W"], case.get("slice", 1), case.get("mode", "vertical"),
                     case.get("fov", (10.0, -30.0)), case.get("crop", CROP))
    ref.update(p=p, e_dev=e_dev, e_ref=e_ref, valid=valid)
    return ref


def cloud_reference(case):
    """pto_ang_map / pto_ang_map_vertical / gen_sparse_points for a cloud [N,4] float32: exact coordinates."""
    x = np.asarray(case["cloud"], np.float32)
    p = x[:, :3].astype(np.float64)
    ref = bin_points(p, np.zeros_like(p), np.ones(len(p), bool), case["H"], case["W"], case.get("slice", 1), case.get("mode", "classic"),
                     case.get("fov", (10.0, -30.0)), case.get("crop", None))
    ref.update(p=p)
    return ref


def case_stats(ref):
    """(undecided live-or-alive pixels / live pixels, dirty occupied beams / occupied beams, live, occupied)."""
    alive = ref.get("valid", np.ones(len(ref["cell"]), bool))
    live, occ = int(ref["live"].sum()), int((ref["winner"] >= 0).sum())
    und = int((~ref["decided"] & alive).sum())
    dirty = int((ref["dirty"] & (ref["winner"] >= 0)).sum())
    return und / max(live, 1), dirty / max(occ, 1), live, occ


def compare(ref, points, count, source, bound=None, label=""):
    """What a float32 evaluation emitted (points [cap,3|4], count, source [cap]) against the restatement: the sources of the clean beams
    EQUAL and in beam order, every emitted coordinate within ``bound`` [n,3] (default e_dev) of its source pixel's.  Returns stats."""
    count = int(count)
    src = np.asarray(source)[:count].astype(np.int64)
    n = len(ref["cell"])
    assert count <= len(ref["kept"]) and np.all((src >= 0) & (src < n)), label
    assert len(np.unique(src)) == count, label
    dec = ref["decided"][src]
    assert np.all(ref["live"][src[dec]]), f"{label}: a decided dead pixel was emitted"
    cell = ref["cell"][src]
    keep = dec & ~ref["dirty"][np.maximum(cell, 0)]
    clean_cells = ref["kept"] & ~ref["dirty"] & (ref["dwinner"] >= 0)
    want = ref["dwinner"][clean_cells]
    assert np.array_equal(src[keep], want), f"{label}: winners of the clean beams differ ({keep.sum()} emitted, {len(want)} expected)"
    if not ref["dirty"].any() and ref["decided"].all():
        assert np.array_equal(src, ref["emitted"]) and np.all(np.diff(cell) > 0), label
    bound = ref["e_dev"] if bound is None else bound
    err = np.abs(np.asarray(points)[:count, :3].astype(np.float64) - ref["p"][src])
    assert np.all(err <= bound[src]), f"{label}: coordinates off by up to {(err / np.maximum(bound[src], 1e-300)).max():.2f} bounds"
    return {"emitted": count, "checked": int(keep.sum()), "worst_err_m": float(err.max()) if count else 0.0,
            "worst_err_in_bounds": float((err / np.maximum(bound[src], 1e-300)).max()) if count else 0.0}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def look_at(yaw, pitch, pos):
    """camera-to-parent [4,4] float64 of an OpenCV camera (z forward, x right, y down) looking along the yawed, pitched +x axis of a
    frame with z up."""
    fwd = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, pos
    return m


def street_case(seed, Hi=96, Wi=160, H=16, W=32, slice=1, yaw=0.0, mode="vertical", downscale=1, specials=True):
    """A street seen by a camera yawed ``yaw`` against the lidar (x forward, y left, z up; world translations up to +-300 m): ground,
    walls at both sides beyond the crop's height and the fov's upper limit, a wall ahead, boxes of constant depth, open sky (0), with
    2 % multiplicative noise so that neighbours fight over a beam; with ``specials`` also zeros, depths beyond max_depth, a NaN, an
    infinity and a negative depth."""
    g = np.random.default_rng(seed)
    f = Wi / 2 * g.uniform(0.9, 1.1)
    K = np.array([f, f * g.uniform(0.97, 1.03), Wi / 2 + g.uniform(-2, 2), Hi / 2 + g.uniform(-2, 2)]) * downscale
    lyaw = g.uniform(-math.pi, math.pi)
    l2w = np.eye(4)
    l2w[:2, :2] = [[math.cos(lyaw), -math.sin(lyaw)], [math.sin(lyaw), math.cos(lyaw)]]
    l2w[:3, 3] = [g.uniform(-300, 300), g.uniform(-300, 300), g.uniform(-5, 5)]
    l2w = l2w.astype(np.float32)
    c2l = look_at(yaw + g.uniform(-0.03, 0.03), g.uniform(-0.03, 0.03), [g.uniform(0.5, 1.5), g.uniform(-0.3, 0.3), g.uniform(-0.3, 0.1)])
    c2w = (l2w.astype(np.float64) @ c2l).astype(np.float32)
    Ks = scaled_intrinsics(K.astype(np.float32), downscale).astype(np.float64)
    v, u = np.divmod(np.arange(Hi * Wi), Wi)
    dirs = np.stack([(u - Ks[2]) / Ks[0], (v - Ks[3]) / Ks[1], np.ones(Hi * Wi)], 1) @ c2l[:3, :3].T
    o = c2l[:3, 3]
    t = np.full(Hi * Wi, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, plane in ((2, -1.7 + g.uniform(-0.1, 0.1)), (1, g.uniform(6, 9)), (1, -g.uniform(6, 9)), (0, g.uniform(60, 75))):
            s = (plane - o[axis]) / dirs[:, axis]
            t = np.where((s > 0) & (s < t), s, t)
    for _ in range(6):
        r0, c0 = int(g.integers(0, Hi - 8)), int(g.integers(0, Wi - 12))
        box = np.zeros((Hi, Wi), bool)
        box[r0:r0 + int(g.integers(4, Hi // 3)), c0:c0 + int(g.integers(6, Wi // 4))] = True
        t = np.where(box.reshape(-1), np.minimum(t, g.uniform(4, 45)), t)
    depth = np.where(np.isfinite(t), t * g.uniform(0.98, 1.02, Hi * Wi), 0.0)
    if specials:
        k = g.random(Hi * Wi)
        depth = np.where(k < 0.03, 0.0, np.where(k < 0.05, g.uniform(80.0, 200.0, Hi * Wi), depth))
        depth[g.integers(0, Hi * Wi, 3)] = [np.nan, np.inf, -3.0]
    return {"depth": depth.reshape(Hi, Wi).astype(np.float32), "K": K.astype(np.float32), "c2w": c2w, "l2w": l2w, "H": H, "W": W,
            "slice": slice, "mode": mode, "downscale": downscale}


def random_case(seed):
    return street_case(seed, **RANDOM_SHAPE, yaw=0.6 * ((seed % 3) - 1))


def cloud_case(seed, H=64, W=32, slice=1, mode="classic", crop=SPARSE_CROP):
    """A cloud with intensity: the lidar-frame points of a street's pixels and points spread beyond the crop."""
    g = np.random.default_rng(seed)
    s = street_case(seed, 40, 64, specials=False)
    pc, _, valid = unproject(s["depth"], scaled_intrinsics(s["K"]), 1e9)
    M = exact_matrix(s["c2w"], s["l2w"])
    a = (pc @ M[:, :3].T + M[:, 3])[valid]
    b = g.uniform([-10, -60, -3], [130, 60, 2], (600, 3))
    xyz = np.concatenate([a, b])[g.permutation(len(a) + len(b))]
    cloud = np.concatenate([xyz, g.random((len(xyz), 1))], 1).astype(np.float32)
    return {"cloud": cloud, "H": H, "W": W, "slice": slice, "mode": mode, "crop": crop}


def invalidate_undecided(case, ref):
    """The case without what the restatement cannot decide: a depth pixel set to 0, a cloud row dropped."""
    out = dict(case)
    if "depth" in case:
        d = case["depth"].copy().reshape(-1)
        d[~ref["decided"]] = 0.0
        out["depth"] = d.reshape(case["depth"].shape)
    else:
        out["cloud"] = case["cloud"][ref["decided"]]
    return out


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def golden_depth_case(name):
    z, spec = golden(), GOLDEN_DEPTH[name]
    return {"depth": z[f"{name}_depth"], "K": z[f"{name}_K"], "c2w": z[f"{name}_c2w"], "l2w": z[f"{name}_l2w"], "H": spec["H"],
            "W": spec["W"], "slice": spec.get("slice", 1), "mode": "vertical", "downscale": spec.get("downscale", 1)}


def golden_cloud_case():
    return {"cloud": golden()["cloud_points"], "H": GOLDEN_CLOUD["H"], "W": GOLDEN_CLOUD["W"], "slice": GOLDEN_CLOUD["slice"],
            "mode": "classic", "crop": SPARSE_CROP}
