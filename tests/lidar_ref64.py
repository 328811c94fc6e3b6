"""Float64 restatement of the lidar scene preparation (bilateral_driving_amd/lidar.py, csrc/lidar.hip), with a rigorous bound on what
float32 may change, the test cases, and a bare dataset object for the reference-named wrappers.  Test infrastructure only.

The bound.  With u = 2^-24 and gamma_4 = 4u / (1 - 4u), a float32 dot product of three terms plus a constant, in any order and with or
without fused multiply-add, is within gamma_4 * (|m0 x| + |m1 y| + |m2 z| + |m3|) of the exact value for the same float32 inputs.
The projection divides: den = fl(z + 1e-6f) carries e_den = e_z (1 + u) + u |den|, and the quotient
    e_u = (e_x + |u| e_den) / (|den| - e_den) * (1 + 2u) + 2u |u|.
For a box the inverse itself is a float32 result: |inv32 - inv64| |[p;1]| is added, inv64 the float64 inverse of the float32 pose.

A point is DECIDED in a view when no such error can change what the view does with it: z is farther than MARGIN e_z from 0 and,
where z > 0, u is either beyond a border by more than MARGIN e_u or farther than that from every integer, v likewise.  A point is
decided for a box when on some axis it is outside by more than MARGIN e_o, or inside by more than that on all three.  A pixel is
CLEAN when no undecided point of its view can land in it (the rectangle of pixels that u +- MARGIN e_u, v +- MARGIN e_v reaches)."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lidar_prep.npz")
U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)
MARGIN = 4.0
EPS32 = float(np.float32(1e-6))
HIT32 = float(np.float32(1e-3))
CAMERAS = ((24, 40), (17, 23))      # (H, W) of the two cameras
FRAMES = 3
SWEEP = 4000
BOX_F, BOX_I = 5, 7
RIGID, SMPL, DEFORMABLE = 0, 1, 2


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def rows_with_bound(M, p):
    """M [3,4] (any float), p [n,3] float32 -> (q [n,3] float64, e [n,3]): M [p;1] exactly and gamma_4 times the sum of magnitudes."""
    M, p = np.asarray(M, np.float64), np.asarray(p, np.float64)
    q = p @ M[:, :3].T + M[:, 3]
    return q, GAMMA4 * (np.abs(p) @ np.abs(M[:, :3]).T + np.abs(M[:, 3]))


def _axis(u, eu, size):
    """-> (inside, pixel, decided) of one image axis."""
    m = MARGIN * eu
    out = (u < -m) | (u > size + m)
    inside = (u >= 0) & (u < size)
    frac = np.abs(u - np.round(u))
    return inside, np.floor(np.where(inside, u, 0)).astype(np.int64), out | (inside & (frac > m))


def project(M, p, W, H, dM=None):
    """One view.  dM [3,4]: how far the matrix itself may lie from the one given, entry by entry (another host's float32 inverse);
    |dM| |[p;1]| is added to the bound.  -> dict: valid [n], px, py, z (float64), ez, decided [n], reach (x0, x1, y0, y1: the pixels an undecided point may
    land in, clipped; empty where it can land nowhere)."""
    q, e = rows_with_bound(M, p)
    if dM is not None:
        e = e + np.concatenate([np.abs(np.asarray(p, np.float64)), np.ones((len(p), 1))], axis=1) @ np.asarray(dM, np.float64).T
    z, ez = q[:, 2], e[:, 2]
    den = z + EPS32
    eden = ez * (1 + U) + U * np.abs(den)
    safe = np.maximum(np.abs(den) - eden, 1e-300)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, v = q[:, 0] / den, q[:, 1] / den
        eu = (e[:, 0] + np.abs(u) * eden) / safe * (1 + 2 * U) + 2 * U * np.abs(u)
        ev = (e[:, 1] + np.abs(v) * eden) / safe * (1 + 2 * U) + 2 * U * np.abs(v)
    behind = z < -MARGIN * ez - MARGIN * eden
    front = (z > MARGIN * ez) & (np.abs(den) > MARGIN * eden)
    fin = np.isfinite(u) & np.isfinite(v) & np.isfinite(eu) & np.isfinite(ev)
    u, v = np.where(fin, u, -1e30), np.where(fin, v, -1e30)
    eu, ev = np.where(fin, eu, np.inf), np.where(fin, ev, np.inf)
    inx, px, dx = _axis(u, eu, W)
    iny, py, dy = _axis(v, ev, H)
    outx, outy = dx & ~inx, dy & ~iny
    decided = behind | (front & (outx | outy | (dx & dy)))
    valid = (z > 0) & inx & iny
    big = 1e9
    x0 = np.clip(np.floor(np.maximum(u - MARGIN * eu, -big)), 0, W).astype(np.int64)
    x1 = np.clip(np.floor(np.minimum(u + MARGIN * eu, big)) + 1, 0, W).astype(np.int64)
    y0 = np.clip(np.floor(np.maximum(v - MARGIN * ev, -big)), 0, H).astype(np.int64)
    y1 = np.clip(np.floor(np.minimum(v + MARGIN * ev, big)) + 1, 0, H).astype(np.int64)
    return {"valid": valid, "px": px, "py": py, "z": z, "ez": ez, "decided": decided, "reach": (x0, x1, y0, y1)}


def project_views(mats, points, ranges, W, H, dmats=None):
    """V views of one camera.  mats [V,3|4,4], points [N,3], ranges [V,2].  -> dict: winner [V,H,W] int64 (the highest valid row, -1),
    depth [V,H,W] float64, edepth [V,H,W], pix [N] (of the last view that sees the point, -1), visible [N], decided [N] (in every view
    that takes the point), clean [V,H,W]."""
    mats = np.asarray(mats)[:, :3, :]
    V, N = len(mats), len(points)
    winner = np.full((V, H, W), -1, np.int64)
    depth, edepth = np.zeros((V, H, W)), np.zeros((V, H, W))
    clean = np.ones((V, H, W), bool)
    pix, decided = np.full(N, -1, np.int64), np.ones(N, bool)
    for v in range(V):
        b, e = int(ranges[v][0]), int(ranges[v][1])
        if e <= b:
            continue
        r = project(mats[v], points[b:e], W, H, None if dmats is None else dmats[v])
        rows = np.arange(b, e)
        decided[b:e] &= r["decided"]
        ok = r["valid"]
        lin = r["py"][ok] * W + r["px"][ok]
        flat = winner[v].reshape(-1)
        np.maximum.at(flat, lin, rows[ok])
        pix[rows[ok]] = v * H * W + lin
        x0, x1, y0, y1 = r["reach"]
        for k in np.nonzero(~r["decided"])[0]:
            clean[v, y0[k]:y1[k], x0[k]:x1[k]] = False
        occupied = flat >= 0
        local = flat[occupied] - b
        depth[v].reshape(-1)[occupied] = r["z"][local]
        edepth[v].reshape(-1)[occupied] = r["ez"][local]
    return {"winner": winner, "depth": depth, "edepth": edepth, "pix": pix, "visible": pix >= 0, "decided": decided, "clean": clean}


def visible_any(mats, sizes, points, dmats=None):
    """check_pts_visibility.  -> (visible [N], decided [N]); sizes [V,2] = (W, H)."""
    vis, dec = np.zeros(len(points), bool), np.ones(len(points), bool)
    for v, (M, (W, H)) in enumerate(zip(np.asarray(mats)[:, :3, :], sizes)):
        r = project(M, points, int(W), int(H), None if dmats is None else dmats[v])
        vis |= r["valid"]
        dec &= r["decided"]
    return vis, dec


def inverse_with_bound(pose32):
    """-> (inv64 [3,4], |inv32 - inv64| [3,4]) of a float32 pose: the float64 inverse and how far torch's float32 inverse on the host
    (what the reference and the product's wrapper call) lies from it."""
    import torch
    inv64 = np.linalg.inv(np.asarray(pose32, np.float64))[:3]
    inv32 = torch.linalg.inv(torch.from_numpy(np.array(pose32, np.float32))).numpy().astype(np.float64)[:3]
    return inv64, np.abs(inv32 - inv64)


def in_box(pose32, size32, points):
    """-> (inside [n], o [n,3] float64, eo [n,3], decided [n]) of one oriented box."""
    inv64, dinv = inverse_with_bound(pose32)
    o, e = rows_with_bound(inv64, points)
    p1 = np.concatenate([np.abs(np.asarray(points, np.float64)), np.ones((len(points), 1))], axis=1)
    eo = e * (1 + 2 * U) + p1 @ (dinv * (1 + GAMMA4)).T
    half = (np.asarray(size32, np.float32) / np.float32(2)).astype(np.float64)
    inside = np.all((o > -half) & (o < half), axis=1)
    m = MARGIN * eo
    out = np.any(np.abs(o) > half + m, axis=1)
    firm_in = np.all(np.abs(o) < half - m, axis=1)
    return inside, o, eo, out | firm_in


def boxes(points, poses, sizes, active, frame_ranges=None, instances=None):
    """Every active (frame, instance) box against the rows of its range (None: all).  -> dict: inside [N] (the OR), decided [N],
    records [(instance, frame, row)] ordered so, o [M,3] float64 and eo [M,3] in that order."""
    F, I = active.shape
    N = len(points)
    inside_any, decided = np.zeros(N, bool), np.ones(N, bool)
    recs = []
    for i in range(I):
        if instances is not None and i not in instances:
            continue
        for f in range(F):
            if not active[f, i]:
                continue
            b, e = (0, N) if frame_ranges is None else (int(frame_ranges[f][0]), int(frame_ranges[f][1]))
            if e <= b:
                continue
            ins, o, eo, dec = in_box(poses[f, i], sizes[i], points[b:e])
            inside_any[b:e] |= ins
            decided[b:e] &= dec
            for k in np.nonzero(ins)[0]:
                recs.append((i, f, b + int(k), o[k], eo[k]))
    return {"inside": inside_any, "decided": decided, "records": [(r[0], r[1], r[2]) for r in recs],
            "o": np.array([r[3] for r in recs]).reshape(-1, 3), "eo": np.array([r[4] for r in recs]).reshape(-1, 3)}


def window(i, n_in, n_out):
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def output_size(H, W, factor):
    return int(math.floor(H * factor)), int(math.floor(W * factor))


def downsample(depth_map, factor, dtype=np.float64):
    """sparse_lidar_map_downsampler for [H,W].  float64: the exact ratio sum / cnt of the float32 values; float32: every sum and every
    division rounded, in the order the kernels take them.  -> (out [Ho,Wo], n [Ho,Wo] the window sizes)."""
    a = np.asarray(depth_map, np.float32).astype(dtype)
    H, W = a.shape
    Ho, Wo = output_size(H, W, factor)
    out, n = np.zeros((Ho, Wo), dtype), np.zeros((Ho, Wo), np.int64)
    for i in range(Ho):
        r0, r1 = window(i, H, Ho)
        for j in range(Wo):
            c0, c1 = window(j, W, Wo)
            s, cnt = dtype(0), dtype(0)
            for v in a[r0:r1, c0:c1].reshape(-1):
                s = dtype(s + v)
                cnt = dtype(cnt + (1 if v > HIT32 else 0))
            kh, kw = dtype(r1 - r0), dtype(c1 - c0)
            n[i, j] = (r1 - r0) * (c1 - c0)
            if cnt > 0:
                out[i, j] = dtype(dtype(dtype(s / kh) / kw) / dtype(dtype(cnt / kh) / kw))
    return out, n


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def q8(g, shape):
    """Random colours on the 8-bit grid k / 255 in float32 (the goldens keep them as bytes)."""
    return from_u8(g.integers(0, 256, shape, dtype=np.uint8))


def from_u8(b):
    return b.astype(np.float32) / np.float32(255)


def to_u8(c):
    b = np.round(np.asarray(c, np.float64) * 255).astype(np.uint8)
    assert np.array_equal(from_u8(b), c)
    return b


def look_at(yaw, pitch, pos):
    """camera-to-world [4,4] float32 of an OpenCV camera (z forward, x right, y down) looking along the yawed, pitched +x axis."""
    fwd = np.array([math.cos(yaw) * math.cos(pitch), math.sin(yaw) * math.cos(pitch), math.sin(pitch)])
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, pos
    return c2w.astype(np.float32)


def lidar2img32(K, c2w):
    """pad(K) @ inverse(c2w) in float32 through torch on the host, as the reference forms it (driving_dataset.py:681-685)."""
    import torch
    K4 = torch.nn.functional.pad(torch.from_numpy(np.asarray(K, np.float32)), (0, 1, 0, 1))
    K4[3, 3] = 1.0
    return (K4 @ torch.from_numpy(np.asarray(c2w, np.float32)).inverse()).numpy()


def lidar2img_bound(K, c2w):
    """[4,4]: how far a float32 pad(K) @ inverse(c2w) may lie from the exact product.  A float32 inverse by LU carries a NORMWISE error:
    every entry within about c n u cond(A) max|inv| of the exact one (c n = 16 for n = 4), however small the entry itself; the 4-term
    products add gamma_4 of their magnitudes."""
    K4 = np.zeros((4, 4))
    K4[:3, :3], K4[3, 3] = np.asarray(K, np.float64), 1.0
    A = np.asarray(c2w, np.float64)
    inv = np.abs(np.linalg.inv(A))
    return np.abs(K4).sum(1, keepdims=True) * (16 * U * np.linalg.cond(A, np.inf) * inv.max()) + GAMMA4 * (np.abs(K4) @ inv)


def projection_case(seed, variant="shared", shuffle=False, sweep=SWEEP):
    """A scene of two cameras x FRAMES frames and four lidar sweeps.  variant "shared": frames 1 and 2 take the same sweep; "sparse":
    sweep 1 has no point and sweep 2 no valid one (all behind both cameras).  shuffle: the cloud's rows are not grouped by timestep.
    Every sweep has points behind the cameras and points planted at u, v in (-1, 0) of camera 0; both cameras see the points ahead."""
    g = np.random.default_rng(seed)
    sweep_times = np.array([0.0, 0.3, 0.6, 1.0], np.float32)
    frame_times = np.array([0.02, 0.33, 0.35] if variant == "shared" else [0.02, 0.31, 0.62], np.float32)
    cams = []
    for c, (H, W) in enumerate(CAMERAS):
        Ks, c2ws = [], []
        for f in range(FRAMES):
            fx = W * g.uniform(0.55, 0.7)
            Ks.append(np.array([[fx, 0, W / 2 + g.uniform(-1, 1)], [0, fx * g.uniform(0.95, 1.05), H / 2 + g.uniform(-1, 1)], [0, 0, 1]], np.float32))
            c2ws.append(look_at(0.25 * c + 0.05 * f + g.uniform(-0.02, 0.02), g.uniform(-0.05, 0.05), [0.8 * f + 0.3 * c, 0.2 * c, 1.5 + 0.1 * f]))
        cams.append({"H": H, "W": W, "intrinsics": np.stack(Ks), "c2w": np.stack(c2ws),
                     "images": q8(g, (FRAMES, H, W, 3))})
    pts, ts = [], []
    for t in range(4):
        n = sweep if t < 3 else sweep // 8      # (no frame takes sweep 3: check_pts_visibility alone sees it)
        if variant == "sparse" and t == 1:
            continue
        p = g.uniform([-25, -20, -1], [35, 20, 6], (n, 3))
        if variant == "sparse" and t == 2:
            p[:, 0], p[:, 1] = -np.abs(p[:, 0]) - 3.0, 0.1 * p[:, 1]      # behind both cameras, whichever frame looks
        else:
            K, c2w = cams[0]["intrinsics"][min(t, FRAMES - 1)].astype(np.float64), cams[0]["c2w"][min(t, FRAMES - 1)].astype(np.float64)
            m = 40
            uv = np.stack([g.uniform(-0.95, -0.05, m), g.uniform(-0.95, cams[0]["H"], m)], 1)      # u in (-1, 0)
            uv[m // 2:] = np.stack([g.uniform(-0.95, cams[0]["W"], m - m // 2), g.uniform(-0.95, -0.05, m - m // 2)], 1)      # v in (-1, 0)
            d = g.uniform(3, 20, m)
            cam_pts = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * d, (uv[:, 1] - K[1, 2]) / K[1, 1] * d, d], 1)
            p[:m] = cam_pts @ c2w[:3, :3].T + c2w[:3, 3]
        pts.append(p)
        ts.append(np.full(len(p), t, np.int64))
    pts, ts = np.concatenate(pts).astype(np.float32), np.concatenate(ts)
    if shuffle:
        order = g.permutation(len(pts))
        pts, ts = pts[order], ts[order]
    return {"cams": cams, "points": pts, "timesteps": ts, "sweep_times": sweep_times, "frame_times": frame_times,
            "colors0": q8(g, (len(pts), 3))}


def closest_sweeps(case):
    return np.abs(case["sweep_times"][None, :] - case["frame_times"][:, None]).argmin(1)


def grouped(case):
    """-> (perm, offsets [T+1]): the stable sort of the rows by timestep and the sweeps' row ranges in the sorted cloud."""
    perm = np.argsort(case["timesteps"], kind="stable")
    return perm, np.searchsorted(case["timesteps"][perm], np.arange(len(case["sweep_times"]) + 1))


def case_views(case):
    """-> per camera (mats [F,4,4] float32, ranges [F,2]) in the SORTED cloud.  A golden case carries the reference's own recorded
    matrices (the bits of a float32 inverse depend on the host that forms it; the recorded results belong to the recorded matrices)."""
    _, offsets = grouped(case)
    idx = closest_sweeps(case)
    ranges = np.stack([offsets[idx], offsets[idx + 1]], 1)
    return [(cam["lidar2img"] if "lidar2img" in cam else np.stack([lidar2img32(cam["intrinsics"][f], cam["c2w"][f]) for f in range(FRAMES)]),
             ranges) for cam in case["cams"]]


def case_dmats(case):
    """Per camera [F,3,4]: how far another host's float32 pad(K) @ inverse(c2w) may lie from the case's matrices -- both within
    lidar2img_bound of the exact product."""
    return [np.stack([2 * lidar2img_bound(cam["intrinsics"][f], cam["c2w"][f])[:3] for f in range(FRAMES)]) for cam in case["cams"]]


def projection_reference(case, matrix_margin=False):
    """The whole of project_lidar_pts_on_images for a case, in the cloud's ORIGINAL row order.  matrix_margin: the bounds (and with
    them ``decided``, ``clean``, ``edepth``) also allow for matrices formed on another host (case_dmats): what a result computed from
    locally formed matrices is held to against results recorded elsewhere.  -> dict: per camera the project_views
    dict with winner / pix mapped to original rows (``cams``), visible [N], color_src [N] = (camera, linear pixel) of the colour a
    point ends with or (-1, -1), decided [N], and check_pts_visibility's (visible_all, decided_all)."""
    perm, _ = grouped(case)
    x = case["points"][perm]
    N = len(x)
    decided, visible = np.ones(N, bool), np.zeros(N, bool)
    src = np.full((N, 2), -1, np.int64)
    out = []
    dm = case_dmats(case) if matrix_margin else [None] * len(case["cams"])
    for c, ((mats, ranges), cam) in enumerate(zip(case_views(case), case["cams"])):
        r = project_views(mats, x, ranges, cam["W"], cam["H"], dm[c])
        decided &= r["decided"]
        visible |= r["visible"]
        seen = r["pix"] >= 0
        src[seen, 0], src[seen, 1] = c, r["pix"][seen]
        r["winner"] = np.where(r["winner"] >= 0, perm[np.maximum(r["winner"], 0)], -1)
        for k in ("pix", "visible", "decided"):
            back = np.empty_like(r[k])
            back[perm] = r[k]
            r[k] = back
        out.append(r)

    def unsort(a):
        b = np.empty_like(a)
        b[perm] = a
        return b
    mats_all = np.concatenate([m for m, _ in case_views(case)])
    sizes = [(cam["W"], cam["H"]) for cam in case["cams"] for _ in range(FRAMES)]
    vis_all, dec_all = visible_any(mats_all, sizes, case["points"], np.concatenate(dm) if matrix_margin else None)
    return {"cams": out, "visible": unsort(visible), "color_src": unsort(src), "decided": unsort(decided), "visible_all": vis_all,
            "decided_all": dec_all}


def expected_colors(case, ref):
    col = case["colors0"].copy()
    for c, cam in enumerate(case["cams"]):
        rows = np.nonzero(ref["color_src"][:, 0] == c)[0]
        col[rows] = cam["images"].reshape(-1, 3)[ref["color_src"][rows, 1]]
    return col


def rotation(g, tilt=0.1):
    yaw, pitch, roll = g.uniform(-math.pi, math.pi), g.uniform(-tilt, tilt), g.uniform(-tilt, tilt)
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def box_case(seed, sweep=1200, planted=70):
    """BOX_F frames x BOX_I instances and one sweep per frame.  Instance 3 is never active (its poses are zero matrices, which no
    inverse may touch), 1 and 2 overlap, 5 lies where no point is, 4 stands still (only_moving drops it), 0 is active in every frame
    with the most points; types: 0-3 rigid, 4-5 deformable, 6 SMPL.  Frame 3 has an empty sweep."""
    g = np.random.default_rng(seed)
    F, I = BOX_F, BOX_I
    sizes = np.stack([g.uniform([3.5, 1.6, 1.4], [5.0, 2.2, 2.0]) for _ in range(I)]).astype(np.float32)
    poses = np.zeros((F, I, 4, 4), np.float32)
    active = g.random((F, I)) > 0.3
    active[:, 0], active[:, 3], active[:, 4] = True, False, True
    active[1:3, 1] = active[1:3, 2] = True
    active[0, 5] = True
    start = g.uniform([-12, -12, 0.5], [12, 12, 1.5], (I, 3))
    vel = g.uniform(-1.5, 1.5, (I, 3)) * [1, 1, 0]
    vel[4] = 0
    R0 = [rotation(g) for _ in range(I)]
    for f in range(F):
        for i in range(I):
            if i == 3:
                continue
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R0[i], start[i] + vel[i] * f
            if i == 2:
                T[:3, :3], T[:3, 3] = R0[1], start[1] + vel[1] * f + [0.6, 0.3, 0.0]
            if i == 5:
                T[:3, 3] = [150.0 + f, 150.0, 40.0]
            poses[f, i] = T
    pts, ts = [], []
    for f in range(F):
        if f == 3:
            continue
        p = [g.uniform([-15, -15, -1], [15, 15, 4], (sweep, 3))]
        for i in range(I):
            if active[f, i] and i != 5:
                n = planted * (3 if i == 0 else 1)
                local = g.uniform(-0.5, 0.5, (n, 3)) * sizes[i].astype(np.float64) * 1.15      # some just outside
                p.append(local @ poses[f, i, :3, :3].astype(np.float64).T + poses[f, i, :3, 3])
        p = np.concatenate(p)
        p = p[g.permutation(len(p))]
        pts.append(p)
        ts.append(np.full(len(p), f, np.int64))
    pts, ts = np.concatenate(pts).astype(np.float32), np.concatenate(ts)
    types = np.array([RIGID, RIGID, RIGID, RIGID, DEFORMABLE, DEFORMABLE, SMPL], np.int64)
    return {"points": pts, "timesteps": ts, "poses": poses, "sizes": sizes, "active": active, "types": types,
            "colors": q8(g, (len(pts), 3))}


def interleave_sweeps(case, seed):
    """The case with its rows no longer grouped by timestep but every sweep's rows still in their order (so a stable regrouping gives
    back the grouped cloud exactly).  -> (case, slot [N]: where each original row went)."""
    g = np.random.default_rng(seed)
    ts = case["timesteps"]
    slots, slot = g.permutation(len(ts)), np.empty(len(ts), np.int64)
    for t in np.unique(ts):
        idx = np.nonzero(ts == t)[0]
        slot[idx] = np.sort(slots[idx])
    out = dict(case)
    for k in ("points", "timesteps", "colors0", "colors"):
        if k in case:
            a = np.empty_like(case[k])
            a[slot] = case[k]
            out[k] = a
    return out, slot


def frame_ranges(timesteps, F):
    """[F,2] row ranges of a cloud whose rows are grouped by timestep."""
    off = np.searchsorted(timesteps, np.arange(F + 1))
    return np.stack([off[:-1], off[1:]], 1)


def depth_case(seed, H, W):
    """A sparse depth map: a third of the pixels hit, a 7x9 corner without a hit, values in (0, 1e-3] among the hits."""
    g = np.random.default_rng(seed)
    m = np.where(g.random((H, W)) < 0.33, g.uniform(0.5, 80.0, (H, W)), 0.0).astype(np.float32)
    m[:7, :9] = 0
    tiny = g.random((H, W)) < 0.05
    m[tiny] = g.uniform(1e-5, 1e-3, int(tiny.sum())).astype(np.float32)
    m[:7, :9] = 0
    m[8, 8] = np.float32(1e-3)
    return m


DEPTH_CASES = ((25, 41, 0.5), (25, 41, 0.25), (24, 40, 0.5))


def keep_decided(case, decided):
    """The case without its undecided rows."""
    out = dict(case)
    for k in ("points", "timesteps", "colors0", "colors"):
        if k in case:
            out[k] = case[k][decided]
    return out


# ---- the goldens ----------------------------------------------------------------------------------------------------------------------
_GOLD = {}


def golden():
    if not _GOLD:
        with np.load(GOLDEN) as z:
            _GOLD.update({k: z[k] for k in z.files})
    return _GOLD


def golden_projection_case(name):
    """The recorded inputs of projection case ``name`` in the form ``projection_case`` returns."""
    z = golden()
    cams = [{"H": int(z[f"{name}_cam{c}_hw"][0]), "W": int(z[f"{name}_cam{c}_hw"][1]), "intrinsics": z[f"{name}_cam{c}_intrinsics"],
             "c2w": z[f"{name}_cam{c}_c2w"], "images": from_u8(z[f"{name}_cam{c}_images"]), "lidar2img": z[f"{name}_cam{c}_lidar2img"]} for c in range(len(CAMERAS))]
    return {"cams": cams, "points": z[f"{name}_points"], "timesteps": z[f"{name}_timesteps"], "sweep_times": z[f"{name}_sweep_times"],
            "frame_times": z[f"{name}_frame_times"], "colors0": from_u8(z[f"{name}_colors0"])}


def golden_box_case():
    z = golden()
    out = {k: z[f"box_{k}"] for k in ("points", "timesteps", "poses", "sizes", "active", "types", "colors")}
    out["colors"] = from_u8(out["colors"])
    return out


# ---- a bare dataset for the reference-named wrappers ----------------------------------------------------------------------------------
class BareCamera:
    def __init__(self, cam, device):
        import torch
        self.HEIGHT, self.WIDTH, self.undistort, self.cam_name = cam["H"], cam["W"], False, "cam"
        self.intrinsics = torch.from_numpy(cam["intrinsics"]).to(device)
        self.cam_to_worlds = torch.from_numpy(cam["c2w"]).to(device)
        self.images = torch.from_numpy(cam["images"]).to(device)
        self.lidar_depth_maps = None

    def __len__(self):
        return len(self.intrinsics)

    def load_depth(self, maps):
        self.lidar_depth_maps = maps


class BareLidar:
    """origins + directions * ranges = the case's points (origins 0, directions the points, ranges 1)."""

    def __init__(self, points, timesteps, sweep_times, colors, device):
        import torch
        self.origins = torch.zeros(len(points), 3, device=device)
        self.directions = torch.from_numpy(points).to(device)
        self.ranges = torch.ones(len(points), 1, device=device)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.unique_normalized_timestamps = torch.from_numpy(sweep_times).to(device)
        self.colors = torch.from_numpy(colors).to(device)
        self.visible_masks = torch.zeros(len(points), dtype=torch.bool, device=device)
        self.deleted = None

    def delete_invisible_pts(self):
        keep = self.visible_masks
        self.deleted = int((~keep).sum())
        self.origins, self.directions, self.ranges = self.origins[keep], self.directions[keep], self.ranges[keep]
        self.timesteps, self.colors, self.visible_masks = self.timesteps[keep], self.colors[keep], None


class Bare:
    pass


def bare_projection_dataset(case, device):
    import torch
    d, ps = Bare(), Bare()
    d.device, d.pixel_source = device, ps
    d.lidar_source = BareLidar(case["points"], case["timesteps"], case["sweep_times"], case["colors0"], device)
    ps.camera_data = {c: BareCamera(cam, device) for c, cam in enumerate(case["cams"])}
    ps.normalized_time = torch.from_numpy(case["frame_times"]).to(device)
    return d


def bare_box_dataset(case, device):
    import torch
    d, ps = Bare(), Bare()
    d.device, d.pixel_source, d.type = device, ps, "Waymo"
    d.frame_num, d.instance_num = case["active"].shape
    d.lidar_source = BareLidar(case["points"], case["timesteps"], np.linspace(0, 1, BOX_F).astype(np.float32), case["colors"], device)
    ps.per_frame_instance_mask = torch.from_numpy(case["active"]).to(device)
    ps.instances_model_types = torch.from_numpy(case["types"]).to(device)
    ps.instances_pose = torch.from_numpy(case["poses"]).to(device)
    ps.instances_size = torch.from_numpy(case["sizes"]).to(device)
    ps.instances_true_id = torch.arange(case["active"].shape[1], device=device) + 100
    ps.smpl_human_all = {106: {}}
    return d


# ---- comparisons shared by the CPU (host shim) and the GPU tests ----------------------------------------------------------------------
CAP = 0.01      # at most this share of the points / of the occupied pixels may be left out of a comparison with the restatement
RANDOM_SEEDS = tuple(range(1000, 1020))


def random_projection_case(seed):
    return projection_case(seed, ("shared", "sparse")[seed % 2], shuffle=seed % 4 < 2, sweep=SWEEP)


def run_projection(case, launch):
    """project_lidar_pts_on_images through ``launch(points, mats [F,3,4], ranges [F,2], W, H, images, visible u8, colors)`` ->
    (depth, winner, pix), which updates visible / colors in place: the rows grouped by one stable sort, one launch per camera, the
    results mapped back to the cloud's row order.  -> {"cams": [{"depth", "winner", "pix"}], "visible", "colors"}."""
    perm, _ = grouped(case)
    x = np.ascontiguousarray(case["points"][perm])
    visible = np.zeros(len(x), np.uint8)
    colors = np.ascontiguousarray(case["colors0"][perm])
    cams = []
    for (mats, ranges), cam in zip(case_views(case), case["cams"]):
        depth, winner, pix = launch(x, np.ascontiguousarray(mats[:, :3, :]), np.ascontiguousarray(ranges.astype(np.int64)), cam["W"],
                                    cam["H"], cam["images"], visible, colors)
        back = np.empty_like(pix)
        back[perm] = pix
        cams.append({"depth": depth, "winner": np.where(winner >= 0, perm[np.maximum(winner, 0)], -1), "pix": back})
    vis, col = np.empty_like(visible), np.empty_like(colors)
    vis[perm], col[perm] = visible, colors
    return {"cams": cams, "visible": vis.astype(bool), "colors": col}


def compare_projection(case, got, exact=False, label=""):
    """``got`` (run_projection's form) against the restatement.  exact: every point must be decided (the goldens); otherwise the
    undecided points and the pixels they can reach are left out, at most CAP of each (asserted)."""
    ref = projection_reference(case)
    dec = ref["decided"]
    n_und = int((~dec).sum())
    assert n_und <= (0 if exact else CAP * len(dec)), (label, n_und, len(dec))
    occupied = dirty = 0
    for c, (r, g) in enumerate(zip(ref["cams"], got["cams"])):
        clean = r["clean"]
        occupied += int((r["winner"] >= 0).sum())
        dirty += int(((r["winner"] >= 0) & ~clean).sum())
        assert np.array_equal(g["winner"][clean], r["winner"][clean]), (label, c)
        assert g["depth"].dtype == np.float32 and np.all(g["depth"][clean & (r["winner"] < 0)] == 0), (label, c)
        assert np.all(np.abs(g["depth"].astype(np.float64) - r["depth"])[clean] <= r["edepth"][clean]), (label, c)
        ok = r["decided"]
        assert np.array_equal(g["pix"][ok], r["pix"][ok]), (label, c)
    assert dirty <= (0 if exact else CAP * occupied), (label, dirty, occupied)
    assert np.array_equal(got["visible"][dec], ref["visible"][dec]), label
    assert np.array_equal(got["colors"][dec], expected_colors(case, ref)[dec]), label      # bit-equal
    return {"undecided": n_und, "points": len(dec), "dirty": dirty, "occupied": occupied}


def compare_projection_golden(name, got):
    """``got`` for the golden case ``name`` against the reference's recorded results."""
    z = golden()
    for c, g in enumerate(got["cams"]):
        gold = z[f"{name}_cam{c}_depth"]
        assert np.array_equal(g["winner"], z[f"{name}_cam{c}_winner"]), (name, c)
        assert np.array_equal(g["depth"] > 0, gold > 0), (name, c)
    assert np.array_equal(got["visible"], z[f"{name}_visible"])
    assert np.array_equal(got["colors"], from_u8(z[f"{name}_colors"]))
    case = golden_projection_case(name)
    ref = projection_reference(case)
    worst = 0.0
    for c, g in enumerate(got["cams"]):
        assert np.all(np.abs(g["depth"].astype(np.float64) - z[f"{name}_cam{c}_depth"]) <= 2 * ref["cams"][c]["edepth"]), (name, c)
        for f in range(FRAMES):      # this host's float32 pad(K) @ inverse(c2w) against the recorded one: each within the bound of the exact
            K, c2w = case["cams"][c]["intrinsics"][f], case["cams"][c]["c2w"][f]
            diff = np.abs(lidar2img32(K, c2w).astype(np.float64) - z[f"{name}_cam{c}_lidar2img"][f])
            worst = max(worst, float((diff / lidar2img_bound(K, c2w)).max()))
    print(f"lidar {name}: this host's lidar2img against the recorded one, worst difference / bound {worst:.3f} (allowed 2)")
    assert worst <= 2.0, (name, worst)
    return compare_projection(case, got, exact=True, label=name)


def box_tables(case, eligible=None, instances=None):
    """The active boxes' tables as the product's wrapper forms them: one batched float32 inverse on the host, (frame, instance) order."""
    import torch
    active = case["active"] if eligible is None else eligible
    if instances is not None:
        active = active & np.isin(np.arange(active.shape[1]), sorted(instances))[None]
    f, i = np.nonzero(active)
    w2o = torch.linalg.inv(torch.from_numpy(case["poses"][f, i])).numpy()[:, :3, :] if len(f) else np.zeros((0, 3, 4), np.float32)
    return np.ascontiguousarray(w2o), np.ascontiguousarray((case["sizes"] / np.float32(2))[i]), np.stack([i, f], 1).astype(np.int32)


def order_records(rec_ids, rec_xyz, F):
    order = np.argsort(rec_ids[:, 0].astype(np.int64) * F + rec_ids[:, 1], kind="stable")
    return rec_ids[order], rec_xyz[order]


def compare_records(case, eligible, rec_ids, rec_xyz, exact=False):
    """The emit form's ordered records against the restatement (frame f tests its own sweep)."""
    F = case["active"].shape[0]
    ref = boxes(case["points"], case["poses"], case["sizes"], eligible, frame_ranges(case["timesteps"], F))
    und = ~ref["decided"]
    assert und.sum() <= (0 if exact else CAP * len(und))
    want = np.array(ref["records"], np.int64).reshape(-1, 3)
    keep_w, keep_g = ~und[want[:, 2]], ~und[rec_ids[:, 2]]
    assert np.array_equal(rec_ids[keep_g], want[keep_w])
    assert np.all(np.abs(rec_xyz[keep_g].astype(np.float64) - ref["o"][keep_w]) <= ref["eo"][keep_w])
    return ref


def eligible_of(case, node_type):
    rigid = case["types"] == RIGID
    return case["active"] & (rigid if node_type == "RigidNodes" else ~rigid)[None]
