"""The lidar scene preparation (bilateral_driving_amd/lidar.py, csrc/lidar.hip) on the CPU: the float64 restatement
(tests/lidar_ref64.py) against the reference's recorded results (tests/golden/lidar_prep.npz, scripts/gen_golden_lidar.py), the device
math on the host (tests/hostmath_lidar_shim.hip) against both, the new kernels' resources, and the C entries' signatures and argument
checks.

What is compared how.  Every golden point is DECIDED (lidar_ref64: no float32 rounding can move it across a pixel edge, an image
border, z = 0 or a box face), so the winner maps, pix, visible, inside and the (instance, frame, row) lists must be EQUAL and the
colours bit-equal; depths and box coordinates are held to the derived bound (gamma_4 times the sum of the dot product's magnitudes,
plus the float32 inverse's own distance from the float64 one for a box), twice that against the reference's float32 value.  Random
cases may leave out their undecided points and the pixels those can reach, at most 1 % of the points and 1 % of the occupied pixels
(asserted for the restatement alone here, for every seed the GPU test uses).  The downsampler is held to 4 ulp of the reference's value
(two divisions on each side of the last one may round differently), and the shim is in fact bit-equal to it; against the exact ratio
the bound is (n + 4) u for a window of n values: n - 1 additions and five divisions.

One test here needs nothing of the product: the check that every random seed stays within the cap runs on the restatement alone, as it
was asked for, and so also passes on a tree without the feature (the module still imports the product's binding and build modules)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from tests import lidar_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("shared", "sparse")


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


# ---- the restatement against the reference's recorded results -----------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_references_projection(name):
    z, case = R.golden(), R.golden_projection_case(name)
    ref = R.projection_reference(case)
    assert ref["decided"].all() and ref["decided_all"].all()
    occupied = collisions = 0
    for c, r in enumerate(ref["cams"]):
        gold = z[f"{name}_cam{c}_depth"]
        assert np.array_equal(r["winner"], z[f"{name}_cam{c}_winner"]) and r["clean"].all()
        assert np.all(np.abs(gold - r["depth"]) <= r["edepth"])
        lin = r["pix"][r["pix"] >= 0]
        occupied += len(np.unique(lin))
        collisions += int((np.bincount(lin) > 1).sum())
    assert np.array_equal(ref["visible"], z[f"{name}_visible"]) and np.array_equal(ref["visible_all"], z[f"{name}_visible_all"])
    assert np.array_equal(R.expected_colors(case, ref), R.from_u8(z[f"{name}_colors"]))
    print(f"\nlidar {name}: {len(case['points'])} points, {occupied} occupied pixels, {collisions} with collisions")
    assert collisions > occupied // 3      # heavy collisions
    # the cases hold what they were built to hold
    idx = R.closest_sweeps(case)
    if name == "shared":
        assert idx[1] == idx[2] and np.any(np.diff(case["timesteps"]) < 0)
        both = (ref["cams"][0]["pix"] >= 0) & (ref["cams"][1]["pix"] >= 0)
        assert both.sum() > 100      # two cameras seeing one point: the later camera's colour
        assert np.all(ref["color_src"][both, 0] == 1)
    else:
        assert list(idx) == [0, 1, 2] and not np.any(case["timesteps"] == 1)
        for r in ref["cams"]:
            assert np.all(r["winner"][1:] < 0)      # the empty sweep, and the one without a valid point
        assert (case["timesteps"] == 2).sum() > 1000
    M = R.case_views(case)[0][0][0]
    pr = R.project(M[:3], case["points"][case["timesteps"] == 0], case["cams"][0]["W"], case["cams"][0]["H"])
    with np.errstate(all="ignore"):
        q, _ = R.rows_with_bound(M[:3], case["points"][case["timesteps"] == 0])
        u, v = q[:, 0] / (q[:, 2] + R.EPS32), q[:, 1] / (q[:, 2] + R.EPS32)
    edge = (q[:, 2] > 0) & (((u > -1) & (u < 0)) | ((v > -1) & (v < 0)))
    assert edge.sum() >= 10 and not pr["valid"][edge].any()      # u, v in (-1, 0): truncation would give pixel 0, the test says no
    assert (q[:, 2] < 0).sum() > 500                              # points behind the camera


def test_restatement_equals_the_references_boxes():
    z, case = R.golden(), R.golden_box_case()
    F, I = case["active"].shape
    assert (F, I) == (R.BOX_F, R.BOX_I) and not case["active"][:, 3].any() and np.all(case["poses"][:, 3] == 0)
    for node_type in ("RigidNodes", "DeformableNodes"):
        ref = R.boxes(case["points"], case["poses"], case["sizes"], R.eligible_of(case, node_type), R.frame_ranges(case["timesteps"], F))
        assert ref["decided"].all()
        recs = np.array(ref["records"], np.int64).reshape(-1, 3)
        for i in z[f"box_{node_type}_full_keys"]:
            sel = recs[:, 0] == i
            want = z[f"box_{node_type}_full_{i}_pts"]
            assert len(want) == sel.sum() and np.all(np.abs(want - ref["o"][sel]) <= ref["eo"][sel])
        if node_type == "RigidNodes":
            rows, n = np.unique(recs[:, 2], return_counts=True)
            assert (n > 1).sum() > 20      # a point inside two overlapping boxes of one frame appears in both
    inst = set(int(i) for i in z["box_filter_instances"])
    ref = R.boxes(case["points"], case["poses"], case["sizes"], case["active"], None, inst)
    assert ref["decided"].all() and np.array_equal(ref["inside"], z["box_filter_inside"])
    assert list(z["box_DeformableNodes_full_keys"]) == [4, 5, 6] and len(z["box_DeformableNodes_full_5_pts"]) == 0      # the empty box
    assert list(z["box_DeformableNodes_sampled_keys"]) == [6] and list(z["box_RigidNodes_sampled_keys"]) == [0, 1, 2]


@pytest.mark.parametrize("k", range(len(R.DEPTH_CASES)))
def test_restatement_equals_the_references_downsampler(k):
    z = R.golden()
    H, W, factor = R.DEPTH_CASES[k]
    m, gold = z[f"depth{k}_map"], z[f"depth{k}_out"]
    assert m.shape == (H, W) and gold.shape == R.output_size(H, W, factor)
    f32, _ = R.downsample(m, factor, np.float32)
    exact, n = R.downsample(m, factor)
    assert np.array_equal(f32, gold)
    assert np.all(np.abs(gold - exact) <= (n + 4) * R.U * np.abs(exact) * 1.01)
    assert gold[0, 0] == 0 and ((m > 0) & (m <= R.HIT32)).sum() > 10      # a window with no hit; values in (0, 1e-3]
    if (H, W) == (25, 41):
        spans = [R.window(i, H, gold.shape[0]) for i in range(gold.shape[0])]
        assert sum(e - b for b, e in spans) > H      # uneven windows: H is no multiple of the output, so neighbours overlap


def test_every_random_seed_stays_within_the_cap_for_the_restatement_alone():
    worst = (0.0, 0.0)
    for seed in R.RANDOM_SEEDS:
        ref = R.projection_reference(R.random_projection_case(seed))
        und = float((~ref["decided"]).mean())
        occ = sum(int((r["winner"] >= 0).sum()) for r in ref["cams"])
        dirty = sum(int(((r["winner"] >= 0) & ~r["clean"]).sum()) for r in ref["cams"])
        worst = (max(worst[0], und), max(worst[1], dirty / max(occ, 1)))
        assert und <= R.CAP and dirty <= R.CAP * occ, (seed, und, dirty, occ)
    print(f"\nlidar random cases: at worst {worst[0]:.4%} of the points undecided, {worst[1]:.4%} of the occupied pixels dirty; cap {R.CAP:.0%}")
    assert len(R.RANDOM_SEEDS) == 20


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("lidar")
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    h.hm_lidar_project.argtypes = [vp, vp, ci, ci, vp, vp, vp]
    h.hm_lidar_views.argtypes = [ci, ci, ci, ll] + [vp] * 9
    h.hm_lidar_views.restype = None
    h.hm_lidar_visible.argtypes = [ll, vp, ci, vp, vp, vp]
    h.hm_lidar_visible.restype = None
    h.hm_lidar_boxes.argtypes = [ll, vp, ci, vp, vp, vp, vp, vp, ll, vp, vp]
    h.hm_lidar_boxes.restype = ll
    h.hm_lidar_window.argtypes = [ci, ci, ci, vp, vp]
    h.hm_lidar_downsample.argtypes = [ci, ci, ci, ci, vp, vp]
    h.hm_lidar_downsample.restype = None
    return h


def shim_launch(shim):
    def launch(x, mats, ranges, W, H, images, visible, colors):
        V, N = len(mats), len(x)
        depth, winner, pix = np.zeros((V, H, W), np.float32), np.zeros((V, H, W), np.int32), np.zeros(N, np.int32)
        images = np.ascontiguousarray(images)
        shim.hm_lidar_views(V, W, H, N, x.ctypes.data, mats.ctypes.data, ranges.ctypes.data, images.ctypes.data, winner.ctypes.data,
                            depth.ctypes.data, pix.ctypes.data, visible.ctypes.data, colors.ctypes.data)
        return depth, winner.astype(np.int64), pix.astype(np.int64)
    return launch


def test_host_projection_rounds_every_operation_on_its_own(shim):
    g = np.random.default_rng(0)
    for _ in range(2000):
        M = g.uniform(-30, 30, 12).astype(np.float32)
        p = g.uniform(-40, 40, 3).astype(np.float32)
        px, py, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
        ok = shim.hm_lidar_project(M.ctypes.data, p.ctypes.data, 40, 24, ctypes.byref(px), ctypes.byref(py), ctypes.byref(d))
        q = [((M[4 * r] * p[0] + M[4 * r + 1] * p[1]) + M[4 * r + 2] * p[2]) + M[4 * r + 3] for r in range(3)]      # float32, no FMA
        assert d.value == q[2]
        den = q[2] + np.float32(1e-6)
        with np.errstate(all="ignore"):
            u, v = q[0] / den, q[1] / den
        want = bool(u >= 0 and u < 40 and v >= 0 and v < 24 and q[2] > 0)
        assert bool(ok) == want
        if want:
            assert (px.value, py.value) == (int(u), int(v))
    M = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1], np.float32)      # u = x, v = y, z = 1 (den = 1 + 1e-6)
    for p, want in (((-0.5, 3.0, 0.0), 0), ((3.0, -0.5, 0.0), 0), ((0.0, 0.0, 0.0), 1), ((39.9, 23.9, 0.0), 1), ((40.1, 3.0, 0.0), 0),
                    ((3.0, 24.1, 0.0), 0), ((np.nan, 1.0, 0.0), 0)):
        p = np.array(p, np.float32)
        px, py, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
        assert shim.hm_lidar_project(M.ctypes.data, p.ctypes.data, 40, 24, ctypes.byref(px), ctypes.byref(py), ctypes.byref(d)) == want, p
    Mneg = M.copy()
    Mneg[11] = -1.0      # z = -1: u = -x > 0 would pass the image test, z > 0 does not
    p = np.array([-3.0, -3.0, 0.0], np.float32)
    px, py, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    assert shim.hm_lidar_project(Mneg.ctypes.data, p.ctypes.data, 40, 24, ctypes.byref(px), ctypes.byref(py), ctypes.byref(d)) == 0


@pytest.mark.parametrize("name", NAMES)
def test_host_projection_equals_the_reference(shim, name):
    case = R.golden_projection_case(name)
    got = R.run_projection(case, shim_launch(shim))
    stats = R.compare_projection_golden(name, got)
    print(f"\nlidar shim {name}: {stats}")
    z = R.golden()
    mats = np.ascontiguousarray(np.concatenate([m[:, :3, :] for m, _ in R.case_views(case)]))
    sizes = np.array([(cam["W"], cam["H"]) for cam in case["cams"] for _ in range(R.FRAMES)], np.int32)
    vis = np.zeros(len(case["points"]), np.uint8)
    shim.hm_lidar_visible(len(vis), case["points"].ctypes.data, len(mats), mats.ctypes.data, sizes.ctypes.data, vis.ctypes.data)
    assert np.array_equal(vis.astype(bool), z[f"{name}_visible_all"])


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:4])
def test_host_projection_matches_the_restatement_on_random_cases(shim, seed):
    case = R.random_projection_case(seed)
    stats = R.compare_projection(case, R.run_projection(case, shim_launch(shim)), label=f"seed {seed}")
    print(f"\nlidar shim seed {seed}: {stats}")


def test_host_boxes_equal_the_reference(shim):
    z, case = R.golden(), R.golden_box_case()
    F = case["active"].shape[0]
    pts = np.ascontiguousarray(case["points"])
    N = len(pts)
    for node_type in ("RigidNodes", "DeformableNodes"):
        eligible = R.eligible_of(case, node_type)
        w2o, half, ids = R.box_tables(case, eligible)
        ranges = np.ascontiguousarray(R.frame_ranges(case["timesteps"], F)[ids[:, 1]].astype(np.int64))
        inside = np.zeros(N, np.uint8)
        cap = 1 << 16
        rec_ids, rec_xyz = np.zeros((cap, 3), np.int32), np.zeros((cap, 3), np.float32)
        M = shim.hm_lidar_boxes(N, pts.ctypes.data, len(w2o), w2o.ctypes.data, half.ctypes.data, ranges.ctypes.data, ids.ctypes.data,
                                inside.ctypes.data, cap, rec_ids.ctypes.data, rec_xyz.ctypes.data)
        assert 0 < M < cap
        assert np.all(np.diff(rec_ids[:M, 2]) >= 0)      # emitted by row
        rec_ids, rec_xyz = R.order_records(rec_ids[:M], rec_xyz[:M], F)
        ref = R.compare_records(case, eligible, rec_ids, rec_xyz, exact=True)
        for i in z[f"box_{node_type}_full_keys"]:
            sel = rec_ids[:, 0] == i
            want = z[f"box_{node_type}_full_{i}_pts"]
            recs = np.array(ref["records"], np.int64).reshape(-1, 3)
            assert sel.sum() == len(want)
            assert np.all(np.abs(rec_xyz[sel].astype(np.float64) - want) <= 2 * ref["eo"][recs[:, 0] == i])
    inst = set(int(i) for i in z["box_filter_instances"])
    w2o, half, ids = R.box_tables(case, None, inst)
    assert len(w2o) > R.BOX_I and not np.any(ids[:, 0] == 3) and not np.any(ids[:, 0] == 6)
    inside = np.zeros(N, np.uint8)
    shim.hm_lidar_boxes(N, pts.ctypes.data, len(w2o), w2o.ctypes.data, half.ctypes.data, None, ids.ctypes.data, inside.ctypes.data, 0, None, None)
    assert np.array_equal(inside.astype(bool), z["box_filter_inside"])


def test_host_downsampler_equals_the_reference(shim):
    z = R.golden()
    for k, (H, W, factor) in enumerate(R.DEPTH_CASES):
        m, gold = np.ascontiguousarray(z[f"depth{k}_map"]), z[f"depth{k}_out"]
        Ho, Wo = R.output_size(H, W, factor)
        out = np.zeros((Ho, Wo), np.float32)
        shim.hm_lidar_downsample(H, W, Ho, Wo, m.ctypes.data, out.ctypes.data)
        worst = ulps(out, gold).max()
        print(f"\nlidar downsampler shim {H}x{W} x{factor}: worst difference from the reference {worst:.2f} ulp")
        assert np.array_equal(out == 0, gold == 0) and worst <= 4.0
        for n_in, n_out in ((H, Ho), (W, Wo), (1080, 540), (1080, 270), (1920, 480), (7, 3), (5, 5)):
            for i in range(n_out):
                s, e = ctypes.c_int(), ctypes.c_int()
                shim.hm_lidar_window(i, n_in, n_out, ctypes.byref(s), ctypes.byref(e))
                assert (s.value, e.value) == R.window(i, n_in, n_out) and 0 <= s.value < e.value <= n_in
                # F.interpolate(mode="area") is adaptive average pooling: its own index arithmetic, in float
                assert s.value == int(np.floor(np.float32(i * n_in) / np.float32(n_out)))
                assert e.value == int(np.ceil(np.float32((i + 1) * n_in) / np.float32(n_out)))


def test_host_downsampler_takes_a_scale_factor_above_one_as_torch_does(shim):
    """F.interpolate(mode="area") accepts any scale factor, and so does the reference's function; the same expression through torch on
    the host (this test's own restatement of it) against the shim, bit for bit."""
    for H, W, factor in ((24, 40, 1.5), (25, 41, 2.0), (17, 23, 1.0), (31, 29, 0.4)):
        m = np.ascontiguousarray(R.depth_case(7, H, W))
        t = torch.from_numpy(m)
        avg = torch.nn.functional.interpolate(t[None, None], scale_factor=factor, mode="area")[0, 0]
        hit = torch.nn.functional.interpolate((t > 1e-3).float()[None, None], scale_factor=factor, mode="area")[0, 0]
        want = torch.where(hit > 0, avg / hit, torch.zeros_like(avg)).numpy()
        Ho, Wo = R.output_size(H, W, factor)
        assert want.shape == (Ho, Wo)
        out = np.zeros((Ho, Wo), np.float32)
        shim.hm_lidar_downsample(H, W, Ho, Wo, m.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, want), (H, W, factor)
        assert np.array_equal(R.downsample(m, factor, np.float32)[0], want)


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_lidar_kernel_resources():
    res = {short_name(k): v for k, v in kernel_resources("lidar.hip").items()}
    want = ["lidar_points_kernel<0>", "lidar_points_kernel<1>", "lidar_resolve_kernel", "lidar_visible_kernel", "lidar_boxes_kernel<0>",
            "lidar_boxes_kernel<1>", "lidar_boxes_kernel<2>", "lidar_scan_kernel", "lidar_downsample_kernel"]
    assert sorted(res) == sorted(want), list(res)
    for k in want:
        print(f"\n{k}: occupancy {res[k]['Occupancy']} waves/SIMD, {res[k]['VGPRs']} VGPRs, LDS {res[k]['LDS Size']} bytes")
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["LDS Size"] <= 16 * 1024, (k, res[k])
        assert res[k]["Occupancy"] >= 8, (k, res[k])
    from bilateral_driving_amd import lidar
    assert res["lidar_visible_kernel"]["LDS Size"] == lidar.VIEW_CHUNK * (12 + 2) * 4
    assert res["lidar_boxes_kernel<0>"]["LDS Size"] == lidar.BOX_CHUNK * (16 + 2) * 4


def test_entries_resolve_with_the_declared_signatures():
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_lidar\w*", k)}
    assert sorted(decl) == ["bds_lidar_boxes_workspace_bytes", "bds_lidar_depth_downsample", "bds_lidar_points_in_boxes",
                            "bds_lidar_points_in_boxes_count", "bds_lidar_points_in_boxes_emit", "bds_lidar_project", "bds_lidar_visible"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    from bilateral_driving_amd import lidar
    for macro, value in (("BDS_LIDAR_VIEW_CHUNK", lidar.VIEW_CHUNK), ("BDS_LIDAR_BOX_CHUNK", lidar.BOX_CHUNK)):
        assert f"#define {macro} {value}\n" in hdr, macro
    assert lidar.MAX_ROWS == 2 ** 31 - 1 - 256
    assert (lidar.RIGID_NODES, lidar.SMPL_NODES, lidar.DEFORMABLE_NODES) == (R.RIGID, R.SMPL, R.DEFORMABLE)
    assert lib.bds_abi_version() == L.ABI_VERSION == 7 and "#define BDS_ABI_VERSION 7 " in hdr
    full = open(os.path.join(ROOT, "include", "bds.h")).read()      # each entry cites the reference lines it serves
    for cite in ("driving_dataset.py:644-727", ":576-603", ":341-354", ":521-536", "pixel_source.py:77-92"):
        assert cite in full, cite


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first
    big = 1 << 31

    def project(V=3, W=40, H=24, N=100, pts=p, M=p, rg=p, img=p, win=p, dep=p, pix=p, vis=p, col=p):
        return lib.bds_lidar_project(V, W, H, N, pts, M, rg, img, win, dep, pix, vis, col, None)
    assert project(V=0, N=0) == 0
    assert lib.bds_lidar_project(0, 0, 0, 0, *([None] * 10)) == 0
    for kw in (dict(V=-1), dict(N=-1), dict(N=big), dict(W=0), dict(H=0), dict(V=1 << 12, W=1 << 10, H=1 << 10), dict(pts=None), dict(M=None),
               dict(rg=None), dict(win=None), dict(dep=None), dict(pix=None), dict(vis=None), dict(img=None), dict(col=None), dict(pts=p + 2),
               dict(M=p + 1), dict(rg=p + 4), dict(win=p + 2), dict(dep=p + 2), dict(pix=p + 2), dict(col=p + 2), dict(img=p + 2)):
        assert project(**kw) == L.BDS_EINVAL, kw

    def visible(N=100, pts=p, V=3, M=p, sz=p, vis=p):
        return lib.bds_lidar_visible(N, pts, V, M, sz, vis, None)
    assert visible(N=0) == 0 and visible(N=0, pts=None, vis=None) == 0
    for kw in (dict(N=-1), dict(N=big), dict(V=-1), dict(pts=None), dict(vis=None), dict(M=None), dict(sz=None), dict(pts=p + 2), dict(M=p + 2),
               dict(sz=p + 2)):
        assert visible(**kw) == L.BDS_EINVAL, kw

    def mask(N=100, pts=p, B=5, w=p, h=p, rg=p, chunk=128, ins=p):
        return lib.bds_lidar_points_in_boxes(N, pts, B, w, h, rg, chunk, ins, None)
    assert mask(N=0) == 0 and mask(N=0, pts=None, ins=None) == 0
    for kw in (dict(N=-1), dict(N=big), dict(B=-1), dict(pts=None), dict(w=None), dict(h=None), dict(ins=None), dict(chunk=0), dict(chunk=129),
               dict(chunk=-1), dict(pts=p + 2), dict(w=p + 2), dict(h=p + 2), dict(rg=p + 4)):
        assert mask(**kw) == L.BDS_EINVAL, kw
    need = lib.bds_lidar_boxes_workspace_bytes(1000)
    assert need >= 1000 * 4 + 4 * 8 and lib.bds_lidar_boxes_workspace_bytes(0) == 0 and lib.bds_lidar_boxes_workspace_bytes(big) == 0
    assert lib.bds_lidar_boxes_workspace_bytes(-3) == 0

    def count(N=1000, pts=p, B=5, w=p, h=p, rg=p, chunk=128, total=p, ws=p, nb=1 << 40):
        return lib.bds_lidar_points_in_boxes_count(N, pts, B, w, h, rg, chunk, total, ws, nb, None)
    for kw in (dict(total=None), dict(total=p + 4), dict(ws=None), dict(ws=p + 8), dict(chunk=0), dict(N=-1), dict(w=None)):
        assert count(**kw) == L.BDS_EINVAL, kw
    assert count(nb=need - 1) == L.BDS_EWORKSPACE and count(nb=0) == L.BDS_EWORKSPACE

    def emit(N=1000, pts=p, B=5, w=p, h=p, rg=p, ids=p, chunk=128, ws=p, nb=1 << 40, cap=10, ri=p, rx=p):
        return lib.bds_lidar_points_in_boxes_emit(N, pts, B, w, h, rg, ids, chunk, ws, nb, cap, ri, rx, None)
    assert emit(N=0) == 0 and emit(B=0) == 0 and emit(cap=0) == 0
    for kw in (dict(cap=-1), dict(ids=None), dict(ri=None), dict(rx=None), dict(ws=None), dict(ws=p + 8), dict(ids=p + 2), dict(ri=p + 2),
               dict(rx=p + 2), dict(chunk=200)):
        assert emit(**kw) == L.BDS_EINVAL, kw
    assert emit(nb=need - 1) == L.BDS_EWORKSPACE

    def down(B=2, H=25, W=41, Ho=12, Wo=20, i=p, o=p):
        return lib.bds_lidar_depth_downsample(B, H, W, Ho, Wo, i, o, None)
    assert down(B=0) == 0 and down(Ho=0) == 0 and down(Wo=0) == 0
    for kw in (dict(B=-1), dict(H=0), dict(W=0), dict(Ho=-1), dict(Wo=-1), dict(i=None), dict(o=None), dict(i=p + 2), dict(o=p + 2),
               dict(B=1 << 12, H=1 << 10, W=1 << 10, Ho=4, Wo=4), dict(B=2, Ho=1 << 16, Wo=1 << 16)):
        assert down(**kw) == L.BDS_EINVAL, kw


def test_python_checks_arguments_and_refuses_cpu_tensors():
    from bilateral_driving_amd import lidar
    import bilateral_driving_amd
    assert bilateral_driving_amd.lidar is lidar
    x, M = torch.rand(10, 3), torch.rand(2, 3, 4)
    with pytest.raises(L.BdsError):
        lidar.project_points(x, M, torch.tensor([[0, 5], [5, 10]]), 40, 24)
    with pytest.raises(L.BdsError):
        lidar.visible_from(x, M, (40, 24))
    with pytest.raises(L.BdsError):
        lidar.points_in_boxes(x, torch.eye(4).expand(2, 3, 4, 4), torch.ones(3, 3), torch.ones(2, 3, dtype=torch.bool))
    with pytest.raises(L.BdsError):
        lidar.downsample_sparse_depth(torch.rand(24, 40), 0.5)
    for bad in (torch.rand(10, 2), torch.rand(10), torch.rand(2, 5, 3)):
        with pytest.raises(ValueError):
            lidar.project_points(bad, M, torch.zeros(2, 2), 40, 24)
        with pytest.raises(ValueError):
            lidar.visible_from(bad, M, (40, 24))
    with pytest.raises(ValueError):
        lidar.downsample_sparse_depth(torch.rand(4), 0.5)
    for factor in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            lidar.downsample_sparse_depth(torch.rand(24, 40), factor)
    assert lidar.output_size(25, 41, 0.5) == (12, 20) and lidar.output_size(25, 41, 0.25) == (6, 10) and lidar.output_size(1080, 1920, 0.25) == (270, 480)
    # the box tables: active boxes only, (frame, instance) order, no inverse of an inactive pose
    case = R.golden_box_case()
    w2o, half, ids = lidar.box_tables(torch.from_numpy(case["poses"]), torch.from_numpy(case["sizes"]), torch.from_numpy(case["active"]))
    want = R.box_tables(case)
    assert np.array_equal(w2o.numpy(), want[0]) and np.array_equal(half.numpy(), want[1]) and np.array_equal(ids.numpy(), want[2])
    assert len(w2o) == int(case["active"].sum()) and half.dtype == torch.float32
    sub = lidar.box_tables(torch.from_numpy(case["poses"]), torch.from_numpy(case["sizes"]), torch.from_numpy(case["active"]), instances=[1, 2])
    assert set(sub[2][:, 0].tolist()) == {1, 2}
    with pytest.raises(ValueError):
        lidar.box_tables(torch.zeros(2, 3, 4, 4), torch.ones(4, 3), torch.ones(2, 3, dtype=torch.bool))
    # the camera matrices: the reference's own formation on the host
    pc = R.golden_projection_case("shared")
    cam = R.BareCamera(pc["cams"][0], "cpu")
    formed = np.stack([R.lidar2img32(pc["cams"][0]["intrinsics"][f], pc["cams"][0]["c2w"][f]) for f in range(R.FRAMES)])
    assert np.array_equal(lidar.camera_matrices(cam).numpy(), formed)      # (on one host: bit for bit)
    # undistortion is refused before anything touches a device
    d = R.bare_projection_dataset(pc, "cpu")
    d.pixel_source.camera_data[1].undistort = True
    with pytest.raises(NotImplementedError):
        lidar.project_lidar_pts_on_images(d)
    with pytest.raises(ValueError):
        lidar.get_init_objects(d, "SMPLNodes")
    # install / uninstall
    class DD:
        def get_init_objects(self):
            return "former"
    mod = types.ModuleType("pixel_source")
    former = DD.__dict__["get_init_objects"]
    lidar.install(DD, mod)
    lidar.install(DD)      # (twice: the former method is still the one remembered)
    for name in ("project_lidar_pts_on_images", "get_init_objects", "filter_pts_in_boxes", "check_pts_visibility"):
        assert DD.__dict__[name] is getattr(lidar, name)
    assert mod.sparse_lidar_map_downsampler is lidar.sparse_lidar_map_downsampler
    lidar.uninstall()
    assert DD.__dict__["get_init_objects"] is former and "check_pts_visibility" not in DD.__dict__
    assert not hasattr(mod, "sparse_lidar_map_downsampler")
