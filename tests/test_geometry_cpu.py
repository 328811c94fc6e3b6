"""Evaluation geometry metrics (bilateral_driving_amd/geometry.py, csrc/geometry.hip) on the CPU: the restatement
(tests/geometry_ref64.py) against known answers, the device math on the host (tests/hostmath_geometry_shim.hip) against that
restatement, the new kernels' resources, and the C entries' signatures and argument checks.

The shim's frame is held to twice the float32 restatement's own error against float64 plus geometry_ref64.FLOOR.  The floor was
measured here, over every case of geometry_ref64.CASES and every scalar and distance array (the test prints each figure): the shim
rounds the same quantities as the float32 restatement in another order (fused multiply-adds in the unprojection and the pair, double
sums), so where the restatement happens to be nearly exact it stands ABOVE twice the restatement's error -- by 5.687e-07 at the worst
(n513_without_egocar chamfer_dynamic: restatement 3.572e-07, shim 1.283e-06; that frame's lidar returns under the ego car lie tens of
metres from the render, so its values are large), by 4.6e-07 and 3.9e-07 for the next two (its chamfer_95 and cham_pred_95), by 1.9e-07
on the validity-edge frame's abs_err trims, and by at most 6.1e-08 on every other case.  FLOOR is the worst figure rounded up to the
next power of ten, 1e-6.  With a camera 10^3 m from the origin (case "far") the restatement's own error, and with it the bound, grows
to 1.9e-3 on the distances, and the shim's equals it."""
import ctypes
import math
import re
import types

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from tests import geometry_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources, short_name


# ---- the restatement against known answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_depths_give_zero_everywhere(dtype):
    pred, gt, masks, _ = R.make_frame(24, 40, 200)
    K, c2w = R.camera(24, 40)
    f = R.frame(gt, gt, K, c2w, masks, None, dtype)
    assert f["valid"] == 200 and np.all(f["dist_pred"] == 0) and np.all(f["dist_gt"] == 0)
    for k in R.SCALARS:
        assert f[k] == 0.0 or (math.isnan(f[k]) and f[f"{k[8:]}_valid"] == 0), k


def test_isolated_returns_with_a_depth_offset_have_the_closed_form():
    """Lidar pixels spaced far apart, pred = gt + delta: every point's nearest neighbour is its own pixel's, delta * |ray| away."""
    H, W, delta = 33, 47, 0.125
    K, c2w = R.camera(H, W)
    gt = np.zeros((H, W), np.float32)
    gt[2::10, 3::10] = 20.0
    pred = np.where(gt > 0, gt + delta, 0).astype(np.float32)
    f = R.frame(pred, gt, K, c2w, {}, None, np.float64)
    v, u = np.nonzero(gt)
    ray2 = ((u - K[0, 2]) / np.float64(K[0, 0])) ** 2 + ((v - K[1, 2]) / np.float64(K[1, 1])) ** 2 + 1
    want = delta ** 2 * ray2
    assert f["valid"] == len(v) == 20 and np.abs(f["dist_pred"] - want).max() < 1e-9 and np.abs(f["dist_gt"] - want).max() < 1e-9
    assert abs(f["chamfer"] - 2 * want.mean()) < 1e-9 and abs(f["depth_err"] - delta) < 1e-12
    assert abs(f["depth_err_median_squared"] - delta ** 2) < 1e-12 and abs(f["depth_err_rmse_95"] - delta) < 1e-12
    assert abs(f["cham_pred_95"] - np.sort(want)[:19].mean()) < 1e-9
    assert f["background_valid"] == 20 and abs(f["chamfer_background"] - f["chamfer"]) < 1e-12 and math.isnan(f["chamfer_sky"])


def test_validity_edges_and_classes_of_the_restatement():
    pred, gt, ok = R.edge_frame()
    assert np.array_equal(R.valid_mask(pred, gt), ok) and ok.sum() == 9
    ego = np.zeros(ok.shape, np.uint8)
    ego[4] = 2
    assert R.valid_mask(pred, gt, ego).sum() == 6
    inp, r64, _ = R.case("empty_human")
    assert r64["human_valid"] == 0 and math.isnan(r64["chamfer_human"]) and "chamfer_human" not in R.reference_frame(r64)
    assert r64["dynamic_valid"] > r64["vehicle_valid"] > 0      # (dynamic pixels of neither subclass)
    assert sum(r64[f"{c}_valid"] for c in ("sky", "dynamic", "background")) == r64["valid"]
    _, one, _ = R.case("one_vehicle")
    assert one["vehicle_valid"] == 1 and one["sky_valid"] == 1 and one["chamfer_vehicle"] > 0
    _, big, _ = R.case("n513")
    assert 0 < big["human_valid"] < big["dynamic_valid"] == big["human_valid"] + big["vehicle_valid"]


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("geometry")
    vp = ctypes.c_void_p
    h.hm_geo_unproject.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, vp, vp, vp]
    h.hm_geo_trim_count.argtypes = [ctypes.c_longlong, ctypes.c_int]
    h.hm_geo_trim_count.restype = ctypes.c_longlong
    h.hm_geo_flags.argtypes = [ctypes.c_float, ctypes.c_float] + [ctypes.c_int] * 5
    h.hm_geo_flags.restype = ctypes.c_uint
    h.hm_geo_pair.argtypes = [ctypes.c_int, vp, vp]
    h.hm_geo_pair.restype = ctypes.c_float
    h.hm_geo_select.argtypes = [vp, ctypes.c_longlong, ctypes.c_longlong, vp]
    h.hm_geo_frame.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 12
    h.hm_geo_frame.restype = ctypes.c_longlong
    return h


def test_host_trim_count_is_pythons_int_of_the_product(shim):
    ns = list(range(1, 4097)) + [(1 << 21) + d for d in (-3, -1, 0, 1, 2, 99, 100, 101)] + [1 << 24]
    for w, q in enumerate((0.99, 0.97, 0.95)):
        assert [shim.hm_geo_trim_count(n, w) for n in ns] == [int(n * q) for n in ns]
    assert shim.hm_geo_trim_count(0, 0) == 0 and shim.hm_geo_trim_count(1, 2) == 0 and shim.hm_geo_trim_count(20, 2) == 19


def test_host_flags_at_the_validity_edges(shim):
    pred, gt, ok = R.edge_frame()
    got = np.array([[shim.hm_geo_flags(float(p), float(g), 0, 0, 0, 0, 0) for p, g in zip(pr, gr)] for pr, gr in zip(pred, gt)])
    assert np.array_equal(got != 0, ok) and set(got[ok]) == {1 | 32}                 # valid, background
    assert shim.hm_geo_flags(5.0, 5.0, 1, 0, 0, 0, 0) == 0                           # under the ego car
    assert shim.hm_geo_flags(5.0, 5.0, 0, 0, 1, 1, 0) == (1 | 4 | 8)                # human inside dynamic: both, not background
    assert shim.hm_geo_flags(5.0, 5.0, 0, 1, 0, 0, 1) == (1 | 2 | 16) and shim.hm_geo_flags(0.0, 5.0, 0, 1, 1, 1, 1) == 0


@pytest.mark.parametrize("translation", [(5.0, -3.0, 1.5), (1000.0, -800.0, 30.0)])
def test_host_unprojection_matches_float64_element_by_element(shim, translation):
    H, W = 24, 40
    K, c2w = R.camera(H, W, translation)
    depth = np.random.default_rng(5).uniform(0.5, 79.0, (H, W)).astype(np.float32)
    r64, r32 = (R.unproject(depth, K, c2w, np.ones((H, W), bool), d) for d in (np.float64, np.float32))
    got = np.zeros((H * W, 3), np.float32)
    Kc, Cc = np.ascontiguousarray(K), np.ascontiguousarray(c2w)
    for i in range(H * W):
        shim.hm_geo_unproject(i % W, i // W, float(depth.flat[i]), Kc.ctypes.data, Cc.ctypes.data, got[i].ctypes.data)
    # per element: half an ulp of the result for the final rounding plus an ulp of each of the three terms' sizes
    tol = 4 * np.finfo(np.float32).eps * (np.abs(r64).max() + 80.0 * 2)
    err, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    print(f"\nunprojection at {translation}: float32 restatement {e32:.3e}, shim {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol and e32 <= tol


def test_host_select_and_trimmed_sums_match_a_sort(shim):
    g = np.random.default_rng(11)
    arrays = [g.uniform(0, 3, 1000).astype(np.float32), np.zeros(37, np.float32), np.array([0.5], np.float32),
              np.repeat(g.uniform(0, 1, 9).astype(np.float32), 23),                       # ties
              np.concatenate([np.zeros(50, np.float32), g.uniform(0, 1e-30, 50).astype(np.float32), [np.float32(np.inf)]]),
              (g.integers(0, 4, 513) * np.float32(0.25)).astype(np.float32)]               # zeros and ties
    for a in arrays:
        a = np.ascontiguousarray(g.permutation(a))
        s = np.sort(a).astype(np.float64)
        for k in sorted({1, 2, len(a) // 2, (len(a) - 1) // 2 + 1, int(len(a) * 0.95), int(len(a) * 0.99), len(a)}):
            if not 1 <= k <= len(a):
                continue
            out = np.zeros(4)
            shim.hm_geo_select(a.ctypes.data, len(a), k, out.ctypes.data)
            assert out[2] == k and out[3] == s[k - 1], (len(a), k)
            want, want2 = s[:k].sum(), np.square(s[:k]).sum()
            if np.isfinite(want):
                assert abs(out[0] - want) <= 1e-12 * max(want, 1e-300) and abs(out[1] - want2) <= 1e-12 * max(want2, 1e-300), (len(a), k)
            else:
                assert out[0] == want and out[1] == want2


def test_host_pair_is_the_squared_or_the_absolute_distance(shim):
    a, b = np.array([1000.5, -800.25, 30.0], np.float32), np.array([1000.25, -800.0, 31.0], np.float32)
    assert shim.hm_geo_pair(2, a.ctypes.data, b.ctypes.data) == 0.0625 + 0.0625 + 1.0      # exact: no |x|^2 + |y|^2 - 2 x.y
    assert shim.hm_geo_pair(1, a.ctypes.data, b.ctypes.data) == 1.5


def shim_frame(shim, inp):
    H, W = inp["pred"].shape
    u8 = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in [inp["egocar"]] + [inp["masks"].get(k) for k in R.MASK_KEYS]]
    row, dp, dg = np.zeros(32), np.zeros(H * W, np.float32), np.zeros(H * W, np.float32)
    K, c2w = np.ascontiguousarray(inp["K"]), np.ascontiguousarray(inp["c2w"])
    n = shim.hm_geo_frame(H, W, inp["pred"].ctypes.data, inp["gt"].ctypes.data, *[None if m is None else m.ctypes.data for m in u8],
                          K.ctypes.data, c2w.ctypes.data, row.ctypes.data, dp.ctypes.data, dg.ctypes.data)
    return n, row, dp[:n], dg[:n]


def test_host_math_frame_matches_float64_within_the_bound(shim):
    from bilateral_driving_amd.geometry import ROW_SLOTS
    worst = (-math.inf, None)
    for name in R.CASES:
        inp, r64, r32 = R.case(name)
        n, row, dp, dg = shim_frame(shim, inp)
        assert n == r64["valid"] == row[ROW_SLOTS["valid"]]
        for c in R.CLASSES:
            assert row[ROW_SLOTS[f"{c}_valid"]] == r64[f"{c}_valid"], (name, c)
        got = {k: row[ROW_SLOTS[k]] for k in R.SCALARS}
        got["dist_pred"], got["dist_gt"] = dp, dg
        for k in R.SCALARS + ("dist_pred", "dist_gt"):
            bound, e32 = R.bound(r64, r32, k)
            err = R.error(got[k], r64, k)
            print(f"geometry shim {name} {k}: float32 restatement {e32:.3e}, bound {bound:.3e}, shim {err:.3e}, excess {err - 2 * e32:.3e}")
            worst = max(worst, (err - 2 * e32, f"{name} {k}"))
            assert err <= bound, (name, k, err, bound)
    print(f"\ngeometry shim: worst excess over twice the float32 restatement's error {worst[0]:.3e} ({worst[1]}); FLOOR {R.FLOOR:.1e}")
    assert worst[0] <= R.FLOOR


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_geometry_kernel_resources():
    res = {short_name(k): v for k, v in kernel_resources("geometry.hip").items()}
    want = ("geo_flag_kernel", "geo_scan_kernel", "geo_scatter_kernel", "geo_nn_kernel<1>", "geo_nn_kernel<2>", "geo_select_kernel",
            "geo_finish_kernel")
    assert sorted(res) == sorted(want), list(res)
    for k in want:
        print(f"\n{k}: occupancy {res[k]['Occupancy']} waves/SIMD, {res[k]['VGPRs']} VGPRs, LDS {res[k]['LDS Size']} bytes")
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert 0 < res[k]["LDS Size"] <= 64 * 1024, (k, res[k])
        assert res[k]["Occupancy"] >= 4, (k, res[k])


def test_entries_resolve_with_the_declared_signatures():
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_geometry_metrics\w*|bds_depth_unproject|bds_chamfer_nn", k)}
    assert sorted(decl) == ["bds_chamfer_nn", "bds_depth_unproject", "bds_geometry_metrics", "bds_geometry_metrics_workspace_bytes"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    from bilateral_driving_amd import geometry
    for macro, value in (("BDS_GEOMETRY_METRICS_ROW", geometry.ROW), ("BDS_GEOMETRY_QUERY_BLOCK", geometry.QUERY_BLOCK),
                         ("BDS_GEOMETRY_TARGET_TILE", geometry.TARGET_TILE)):
        assert f"#define {macro} {value}\n" in hdr, macro
    assert sorted(geometry.ROW_SLOTS.values()) == list(range(geometry.ROW))
    assert lib.bds_abi_version() == L.ABI_VERSION == 7 and "#define BDS_ABI_VERSION 7 " in hdr


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first

    def run(H=17, W=23, pred=p, gt=p, ego=None, masks=(None,) * 4, kind=0, K=p, c2w=p, row=p, dp=None, dg=None, ws=p, nb=1 << 40):
        return lib.bds_geometry_metrics(H, W, pred, gt, ego, *masks, kind, K, c2w, row, dp, dg, ws, nb, None)

    def unproject(H=17, W=23, depth=p, mask=None, kind=0, K=p, c2w=p, points=p, count=p, ws=p, nb=1 << 40):
        return lib.bds_depth_unproject(H, W, depth, mask, kind, K, c2w, points, count, ws, nb, None)

    for H, W in ((0, 23), (17, 0), (-1, 23), (1 << 12, (1 << 12) + 1), (1 << 30, 1 << 30)):
        assert run(H=H, W=W) == L.BDS_EINVAL and unproject(H=H, W=W) == L.BDS_EINVAL, (H, W)
        assert lib.bds_geometry_metrics_workspace_bytes(H, W) == 0, (H, W)
    for name in ("pred", "gt", "K", "c2w", "row", "ws"):
        assert run(**{name: None}) == L.BDS_EINVAL, name
    for name in ("pred", "gt", "K", "c2w"):
        assert run(**{name: p + 2}) == L.BDS_EINVAL, name
    assert run(row=p + 4) == L.BDS_EINVAL and run(ws=p + 8) == L.BDS_EINVAL and run(kind=2) == L.BDS_EINVAL and run(kind=-1) == L.BDS_EINVAL
    assert run(dp=p) == L.BDS_EINVAL and run(dg=p) == L.BDS_EINVAL and run(dp=p + 2, dg=p) == L.BDS_EINVAL      # one without the other
    assert run(masks=(None, p + 1, None, None), kind=1) == L.BDS_EINVAL and run(ego=p + 2, kind=1) == L.BDS_EINVAL   # misaligned float masks
    need = lib.bds_geometry_metrics_workspace_bytes(17, 23)
    assert need >= 17 * 23 * 57 and run(nb=need - 1) == L.BDS_EWORKSPACE and unproject(nb=need - 1) == L.BDS_EWORKSPACE
    assert lib.bds_geometry_metrics_workspace_bytes(1280, 1920) >= 1280 * 1920 * 57
    for name in ("depth", "K", "c2w", "points", "count", "ws"):
        assert unproject(**{name: None}) == L.BDS_EINVAL, name
    assert unproject(count=p + 4) == L.BDS_EINVAL and unproject(points=p + 1) == L.BDS_EINVAL and unproject(kind=3) == L.BDS_EINVAL
    assert unproject(mask=p + 2, kind=1) == L.BDS_EINVAL

    def nn(P1=5, P2=7, x=p, y=p, norm=2, dx=p, dy=p):
        return lib.bds_chamfer_nn(P1, P2, x, y, norm, dx, dy, None)
    assert nn(P1=-1) == L.BDS_EINVAL and nn(P2=1 << 31) == L.BDS_EINVAL and nn(norm=0) == L.BDS_EINVAL and nn(norm=3) == L.BDS_EINVAL
    for name in ("x", "y", "dx", "dy"):
        assert nn(**{name: None}) == L.BDS_EINVAL and nn(**{name: p + 1}) == L.BDS_EINVAL, name
    assert nn(P1=0, P2=0, x=None, y=None, dx=None, dy=None) == L.BDS_OK      # nothing to do: no launch


def test_python_checks_shapes_and_refuses_cpu_tensors():
    from bilateral_driving_amd import geometry
    d, K, c2w = torch.rand(17, 23) + 1, torch.eye(3), torch.eye(4)
    infos, cams = {"lidar_depth_map": d}, {"intrinsics": K, "camera_to_world": c2w}
    with pytest.raises(L.BdsError):
        geometry.geometry_metrics(d, d, K, c2w)
    with pytest.raises(L.BdsError):
        geometry.frame_geometry(d, infos, cams)
    with pytest.raises(L.BdsError):
        geometry.depth_map_to_point_cloud(d, K, c2w)
    with pytest.raises(L.BdsError):
        geometry.chamfer_distance(torch.rand(5, 3), torch.rand(7, 3))
    for norm in (0, 3, 2.5):
        with pytest.raises(ValueError):
            geometry.chamfer_distance(torch.rand(5, 3), torch.rand(7, 3), norm=norm)
    for x, y in ((torch.rand(5, 2), torch.rand(7, 2)), (torch.rand(5, 3), torch.rand(7, 4)), (torch.rand(2, 5, 3), torch.rand(3, 5, 3)),
                 (torch.rand(15), torch.rand(15))):
        with pytest.raises(ValueError):
            geometry.chamfer_distance(x, y)
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, torch.rand(17, 24), K, c2w)
    with pytest.raises(ValueError):
        geometry.geometry_metrics(torch.rand(17, 23, 3), torch.rand(17, 23, 3), K, c2w)
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, d, torch.eye(2), c2w)
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, d, K, torch.eye(3))
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, d, K, c2w, {"sky_masks": torch.ones(23, 17)})
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, d, K, c2w, {"road_masks": torch.ones(17, 23)})
    with pytest.raises(ValueError):
        geometry.geometry_metrics(d, d, K, c2w, egocar=torch.ones(17, 24))
    import bilateral_driving_amd
    assert bilateral_driving_amd.geometry is geometry
    mod = types.ModuleType("chamfer_distance")
    mod.chamfer_distance = mod.depth_map_to_point_cloud = mod.vis_cd = None
    geometry.install(mod)
    assert mod.chamfer_distance is geometry.chamfer_distance and mod.depth_map_to_point_cloud is geometry.depth_map_to_point_cloud
    assert mod.vis_cd is None
