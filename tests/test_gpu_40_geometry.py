"""Evaluation geometry metrics on the MI355X (csrc/geometry.hip through bilateral_driving_amd/geometry.py) against the float64
restatement of the reference's geometry scoring (tests/geometry_ref64.py: brute-force nearest neighbours from coordinate differences).

The cases (geometry_ref64.CASES) set the number of valid points n through the lidar hit rate of small images: 0, 1, 2, 19, 20, 21 (k = 0
for some trims and the smallest non-empty ones), one below, at and one above the pair loop's query block and target tile (read from the
module), several of each (1700), an empty class, classes of one point, human inside dynamic, an absent mask key and no masks at all,
egocar present and absent, depths on and next to the validity limits, and a camera 10^3 m from the origin.  The bound is not fixed: per
case and per value the float32 restatement's own distance from float64 is measured, and the kernels are held to twice that plus
geometry_ref64.FLOOR (measured with the host shim, tests/test_geometry_cpu.py) -- for the two distance arrays, the worst element's."""
import math
import types

import numpy as np
import pytest
import torch

from tests import geometry_ref64 as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import geometry
    return geometry


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def infos(inp, as_type=None):
    out = {"lidar_depth_map": dev(inp["gt"]), **{k: dev(v) if as_type is None else dev(v).to(as_type) for k, v in inp["masks"].items()}}
    if inp["egocar"] is not None:
        out["egocar_masks"] = dev(inp["egocar"]).float()
    return out


def cams(inp):
    K4 = np.eye(4, dtype=np.float32)
    K4[:3, :3] = inp["K"]
    return {"intrinsics": dev(K4), "camera_to_world": dev(inp["c2w"])}      # (the dataset's intrinsics are 4x4: the upper-left 3x3 counts)


def run(G, inp, **kw):
    masks = {k: dev(v) for k, v in inp["masks"].items()}
    ego = None if inp["egocar"] is None else dev(inp["egocar"])
    return G.geometry_metrics(dev(inp["pred"]), dev(inp["gt"]), dev(inp["K"]), dev(inp["c2w"]), masks, ego, **kw)


def bits(d):
    return {k: (v.view(torch.int64) if v.dtype == torch.float64 else v.view(torch.int32)).cpu() for k, v in d.items()}


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def same_floats(a, b):
    return a.keys() == b.keys() and all(np.float64(a[k]).view(np.int64) == np.float64(b[k]).view(np.int64) for k in a)


def test_the_cases_cover_the_sizes_at_which_the_pair_loop_changes_path(G):
    assert G.QUERY_BLOCK == G.TARGET_TILE == 512
    ns = {c[2] for c in R.CASES.values()}
    for edge in (G.QUERY_BLOCK, G.TARGET_TILE):
        assert {edge - 1, edge, edge + 1} <= ns and max(ns) > 3 * edge
    assert {0, 1, 2, 19, 20, 21} <= ns


# ---- every scalar and both distance arrays ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_scalars_and_distances_match_float64_within_the_float32_restatements_error(G, name):
    inp, r64, r32 = R.case(name)
    got = run(G, inp, return_distances=True)
    n = r64["valid"]
    assert got["chamfer"].dtype == torch.float64 and got["chamfer"].is_cuda and got["chamfer"].dim() == 0
    assert float(got["valid"]) == n and all(float(got[f"{c}_valid"]) == r64[f"{c}_valid"] for c in R.CLASSES)
    vals = {k: float(got[k]) for k in R.SCALARS}
    vals["dist_pred"], vals["dist_gt"] = (got[k][:n].cpu().numpy() for k in ("dist_pred", "dist_gt"))
    for k in R.SCALARS + ("dist_pred", "dist_gt"):
        bound, e32 = R.bound(r64, r32, k)
        err = R.error(vals[k], r64, k)
        print(f"geometry {name} {k}: float32 restatement {e32:.3e}, bound {bound:.3e}, kernel {err:.3e}")
        assert err <= bound, (name, k, vals[k], r64[k], bound)
    # the frame form, the accumulator and the device form agree bit for bit
    want = {k: float(got[k]) for k in R.FRAME_KEYS}
    want.update({f"chamfer_{c}": float(got[f"chamfer_{c}"]) for c in R.CLASSES if not math.isnan(float(got[f"chamfer_{c}"]))})
    assert want.keys() == R.reference_frame(r64).keys()
    fg = G.frame_geometry(dev(inp["pred"])[None, ..., None], infos(inp), cams(inp))      # (the render's depth is [1,H,W,1])
    acc = G.GeometryAccumulator(2)
    acc.add(dev(inp["pred"]), infos(inp), cams(inp))
    assert len(acc) == 1 and same_floats(fg, want) and same_floats(acc.per_frame()[0], want)


def test_the_far_camera_widens_the_bound_and_the_kernel_stays_inside(G):
    _, n64, n32 = R.case("no_masks")              # the same depths from a camera 6 m from the origin
    inp, f64, f32 = R.case("far")
    near, far = R.bound(n64, n32, "dist_pred")[0], R.bound(f64, f32, "dist_pred")[0]
    # coordinates of up to 64 m resolve 4e-6 m in float32, those of 10^3 m 6e-5 m: 16 times coarser; half of that is asked for
    assert far > 8 * near
    got = run(G, inp, return_distances=True)
    err = R.error(got["dist_pred"][:300].cpu().numpy(), f64, "dist_pred")
    assert R.FLOOR < err <= far                  # the error is real, yet far below the ~0.1 m^2 that |x|^2 + |y|^2 - 2 x.y loses there


# ---- masks -----------------------------------------------------------------------------------------------------------------------------
def test_mask_element_types_give_the_same_bits(G):
    inp, _, _ = R.case("n513")
    p, g, K, c = dev(inp["pred"]), dev(inp["gt"]), dev(inp["K"]), dev(inp["c2w"])
    m, ego = {k: dev(v) for k, v in inp["masks"].items()}, dev(inp["egocar"])
    as_bool = G.geometry_metrics(p, g, K, c, m, ego)
    as_u8 = G.geometry_metrics(p, g, K, c, {k: v.to(torch.uint8) * 3 for k, v in m.items()}, ego.to(torch.uint8) * 7)      # non-zero = true
    as_f32 = G.geometry_metrics(p, g, K, c, {k: v.float() * 0.5 for k, v in m.items()}, ego.float())
    mixed = G.geometry_metrics(p, g, K, c, {k: (v.float() if i % 2 else v.double()) for i, (k, v) in enumerate(m.items())}, ego)
    assert same_bits(as_bool, as_u8) and same_bits(as_bool, as_f32) and same_bits(as_bool, mixed)
    assert float(as_bool["valid"]) == 513


def test_an_absent_mask_key_is_an_all_false_mask(G):
    inp, r64, _ = R.case("absent_vehicle")
    absent = run(G, inp)
    zeros = dict(inp, masks=dict(inp["masks"], vehicle_masks=np.zeros(inp["pred"].shape, bool)))
    assert same_bits(absent, run(G, zeros))
    assert float(absent["vehicle_valid"]) == 0 and math.isnan(float(absent["chamfer_vehicle"]))
    assert float(absent["background_valid"]) == r64["background_valid"] > 0
    none = run(G, R.case("no_masks")[0])
    assert float(none["background_valid"]) == float(none["valid"]) == 300
    assert abs(float(none["chamfer_background"]) - float(none["chamfer"])) <= 1e-12 * float(none["chamfer"])      # the same pairs


def test_validity_edges(G):
    inp, r64, _ = R.case("edges")
    _, _, ok = R.edge_frame()
    H, W = ok.shape
    K, c2w = dev(inp["K"]), dev(inp["c2w"])
    got = run(G, inp)
    assert float(got["valid"]) == ok.sum() == 9 and float(got["dynamic_valid"]) == r64["dynamic_valid"] > 0
    # which pixels: the valid ones unproject to the restatement's points, in row-major order
    pts = G.depth_map_to_point_cloud(dev(inp["gt"]), K, c2w, dev(ok))
    want = R.unproject(inp["gt"], inp["K"], inp["c2w"], ok, np.float64)
    assert pts.shape == (9, 3) and np.abs(pts.cpu().numpy() - want).max() <= 4 * np.finfo(np.float32).eps * (np.abs(want).max() + 160)


# ---- the reference's two functions ------------------------------------------------------------------------------------------------------
def test_depth_map_to_point_cloud_is_row_major_and_masked(G):
    H, W = 40, 56
    K, c2w = R.camera(H, W)
    depth = np.random.default_rng(5).uniform(0.5, 79.0, (H, W)).astype(np.float32)
    mask = np.random.default_rng(6).uniform(0, 1, (H, W)) < 0.4
    for m in (None, mask):
        want = R.unproject(depth, K, c2w, np.ones((H, W), bool) if m is None else m, np.float64)
        tol = 4 * np.finfo(np.float32).eps * (np.abs(want).max() + 160)      # as the host test's: an ulp of each term
        for cast in (lambda t: t, lambda t: t.float(), lambda t: t.to(torch.uint8)):
            got = G.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), None if m is None else cast(dev(m)))
            assert got.dtype == torch.float32 and got.shape == want.shape and np.abs(got.cpu().numpy() - want).max() <= tol
    assert G.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), dev(np.zeros((H, W), bool))).shape == (0, 3)
    # a 4x4 intrinsics matrix: its upper-left 3x3
    K4 = np.eye(4, dtype=np.float32)
    K4[:3, :3] = K
    assert torch.equal(G.depth_map_to_point_cloud(dev(depth), dev(K4), dev(c2w), dev(mask)), got)


@pytest.mark.parametrize("norm", [2, 1])
def test_chamfer_distance_between_clouds_of_different_sizes(G, norm):
    g = np.random.default_rng(norm)
    x, y = g.uniform(-20, 20, (700, 3)).astype(np.float32), g.uniform(-20, 20, (1300, 3)).astype(np.float32)
    cx, cy = G.chamfer_distance(dev(x), dev(y), norm=norm)
    assert cx.shape == (700,) and cy.shape == (1300,) and cx.dtype == torch.float32 and cx.is_cuda
    for got, a, b in ((cx, x, y), (cy, y, x)):
        r64, r32 = R.nearest(a.astype(np.float64), b.astype(np.float64), norm), R.nearest(a, b, norm)
        bound = 2 * np.abs(r32 - r64).max() + R.FLOOR
        assert np.abs(got.cpu().numpy() - r64).max() <= bound
    bx, by = G.chamfer_distance(dev(np.stack([x[:600], x[100:]])), dev(np.stack([y, y[::-1]])), norm=norm)      # batched [N,P,3]
    assert bx.shape == (2, 600) and by.shape == (2, 1300) and torch.equal(bx[0], G.chamfer_distance(dev(x[:600]), dev(y), norm)[0])
    assert torch.equal(by[1].flip(0), G.chamfer_distance(dev(x[100:]), dev(y), norm)[1])
    ex, ey = G.chamfer_distance(dev(x[:5]), dev(y[:0]), norm=norm)
    assert ey.shape == (0,) and bool(torch.isinf(ex).all())
    with pytest.raises(ValueError):
        G.chamfer_distance(dev(x), dev(y), norm=3)
    with pytest.raises(ValueError):
        G.chamfer_distance(dev(x[:, :2]), dev(y[:, :2]))


def test_install_lets_the_references_own_flow_reach_the_same_distances(G):
    mod = types.ModuleType("chamfer_distance")
    mod.chamfer_distance = mod.depth_map_to_point_cloud = None
    G.install(mod)
    assert mod.chamfer_distance is G.chamfer_distance and mod.depth_map_to_point_cloud is G.depth_map_to_point_cloud
    inp, r64, _ = R.case("n513")
    fused = run(G, inp, return_distances=True)
    # video_utils.py:366-384, through the module's two names
    pred, gt = dev(inp["pred"]), dev(inp["gt"])
    hit = (gt > 0).float() * (1.0 - dev(inp["egocar"]).float())
    pred, gt = pred * hit, gt * hit
    valid = (gt > 0.01) & (gt < 80.0) & (pred > 0.0001) & (pred < 80.0)
    lidar = mod.depth_map_to_point_cloud(gt, dev(inp["K"]), dev(inp["c2w"]), valid)
    cloud = mod.depth_map_to_point_cloud(pred, dev(inp["K"]), dev(inp["c2w"]), valid)
    cham_pred, cham_gt = mod.chamfer_distance(cloud, lidar)
    assert cham_pred.shape == (513,) and torch.equal(cham_pred, fused["dist_pred"][:513]) and torch.equal(cham_gt, fused["dist_gt"][:513])
    assert abs(cham_pred.double().mean().item() - float(fused["cham_pred"])) <= 1e-12 * float(fused["cham_pred"])


# ---- determinism, the accumulator, errors --------------------------------------------------------------------------------------------------
def test_two_runs_of_a_frame_give_bit_equal_rows(G):
    inp, _, _ = R.case("n1700")
    a, b = run(G, inp, return_distances=True), run(G, inp, return_distances=True)
    n = int(a["valid"])
    assert n == 1700 and same_bits({k: (v[:n] if v.dim() else v) for k, v in a.items()}, {k: (v[:n] if v.dim() else v) for k, v in b.items()})
    assert all(math.isfinite(float(a[k])) for k in R.SCALARS)


def test_accumulator_means_leave_out_the_frames_whose_class_is_empty(G):
    names = ("empty_human", "one_vehicle", "n513", "absent_vehicle", "n1")
    acc = G.GeometryAccumulator(len(names))
    for i, name in enumerate(names):
        inp = R.case(name)[0]
        acc.add(dev(inp["pred"]), infos(inp, torch.float32 if i % 2 else None), cams(inp))
    assert len(acc) == len(names)
    res, frames = acc.results(), acc.per_frame()
    r64, r32 = ([R.reference_frame(R.case(name)[j]) for name in names] for j in (1, 2))
    want = R.results(r64)
    assert sorted(res) == sorted(want) == sorted(G.RESULT_KEYS)
    assert [sorted(f) for f in frames] == [sorted(f) for f in r64]
    assert "chamfer_human" not in frames[0] and "chamfer_vehicle" not in frames[3] and "chamfer_human" in frames[2]
    for key, v in want.items():
        k = key[4:] if key.startswith("avg_") else key
        if k.startswith("chamfer_9") or k in ("depth_err_rmse_99", "depth_err_rmse_97", "depth_err_rmse_95"):
            assert math.isnan(v) and math.isnan(res[key]), key              # the one-point frame's trims are NaN, and are not filtered
            continue
        per = [(a[k], b[k]) for a, b in zip(r64, r32) if k in a]
        assert len(per) == sum(k in f for f in frames) >= 1
        bound = sum(2 * abs(a - b) + R.FLOOR for a, b in per) / len(per)     # (a mean's error is at most its terms' mean error)
        assert abs(res[key] - v) <= bound, (key, res[key], v, bound)
    with pytest.raises(IndexError):
        acc.add(dev(inp["pred"]), infos(inp), cams(inp))
    assert G.GeometryAccumulator(3).results() == {k: -1 for k in G.RESULT_KEYS}
    other = G.GeometryAccumulator(2)
    other.add(dev(inp["pred"]), infos(inp), cams(inp))
    from bilateral_driving_amd import _lib as L
    with torch.cuda.stream(torch.cuda.Stream()), pytest.raises(L.BdsError):
        other.add(dev(inp["pred"]), infos(inp), cams(inp))
    torch.cuda.synchronize()


def test_errors(G):
    from bilateral_driving_amd import _lib as L
    d = torch.rand(17, 23, device="cuda") + 1
    K, c2w = torch.eye(3, device="cuda"), torch.eye(4, device="cuda")
    with pytest.raises(ValueError):
        G.geometry_metrics(d, d[:, :22], K, c2w)
    with pytest.raises(ValueError):
        G.geometry_metrics(d, d, K, c2w, {"sky_masks": torch.ones(23, 17, device="cuda")})
    with pytest.raises(ValueError):
        G.geometry_metrics(d, d, K[:2], c2w)
    with pytest.raises(L.BdsError):
        G.geometry_metrics(d.cpu(), d.cpu(), K.cpu(), c2w.cpu())
    with pytest.raises(L.BdsError):
        G.geometry_metrics(d, d, K, c2w, {"sky_masks": torch.ones(17, 23)})
    with pytest.raises(L.BdsError):
        G.chamfer_distance(torch.rand(5, 3), torch.rand(7, 3, device="cuda"))
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    row = torch.empty(G.ROW, dtype=torch.float64, device="cuda")
    args = (L.ptr(d), L.ptr(d), None, None, None, None, None, 0, L.ptr(K), L.ptr(c2w), L.ptr(row), None, None, L.ptr(ws), 256, L.stream())
    assert L.lib().bds_geometry_metrics(17, 23, *args) == L.BDS_EWORKSPACE and L.lib().bds_geometry_metrics(0, 23, *args) == L.BDS_EINVAL
