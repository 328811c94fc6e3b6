"""Pseudo-lidar generation on the MI355X (csrc/pseudo_lidar.hip through bilateral_driving_amd/pseudo_lidar.py) against the reference's
recorded results (tests/golden/pseudo_lidar.npz) and the float64 restatement (tests/pseudo_lidar_ref64.py, pinned to the reference by
tests/test_pseudo_lidar_cpu.py, which also derives every bound used here).

Golden cases: counts and the emitted winners (``source``) EQUAL, coordinates within e_dev of the restatement and within e_dev + e_ref of
the reference's float64 output, a cloud's rows -- intensities too -- bit for bit.  Random cases and edge shapes: the winners of the clean
beams equal and in beam order, every emitted coordinate within e_dev of its source pixel's, under the caps (at most 1 % of the live
pixels undecided, 2 % of the occupied beams dirty), asserted per case.  The shapes are the smallest that cross what the kernels
cross: an image whose pixel count is no multiple of 64 or 256 (runs of equal cells end at wave, workgroup and image-row ends), a
batch whose middle camera is empty, a beam map of 32 scan passes, a slice beyond H."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import pseudo_lidar_ref64 as R

pytestmark = pytest.mark.gpu

DEPTH_NAMES = tuple(R.GOLDEN_DEPTH)
EDGE = {"odd": dict(seed=31, Hi=47, Wi=83, H=8, W=16),                      # 3901 pixels: 15 workgroups and a part, rows of 83
        "chunks": dict(seed=32, Hi=96, Wi=160, H=64, W=512),                # 32768 cells: 32 scan passes, sparse
        "slice": dict(seed=33, Hi=61, Wi=83, H=16, W=32, slice=40)}         # only row 0 is kept (the ground 3 m ahead)


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import pseudo_lidar
    return pseudo_lidar


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def golden_ref(name):
    case = R.golden_depth_case(name)
    return case, R.depth_reference(case)


@functools.lru_cache(maxsize=None)
def street_ref(key):
    case = R.random_case(key) if isinstance(key, int) else R.street_case(**EDGE[key])
    return case, R.depth_reference(case, "device")


def run(P, cases, **kw):
    """One batched call over cases of one shape.  -> (points, counts, source) on the device."""
    c = cases[0]
    return P.depth_to_lidar(dev(np.stack([k["depth"] for k in cases])), dev(np.stack([k["K"] for k in cases])),
                            torch.from_numpy(np.stack([k["c2w"] for k in cases])), torch.from_numpy(np.stack([k["l2w"] for k in cases])),
                            c["H"], c["W"], c["slice"], c["downscale"], c["mode"], return_source=True, **kw)


def host(points, counts, source, c=0):
    return points[c].cpu().numpy(), int(counts[c]), source[c].cpu().numpy()


def within_caps(ref, label):
    und, dirty, live, occ = R.case_stats(ref)
    print(f"\npseudo-lidar {label}: {live} live pixels, {occ} occupied beams, {und:.4%} undecided, {dirty:.4%} dirty")
    assert und <= R.CAP_UNDECIDED and dirty <= R.CAP_DIRTY, (label, und, dirty)


# ---- the reference's recorded results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_depth_cases_equal_the_reference(P, name):
    z = R.golden()
    case, ref = golden_ref(name)
    points, counts, source = run(P, [case])
    cap = -(-case["H"] // case["slice"]) * case["W"]
    assert tuple(points.shape) == (1, cap, 3) and points.dtype == torch.float32 and counts.dtype == torch.int32 and source.dtype == torch.int32
    pts, n, src = host(points, counts, source)
    assert n == len(z[f"{name}_source"]) and np.array_equal(src[:n], z[f"{name}_source"])
    stats = R.compare(ref, pts, n, src, label=name)
    err = np.abs(pts[:n].astype(np.float64) - z[f"{name}_points"])
    assert np.all(err <= ref["e_dev"][src[:n]] + ref["e_ref"][src[:n]])
    print(f"\npseudo-lidar {name} on the device: {stats}; against the reference's float64 output at most {err.max():.2e} m")
    split, split_src = P.depth_to_lidar(dev(case["depth"]), dev(case["K"])[None], torch.from_numpy(case["c2w"])[None], torch.from_numpy(case["l2w"]),
                                        case["H"], case["W"], case["slice"], case["downscale"], return_source=True, split=True)
    assert len(split) == 1 and torch.equal(split[0], points[0, :n]) and torch.equal(split_src[0], source[0, :n])


def test_the_entry_leaves_rows_beyond_the_count_untouched_and_returns_the_winner_map(P):
    """The C entry into prefilled outputs: rows at and past counts[c] keep their value, winner [C,H,W] is the restatement's map."""
    from bilateral_driving_amd import _lib as L
    case, ref = golden_ref("front")
    H, W = case["H"], case["W"]
    Hi, Wi = case["depth"].shape
    cams = P.camera_table(torch.from_numpy(case["K"])[None], torch.from_numpy(case["c2w"])[None], torch.from_numpy(case["l2w"])).cuda()
    beams, d = dev(P.beam_table(H, W)), dev(case["depth"])
    winner = torch.full((H, W), 12345, dtype=torch.int32, device="cuda")
    points = torch.full((H * W, 3), 7.0, device="cuda")
    source = torch.full((H * W,), -5, dtype=torch.int32, device="cuda")
    counts = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    L.check(L.lib().bds_pseudo_lidar_from_depth(1, Hi, Wi, L.ptr(d), L.ptr(cams), L.ptr(beams), H, W, 1, P.VERTICAL, L.ptr(winner), L.ptr(points),
                                                L.ptr(counts), L.ptr(source), L.stream()), "bds_pseudo_lidar_from_depth")
    n = int(counts[0])
    assert n == len(ref["emitted"]) and 0 < n < H * W
    assert bool((points[n:] == 7.0).all()) and bool((source[n:] == -5).all()) and bool((points[:n] != 7.0).any())
    assert np.array_equal(winner.cpu().numpy().reshape(-1), ref["winner"])
    assert np.array_equal(source[:n].cpu().numpy(), ref["emitted"])


def test_cloud_case_equals_the_reference(P):
    z, case = R.golden(), R.golden_cloud_case()
    points, counts, source = P.cloud_to_lidar(dev(case["cloud"]), case["H"], case["W"], case["slice"], "classic", crop=R.SPARSE_CROP, return_source=True)
    n = int(counts[0])
    assert tuple(points.shape) == (case["H"] * case["W"], 4) and n == len(z["cloud_source"])
    assert np.array_equal(source[:n].cpu().numpy(), z["cloud_source"])
    assert np.array_equal(points[:n].cpu().numpy().view(np.int32), z["cloud_out"].view(np.int32))      # intensities too, bit for bit
    keep = z["cloud_vertical_keep"]
    points, counts, source = P.cloud_to_lidar(dev(case["cloud"][keep]), 16, case["W"], 1, "vertical", return_source=True)
    assert np.array_equal(np.nonzero(keep)[0][source[:int(counts[0])].cpu().numpy()], z["cloud_vertical_source"])
    with pytest.raises(ValueError):
        bad = case["cloud"][:100].copy()
        bad[7, 1] = np.nan
        P.cloud_to_lidar(dev(bad))
    points, counts = P.cloud_to_lidar(torch.zeros(0, 4, device="cuda"), 8, 16)
    assert int(counts[0]) == 0


def test_reference_named_wrappers_return_the_references_shapes_and_types(P, tmp_path):
    z = R.golden()
    gd, d2 = types.ModuleType("generate_lidar_from_depth"), types.ModuleType("depth2lidar")
    gd.depth_map_to_lidar_points = gd.pto_ang_map = gd.pto_ang_map_vertical = d2.pto_ang_map = d2.gen_sparse_points = former = lambda *a, **k: "former"
    P.install(gd)
    P.install(d2)
    try:
        case, ref = golden_ref("slice")
        Hi, Wi = case["depth"].shape
        got = gd.depth_map_to_lidar_points(dev(case["depth"]), torch.from_numpy(case["K"]), torch.from_numpy(case["c2w"]), Wi, Hi,
                                           torch.from_numpy(case["l2w"]), H=case["H"], W=case["W"], slice=case["slice"],
                                           downscale_when_loading=case["downscale"])
        gold, src = z["slice_points"], z["slice_source"]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == gold.shape
        assert np.all(np.abs(got - gold) <= ref["e_dev"][src] + ref["e_ref"][src])
        cloud = R.golden_cloud_case()["cloud"]
        path = str(tmp_path / "000000.bin")
        cloud.tofile(path)
        got = d2.gen_sparse_points(path, types.SimpleNamespace(H=R.GOLDEN_CLOUD["H"], W=R.GOLDEN_CLOUD["W"], slice=R.GOLDEN_CLOUD["slice"]))
        assert got.dtype == np.float64 and np.array_equal(got, z["cloud_out"].astype(np.float64))
        keep = z["cloud_vertical_keep"]
        got = gd.pto_ang_map_vertical(cloud[keep].astype(np.float64), H=16, W=R.GOLDEN_CLOUD["W"], slice=1)
        assert got.dtype == np.float64 and np.array_equal(got, cloud[z["cloud_vertical_source"]].astype(np.float64))
        plain = gd.pto_ang_map(cloud, H=64, W=32)
        again = d2.pto_ang_map(dev(cloud), 64, 32, 1)
        assert plain.dtype == np.float64 and plain.ndim == 2 and plain.shape[1] == 4 and np.array_equal(plain, again) and len(plain) >= len(z["cloud_out"])
    finally:
        P.uninstall()
    assert gd.pto_ang_map is former and d2.gen_sparse_points is former


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_random_cases_match_the_restatement(P, seed):
    case, ref = street_ref(seed)
    within_caps(ref, f"seed {seed}")
    stats = R.compare(ref, *host(*run(P, [case])), label=f"seed {seed}")
    print(f"pseudo-lidar seed {seed} on the device: {stats}")


@pytest.mark.parametrize("name", tuple(EDGE))
def test_edge_shapes_match_the_restatement(P, name):
    case, ref = street_ref(name)
    within_caps(ref, name)
    points, counts, source = run(P, [case])
    pts, n, src = host(points, counts, source)
    stats = R.compare(ref, pts, n, src, label=name)
    print(f"pseudo-lidar {name} on the device: {stats}")
    assert n > 0 and stats["checked"] > 0.9 * n
    dec = ref["decided"][src[:n]]
    assert np.all(np.diff(ref["cell"][src[:n]][dec]) > 0)      # emission order is beam order
    if name == "chunks":
        assert n < 0.5 * case["H"] * case["W"] and len(np.unique(ref["cell"][src[:n]] // 1024)) > 8      # sparse, over many scan passes
    if name == "slice":
        assert tuple(points.shape) == (1, case["W"], 3) and np.all(ref["cell"][src[:n]][dec] < case["W"])


def test_a_batch_with_an_empty_middle_camera_and_an_all_zero_map(P):
    """C = 3 with different matrices: the middle camera has no valid pixel (zeros, depths beyond max_depth, a NaN) -- its count is 0 and
    its neighbours are what they are alone; the batched call equals the C single-camera calls bit for bit; two runs are bit-identical."""
    a, ra = street_ref(R.RANDOM_SEEDS[0])
    c, rc = street_ref(R.RANDOM_SEEDS[1])
    b = dict(street_ref(R.RANDOM_SEEDS[2])[0])
    d = np.zeros_like(b["depth"])
    d[::3, ::5], d[5, 7], d[9, 9] = 95.0, np.nan, -2.0
    b["depth"] = d
    assert not np.array_equal(a["c2w"], c["c2w"]) and not np.array_equal(a["l2w"], c["l2w"])
    points, counts, source = run(P, [a, b, c])
    assert counts.cpu().tolist()[1] == 0 and int(counts[0]) > 0 and int(counts[2]) > 0
    R.compare(ra, *host(points, counts, source, 0), label="batch camera 0")
    R.compare(rc, *host(points, counts, source, 2), label="batch camera 2")
    again = run(P, [a, b, c])
    for k, case in enumerate((a, b, c)):
        n = int(counts[k])
        single = run(P, [case])
        assert int(single[1][0]) == n == int(again[1][k])
        for whole, other, one in zip((points, source), (again[0], again[2]), (single[0], single[2])):
            assert torch.equal(whole[k, :n].view(torch.int32), one[0, :n].view(torch.int32))
            assert torch.equal(whole[k, :n].view(torch.int32), other[k, :n].view(torch.int32))
    zeros = dict(a, depth=np.zeros_like(a["depth"]))
    points, counts, source = run(P, [zeros])
    assert counts.cpu().tolist() == [0]
    # one lidar_to_world for all cameras; no source asked for
    pts2, cnt2 = P.depth_to_lidar(dev(np.stack([a["depth"], a["depth"]])), dev(np.stack([a["K"], a["K"]])),
                                  torch.from_numpy(np.stack([a["c2w"], a["c2w"]])), torch.from_numpy(a["l2w"]), a["H"], a["W"])
    one = run(P, [a])
    n = int(one[1][0])
    assert cnt2.cpu().tolist() == [n, n] and torch.equal(pts2[0, :n], one[0][0, :n]) and torch.equal(pts2[1, :n], one[0][0, :n])
