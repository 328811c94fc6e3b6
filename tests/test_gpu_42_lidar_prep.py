"""Lidar scene preparation on the MI355X (csrc/lidar.hip through bilateral_driving_amd/lidar.py) against the reference's recorded
results (tests/golden/lidar_prep.npz) and the float64 restatement (tests/lidar_ref64.py, pinned to the reference by
tests/test_lidar_cpu.py, which also derives every bound used here).

Goldens: every point is decided, so winner maps, pix, visible, inside and the (instance, frame, row) lists are EQUAL, colours bit-equal,
depths and box coordinates within the derived bound, the downsampler within 4 ulp.  Random cases (lidar_ref64.RANDOM_SEEDS, 20 of them
at the goldens' sizes) leave out the undecided points and the pixels they can reach, at most 1 % of the points and of the occupied
pixels, asserted per case; a few random cases each for the visibility, both box forms and the downsampler under the same cap.

The product's own regrouping (lidar.group_by_timestep, and the permutation's way through project_lidar_pts_on_images and
get_init_objects) is tested on clouds whose rows are not grouped by timestep: against the reference's winners in the cloud's own row
order, and bit for bit against the same cloud grouped beforehand."""
import types

import numpy as np
import pytest
import torch

from tests import lidar_ref64 as R

pytestmark = pytest.mark.gpu

NAMES = ("shared", "sparse")
SAMPLE_MAX, SAMPLE_SEED = 350, 11      # scripts/gen_golden_lidar.py


@pytest.fixture(scope="module")
def LD():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import lidar
    return lidar


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


def gpu_launch(LD, keep=None):
    """lidar_ref64.run_projection's launch through ``project_points``; ``keep``: a list that receives every launch's device outputs."""
    def launch(x, mats, ranges, W, H, images, visible, colors):
        vis, col = dev(visible), dev(colors)
        depth, winner, pix, vis2, col2 = LD.project_points(dev(x), dev(mats), dev(ranges), W, H, dev(images), vis, col)
        assert vis2 is vis and col2 is col and winner.dtype == torch.int32 and pix.dtype == torch.int32 and depth.dtype == torch.float32
        if keep is not None:
            keep.append((depth, winner, pix, vis.clone(), col.clone()))
        visible[:] = vis.cpu().numpy()
        colors[:] = col.cpu().numpy()
        return depth.cpu().numpy(), winner.cpu().numpy().astype(np.int64), pix.cpu().numpy().astype(np.int64)
    return launch


@pytest.mark.parametrize("name", NAMES)
def test_projection_equals_the_reference(LD, name):
    case = R.golden_projection_case(name)
    stats = R.compare_projection_golden(name, R.run_projection(case, gpu_launch(LD)))
    print(f"\nlidar {name} on the device: {stats}")
    z = R.golden()
    mats = np.concatenate([m for m, _ in R.case_views(case)])
    sizes = [(cam["W"], cam["H"]) for cam in case["cams"] for _ in range(R.FRAMES)]
    vis = LD.visible_from(dev(case["points"]), dev(mats), torch.tensor(sizes))
    assert vis.dtype == torch.bool and np.array_equal(vis.cpu().numpy(), z[f"{name}_visible_all"])
    one = LD.visible_from(dev(case["points"]), dev(mats[:R.FRAMES]), sizes[0])      # one (W, H) for all views
    ref_one, dec = R.visible_any(mats[:R.FRAMES], sizes[:R.FRAMES], case["points"])
    assert dec.all() and np.array_equal(one.cpu().numpy(), ref_one)
    assert not LD.visible_from(dev(case["points"]), torch.zeros(0, 3, 4), torch.zeros(0, 2)).any()


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_projection_matches_the_restatement_on_random_cases(LD, seed):
    case = R.random_projection_case(seed)
    stats = R.compare_projection(case, R.run_projection(case, gpu_launch(LD)), label=f"seed {seed}")
    print(f"\nlidar seed {seed} on the device: {stats}")
    assert stats["undecided"] <= R.CAP * stats["points"] and stats["dirty"] <= R.CAP * stats["occupied"]


def test_projection_is_bit_identical_run_to_run_and_under_regrouping(LD):
    case = R.golden_projection_case("shared")      # its rows are not grouped by timestep
    a, b = [], []
    ga = R.run_projection(case, gpu_launch(LD, a))
    gb = R.run_projection(case, gpu_launch(LD, b))
    for x, y in zip(a, b):
        for t, u in zip(x, y):
            assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, u.view(torch.int32) if u.dtype == torch.float32 else u)
    # the same cloud with its rows already grouped: every result, mapped back, is the same bit for bit
    perm, _ = R.grouped(case)
    sorted_case = dict(case, points=case["points"][perm], timesteps=case["timesteps"][perm], colors0=case["colors0"][perm])
    assert not np.any(np.diff(sorted_case["timesteps"]) < 0)
    gs = R.run_projection(sorted_case, gpu_launch(LD))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    for ca, cs in zip(ga["cams"], gs["cams"]):
        assert np.array_equal(ca["depth"].view(np.int32), cs["depth"].view(np.int32))
        assert np.array_equal(ca["winner"], np.where(cs["winner"] >= 0, perm[np.maximum(cs["winner"], 0)], -1))
        assert np.array_equal(ca["pix"][perm], cs["pix"])
    assert np.array_equal(ga["visible"][perm], gs["visible"]) and np.array_equal(ga["colors"][perm].view(np.int32), gs["colors"].view(np.int32))
    assert np.array_equal(ga["colors"].view(np.int32), gb["colors"].view(np.int32))


def test_projection_edge_shapes_and_errors(LD):
    from bilateral_driving_amd import _lib as L
    M = dev(R.golden()["shared_cam0_lidar2img"])
    # no point at all: every map empty
    depth, winner, pix, vis, col = LD.project_points(torch.zeros(0, 3).cuda(), M, torch.zeros(3, 2, dtype=torch.int64), 40, 24)
    assert (winner == -1).all() and (depth == 0).all() and pix.numel() == 0 and vis.numel() == 0 and col is None
    # no view at all
    x = dev(R.golden()["shared_points"][:300])
    depth, winner, pix, vis, col = LD.project_points(x, torch.zeros(0, 3, 4), torch.zeros(0, 2, dtype=torch.int64), 40, 24)
    assert depth.shape == (0, 24, 40) and (pix == -1).all() and not vis.any()
    # ranges beyond the cloud are clamped; without images no colours
    depth, winner, pix, vis, col = LD.project_points(x, M[:1], torch.tensor([[-5, 10 ** 9]]), 40, 24)
    assert col is None and int(winner.max()) < 300 and vis.dtype == torch.bool and bool((pix >= 0).eq(vis).all())
    # more views than one LDS stage holds: the same matrix VIEW_CHUNK + 3 times over disjoint ranges gives one view's result in pieces
    V = LD.VIEW_CHUNK + 3
    cuts = torch.linspace(0, 300, V + 1).long()
    many = LD.project_points(x, M[:1].expand(V, 4, 4), torch.stack([cuts[:-1], cuts[1:]], 1), 40, 24)
    assert torch.equal(many[1].max(0).values, winner[0]) and torch.equal(many[3], vis)
    assert torch.equal(torch.where(many[2] >= 0, many[2] % (24 * 40), many[2]), pix)
    bad = x.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError):
        LD.project_points(bad, M[:1], torch.tensor([[0, 300]]), 40, 24)
    bad[7, 1] = float("inf")
    with pytest.raises(ValueError):
        LD.visible_from(bad, M, (40, 24))
    with pytest.raises(ValueError):
        LD.points_in_boxes(bad, torch.eye(4)[None, None], torch.ones(1, 3), torch.ones(1, 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        LD.project_points(x, M, torch.zeros(2, 2, dtype=torch.int64), 40, 24)
    with pytest.raises(ValueError):
        LD.project_points(x, M, torch.zeros(3, 2, dtype=torch.int64), 40, 24, images=torch.zeros(3, 24, 41, 3).cuda())
    with pytest.raises(L.BdsError):
        LD.project_points(x.cpu(), M, torch.zeros(3, 2, dtype=torch.int64), 40, 24)


@pytest.mark.parametrize("chunk", [3, 128])
def test_boxes_equal_the_reference(LD, chunk):
    """chunk 3: 24 active boxes go through eight LDS stages; 128: one."""
    z, case = R.golden(), R.golden_box_case()
    F = case["active"].shape[0]
    x, poses, sizes = dev(case["points"]), torch.from_numpy(case["poses"]), torch.from_numpy(case["sizes"])
    fr = R.frame_ranges(case["timesteps"], F)
    for node_type in ("RigidNodes", "DeformableNodes"):
        eligible = R.eligible_of(case, node_type)
        assert eligible.sum() > chunk or chunk == 128
        rec = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(eligible), torch.from_numpy(fr), emit=True, chunk=chunk)
        ids = torch.stack([rec["instance"], rec["frame"], rec["row"]], 1).cpu().numpy()
        xyz = rec["xyz"].cpu().numpy()
        ref = R.compare_records(case, eligible, ids, xyz, exact=True)
        recs = np.array(ref["records"], np.int64).reshape(-1, 3)
        for i in z[f"box_{node_type}_full_keys"]:
            want = z[f"box_{node_type}_full_{i}_pts"]
            assert (ids[:, 0] == i).sum() == len(want)
            assert np.all(np.abs(xyz[ids[:, 0] == i].astype(np.float64) - want) <= 2 * ref["eo"][recs[:, 0] == i])
        again = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(eligible), torch.from_numpy(fr), emit=True, chunk=chunk)
        assert all(torch.equal(rec[k].view(torch.int32) if k == "xyz" else rec[k], again[k].view(torch.int32) if k == "xyz" else again[k]) for k in rec)
    inst = [int(i) for i in z["box_filter_instances"]]
    inside = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(case["active"]), instances=inst, chunk=chunk)
    assert inside.dtype == torch.bool and np.array_equal(inside.cpu().numpy(), z["box_filter_inside"])
    # nothing active, no point
    none = torch.zeros_like(torch.from_numpy(case["active"]))
    assert not LD.points_in_boxes(x, poses, sizes, none, chunk=chunk).any()
    empty = LD.points_in_boxes(x, poses, sizes, none, emit=True, chunk=chunk)
    assert empty["row"].numel() == 0 and empty["xyz"].shape == (0, 3)
    assert LD.points_in_boxes(torch.zeros(0, 3).cuda(), poses, sizes, torch.from_numpy(case["active"]), emit=True)["row"].numel() == 0
    for bad in (0, 129, 2.0):
        with pytest.raises(ValueError):
            LD.points_in_boxes(x, poses, sizes, none, chunk=bad)


def test_downsampler_equals_the_reference(LD):
    z = R.golden()
    for k, (H, W, factor) in enumerate(R.DEPTH_CASES):
        m, gold = z[f"depth{k}_map"], z[f"depth{k}_out"]
        out = LD.downsample_sparse_depth(dev(m), factor)
        assert out.shape == gold.shape and out.dtype == torch.float32
        got = out.cpu().numpy()
        worst = ulps(got, gold).max()
        print(f"\nlidar downsampler {H}x{W} x{factor} on the device: worst difference from the reference {worst:.2f} ulp")
        assert np.array_equal(got == 0, gold == 0) and worst <= 4.0
        exact, n = R.downsample(m, factor)
        assert np.all(np.abs(got - exact) <= (n + 4) * R.U * np.abs(exact) * 1.01)
        batch = LD.downsample_sparse_depth(torch.stack([dev(m), dev(m).flip(0), dev(m)]), factor)      # a leading dimension
        assert batch.shape == (3,) + gold.shape and torch.equal(batch[0], out) and torch.equal(batch[2], out)
        assert torch.equal(batch[1], LD.downsample_sparse_depth(dev(m).flip(0).contiguous(), factor))
        assert torch.equal(LD.sparse_lidar_map_downsampler(dev(m), factor), out)
    assert torch.equal(LD.downsample_sparse_depth(dev(z["depth0_map"]), 1.0), dev(z["depth0_map"]) * (dev(z["depth0_map"]) > 1e-3))


@pytest.mark.parametrize("name", NAMES)
def test_reference_named_projection_on_a_bare_dataset(LD, name):
    z, case = R.golden(), R.golden_projection_case(name)
    d = R.bare_projection_dataset(case, "cuda")
    assert LD.project_lidar_pts_on_images(d, delete_out_of_view_points=False) is None
    # the wrapper forms lidar2img on THIS host; the fixture's points are decided under the difference between two hosts' matrices too
    ref = R.projection_reference(case, matrix_margin=True)
    assert ref["decided"].all() and ref["decided_all"].all()
    for c, cam in d.pixel_source.camera_data.items():
        maps = cam.lidar_depth_maps
        assert maps.is_cuda and maps.dtype == torch.float32 and maps.shape == z[f"{name}_cam{c}_depth"].shape
        got = maps.cpu().numpy()
        assert np.array_equal(got > 0, z[f"{name}_cam{c}_depth"] > 0)
        assert np.all(np.abs(got.astype(np.float64) - z[f"{name}_cam{c}_depth"]) <= 2 * ref["cams"][c]["edepth"])
    ls = d.lidar_source
    assert ls.visible_masks.dtype == torch.bool and np.array_equal(ls.visible_masks.cpu().numpy(), z[f"{name}_visible"])
    assert np.array_equal(ls.colors.cpu().numpy(), R.from_u8(z[f"{name}_colors"]))
    vis = LD.check_pts_visibility(d, torch.from_numpy(case["points"]))
    assert vis.is_cuda and np.array_equal(vis.cpu().numpy(), z[f"{name}_visible_all"])
    d2 = R.bare_projection_dataset(case, "cuda")
    LD.project_lidar_pts_on_images(d2)      # deletes the invisible points
    keep = z[f"{name}_visible"]
    assert d2.lidar_source.visible_masks is None and d2.lidar_source.deleted == int((~keep).sum())
    assert np.array_equal(d2.lidar_source.directions.cpu().numpy(), case["points"][keep])
    assert np.array_equal(d2.lidar_source.colors.cpu().numpy(), R.from_u8(z[f"{name}_colors"])[keep])


def test_reference_named_box_methods_on_a_bare_dataset(LD):
    z, case = R.golden(), R.golden_box_case()
    d = R.bare_box_dataset(case, "cuda")
    F = case["active"].shape[0]
    for node_type in ("RigidNodes", "DeformableNodes"):
        eligible = R.eligible_of(case, node_type)
        ref = R.boxes(case["points"], case["poses"], case["sizes"], eligible, R.frame_ranges(case["timesteps"], F))
        recs = np.array(ref["records"], np.int64).reshape(-1, 3)
        full = LD.get_init_objects(d, node_type, instance_max_pts=10 ** 9, only_moving=False)
        assert list(full.keys()) == list(z[f"box_{node_type}_full_keys"])
        for i, v in full.items():
            want, sel = z[f"box_{node_type}_full_{i}_pts"], recs[:, 0] == i
            assert v["node_type"] == node_type and v["num_pts"] == len(want) == v["pts"].shape[0] and v["pts"].is_cuda
            assert np.all(np.abs(v["pts"].cpu().numpy().astype(np.float64) - want) <= 2 * ref["eo"][sel])
            assert np.array_equal(v["colors"].cpu().numpy(), case["colors"][recs[sel, 2]])
            assert torch.equal(v["poses"].cpu(), torch.from_numpy(case["poses"][:, i])) and torch.equal(v["size"].cpu(), torch.from_numpy(case["sizes"][i]))
            assert torch.equal(v["frame_info"].cpu(), torch.from_numpy(case["active"][:, i]))
        torch.manual_seed(SAMPLE_SEED)
        sampled = LD.get_init_objects(d, node_type, instance_max_pts=SAMPLE_MAX)      # only_moving, threshold 0.5
        assert list(sampled.keys()) == list(z[f"box_{node_type}_sampled_keys"])
        torch.manual_seed(SAMPLE_SEED)      # the reference's draws replayed: one randperm per instance above the cap, in its dict order
        picks = {i: (torch.randperm(v["num_pts"])[:SAMPLE_MAX].numpy() if v["num_pts"] > SAMPLE_MAX else np.arange(v["num_pts"]))
                 for i, v in full.items()}
        for i, v in sampled.items():
            want = z[f"box_{node_type}_sampled_{i}_pts"]
            assert v["num_pts"] == len(want) == min(SAMPLE_MAX, full[i]["num_pts"])
            assert np.array_equal(v["colors"].cpu().numpy(), R.from_u8(z[f"box_{node_type}_sampled_{i}_colors"]))
            assert torch.equal(v["pts"], full[i]["pts"][torch.from_numpy(picks[i]).cuda()])      # the same rows as the reference drew
            bound = ref["eo"][recs[:, 0] == i][picks[i]]
            assert np.all(np.abs(v["pts"].cpu().numpy().astype(np.float64) - want) <= 2 * bound)
    skipped = LD.get_init_objects(d, "DeformableNodes", instance_max_pts=10 ** 9, only_moving=False, exclude_smpl=True)
    assert list(skipped.keys()) == [4, 5]      # instance 6's true id is in smpl_human_all
    d.type = "KITTI"      # threshold 5.0: nothing here moves that far
    assert list(LD.get_init_objects(d, "RigidNodes", instance_max_pts=SAMPLE_MAX).keys()) == [
        i for i in (0, 1, 2) if np.linalg.norm(np.diff(case["poses"][case["active"][:, i], i, :3, 3], axis=0), axis=1).sum() > 5.0]
    d.type = "Waymo"
    inst = {int(i): None for i in z["box_filter_instances"]}
    N = len(case["points"])
    seed = dev(case["points"])
    kept = LD.filter_pts_in_boxes(d, seed, inst, dev(case["colors"]), torch.arange(N).cuda())
    keep = ~z["box_filter_inside"]
    assert np.array_equal(kept["time"].cpu().numpy(), np.nonzero(keep)[0]) and np.array_equal(kept["pts"].cpu().numpy(), case["points"][keep])
    assert np.array_equal(kept["colors"].cpu().numpy(), case["colors"][keep])
    only = LD.filter_pts_in_boxes(d, seed, inst)
    assert only["colors"] is None and only["time"] is None and torch.equal(only["pts"], kept["pts"])


def test_install_and_uninstall_on_reference_shaped_objects(LD):
    class DrivingDataset:
        def check_pts_visibility(self, pts_xyz):
            return "former"
    mod = types.ModuleType("datasets.base.pixel_source")
    mod.sparse_lidar_map_downsampler = former = lambda m, f: "former"
    LD.install(DrivingDataset, mod)
    case = R.golden_projection_case("sparse")
    d = R.bare_projection_dataset(case, "cuda")
    ds = DrivingDataset()
    ds.__dict__.update(d.__dict__)
    vis = ds.check_pts_visibility(torch.from_numpy(case["points"]))      # bound like the reference's method
    assert np.array_equal(vis.cpu().numpy(), R.golden()["sparse_visible_all"])
    ds.project_lidar_pts_on_images(delete_out_of_view_points=False)
    assert np.array_equal(ds.lidar_source.visible_masks.cpu().numpy(), R.golden()["sparse_visible"])
    m = dev(R.golden()["depth2_map"])
    assert torch.equal(mod.sparse_lidar_map_downsampler(m, 0.5), LD.downsample_sparse_depth(m, 0.5))
    LD.uninstall(DrivingDataset, mod)
    assert ds.check_pts_visibility(None) == "former" and mod.sparse_lidar_map_downsampler is former
    assert not hasattr(DrivingDataset, "project_lidar_pts_on_images")


# ---- the product's own regrouping -------------------------------------------------------------------------------------------------------
def test_group_by_timestep_then_project_points_gives_the_references_winners(LD):
    """``lidar.group_by_timestep`` on the shuffled golden cloud, its permutation and offsets fed to ``project_points``, the winner map and
    pix mapped back through that permutation: equal to the reference's winners in the cloud's own row order."""
    name = "shared"
    z, case = R.golden(), R.golden_projection_case(name)
    assert np.any(np.diff(case["timesteps"]) < 0)
    T = len(case["sweep_times"])
    perm, offsets = LD.group_by_timestep(dev(case["timesteps"]), T)
    want_perm, want_off = R.grouped(case)
    assert perm.is_cuda and np.array_equal(perm.cpu().numpy(), want_perm) and np.array_equal(offsets.cpu().numpy(), want_off)
    ident, off2 = LD.group_by_timestep(dev(case["timesteps"][want_perm]), T)      # a grouped cloud: the identity
    assert torch.equal(ident, torch.arange(len(want_perm)).cuda()) and torch.equal(off2, offsets)
    x = dev(case["points"])[perm]
    idx = torch.from_numpy(R.closest_sweeps(case)).cuda()
    ranges = torch.stack([offsets[idx], offsets[idx + 1]], 1)
    ref = R.projection_reference(case)
    for c, cam in enumerate(case["cams"]):
        depth, winner, pix, vis, col = LD.project_points(x, dev(z[f"{name}_cam{c}_lidar2img"]), ranges, cam["W"], cam["H"], dev(cam["images"]))
        back = torch.where(winner >= 0, perm[winner.long().clamp(min=0)], torch.full_like(winner, -1).long())
        assert np.array_equal(back.cpu().numpy(), z[f"{name}_cam{c}_winner"])
        pix_back = torch.empty_like(pix)
        pix_back[perm] = pix
        assert np.array_equal(pix_back.cpu().numpy(), ref["cams"][c]["pix"])


def test_reference_named_projection_is_bit_identical_under_regrouping(LD):
    """project_lidar_pts_on_images on the shuffled cloud and on the same cloud grouped beforehand: the depth maps, and visible_masks and
    colours once mapped back, are the same bit for bit; so are the clouds left after the invisible points are deleted."""
    case = R.golden_projection_case("shared")
    perm, _ = R.grouped(case)
    assert not np.array_equal(perm, np.arange(len(perm)))
    sorted_case = dict(case, points=case["points"][perm], timesteps=case["timesteps"][perm], colors0=case["colors0"][perm])
    for delete in (False, True):
        a, b = R.bare_projection_dataset(case, "cuda"), R.bare_projection_dataset(sorted_case, "cuda")
        LD.project_lidar_pts_on_images(a, delete_out_of_view_points=delete)
        LD.project_lidar_pts_on_images(b, delete_out_of_view_points=delete)
        for ca, cb in zip(a.pixel_source.camera_data.values(), b.pixel_source.camera_data.values()):
            assert torch.equal(ca.lidar_depth_maps.view(torch.int32), cb.lidar_depth_maps.view(torch.int32))
            assert bool((ca.lidar_depth_maps > 0).any())
        if not delete:
            p = torch.from_numpy(perm).cuda()
            assert torch.equal(a.lidar_source.visible_masks[p], b.lidar_source.visible_masks)
            assert torch.equal(a.lidar_source.colors[p].view(torch.int32), b.lidar_source.colors.view(torch.int32))
        else:      # the survivors: the same points with the same colours (a's in the shuffled order, b's grouped)
            keep = R.golden()["shared_visible"]
            order = np.argsort(case["timesteps"][keep], kind="stable")
            o = torch.from_numpy(order).cuda()
            assert torch.equal(a.lidar_source.directions[o], b.lidar_source.directions)
            assert torch.equal(a.lidar_source.colors[o].view(torch.int32), b.lidar_source.colors.view(torch.int32))


def test_get_init_objects_is_bit_identical_under_regrouping(LD):
    """get_init_objects and filter_pts_in_boxes on the box cloud with its sweeps interleaved (every sweep's rows still in their order)
    against the grouped cloud: keys, points, colours and counts equal bit for bit, with and without sampling."""
    case = R.golden_box_case()
    mixed, slot = R.interleave_sweeps(case, 5)
    assert np.any(np.diff(mixed["timesteps"]) < 0) and np.array_equal(mixed["points"][slot], case["points"])
    a, b = R.bare_box_dataset(mixed, "cuda"), R.bare_box_dataset(case, "cuda")
    for node_type in ("RigidNodes", "DeformableNodes"):
        for kw in (dict(instance_max_pts=10 ** 9, only_moving=False), dict(instance_max_pts=SAMPLE_MAX)):
            torch.manual_seed(SAMPLE_SEED)
            ra = LD.get_init_objects(a, node_type, **kw)
            torch.manual_seed(SAMPLE_SEED)
            rb = LD.get_init_objects(b, node_type, **kw)
            assert list(ra.keys()) == list(rb.keys()) and len(rb) > 0
            for i in rb:
                assert ra[i]["num_pts"] == rb[i]["num_pts"]
                assert torch.equal(ra[i]["pts"].view(torch.int32), rb[i]["pts"].view(torch.int32))
                assert torch.equal(ra[i]["colors"].view(torch.int32), rb[i]["colors"].view(torch.int32))
    inst = {int(i): None for i in R.golden()["box_filter_instances"]}
    ka = LD.filter_pts_in_boxes(a, dev(mixed["points"]), inst, None, dev(slot.argsort()))      # time = the row's place in the grouped cloud
    kb = LD.filter_pts_in_boxes(b, dev(case["points"]), inst, None, torch.arange(len(slot)).cuda())
    assert torch.equal(ka["time"].sort().values, kb["time"]) and ka["pts"].shape == kb["pts"].shape


# ---- random cases for the other ops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.RANDOM_SEEDS[:3])
def test_visibility_matches_the_restatement_on_random_cases(LD, seed):
    case = R.random_projection_case(seed)
    mats = np.concatenate([m for m, _ in R.case_views(case)])
    sizes = [(cam["W"], cam["H"]) for cam in case["cams"] for _ in range(R.FRAMES)]
    want, dec = R.visible_any(mats, sizes, case["points"])
    assert (~dec).sum() <= R.CAP * len(dec)
    got = LD.visible_from(dev(case["points"]), dev(mats), torch.tensor(sizes)).cpu().numpy()
    assert np.array_equal(got[dec], want[dec]) and want.any() and not want.all()


@pytest.mark.parametrize("seed", (2000, 2001, 2002))
def test_boxes_match_the_restatement_on_random_cases(LD, seed):
    case = R.box_case(seed)
    F = case["active"].shape[0]
    x, poses, sizes = dev(case["points"]), torch.from_numpy(case["poses"]), torch.from_numpy(case["sizes"])
    rec = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(case["active"]), torch.from_numpy(R.frame_ranges(case["timesteps"], F)),
                             emit=True, chunk=5 + seed % 3)
    ids = torch.stack([rec["instance"], rec["frame"], rec["row"]], 1).cpu().numpy()
    ref = R.compare_records(case, case["active"], ids, rec["xyz"].cpu().numpy())      # at most CAP of the points undecided (asserted)
    assert len(ref["records"]) > 500
    full = R.boxes(case["points"], case["poses"], case["sizes"], case["active"])
    assert (~full["decided"]).sum() <= R.CAP * len(full["decided"])
    inside = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(case["active"]), chunk=5 + seed % 3).cpu().numpy()
    assert np.array_equal(inside[full["decided"]], full["inside"][full["decided"]])


@pytest.mark.parametrize("seed,H,W,factor", [(3000, 25, 41, 0.5), (3001, 17, 23, 0.25), (3002, 24, 40, 1.5), (3003, 31, 29, 0.4)])
def test_downsampler_matches_the_restatement_on_random_cases(LD, seed, H, W, factor):
    m = R.depth_case(seed, H, W)
    got = LD.downsample_sparse_depth(dev(m), factor).cpu().numpy()
    f32, _ = R.downsample(m, factor, np.float32)
    exact, n = R.downsample(m, factor)
    assert got.shape == f32.shape == R.output_size(H, W, factor)
    assert np.array_equal(got == 0, f32 == 0) and ulps(got, f32).max() <= 4.0
    assert np.all(np.abs(got - exact) <= (n + 4) * R.U * np.abs(exact) * 1.01)
