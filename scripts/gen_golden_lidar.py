#!/usr/bin/env python3
"""Golden vectors for the lidar scene preparation (bilateral_driving_amd/lidar.py, csrc/lidar.hip), produced by the REFERENCE's own
DrivingDataset.project_lidar_pts_on_images / get_init_objects / filter_pts_in_boxes / check_pts_visibility
(datasets/driving_dataset.py:280-416, 496-603, 644-727), its lidar source's get_lidar_rays / find_closest_timestep /
delete_invisible_pts (datasets/base/lidar_source.py:208-260) and sparse_lidar_map_downsampler (datasets/base/pixel_source.py:77-92),
called on the CPU on bare objects that hold only the attributes they read.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_lidar.py        (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

The imports are stubbed the way scripts/gen_golden_node_pose.py does it; whatever else the reference's dataset modules import and the
environment lacks (OpenCV, for one) becomes an empty module.

The cases come from tests/lidar_ref64.py.  Every point that the restatement there cannot DECIDE (one that float32 rounding could move
across a pixel edge, an image border, z = 0 or a box face -- for the projection also under the difference between two hosts' float32
pad(K) @ inverse(c2w), lidar_ref64.case_dmats) is dropped before the reference runs, so the recorded results hold exactly
for any float32 evaluation.  The script checks the restatement against the reference as it records: the winner of every pixel -- found
as the one candidate whose depth the map holds -- is the HIGHEST row among the points that land there (the last write of the serial
index_put_), visibility, colours, box membership and record counts are equal, depths and box coordinates within the bound.

tests/golden/lidar_prep.npz: per projection case ("shared": two frames on one sweep, rows not grouped by timestep; "sparse": an empty
sweep and one with no valid point) the inputs, the reference's lidar2img matrices, depth maps, visible mask, colours and
check_pts_visibility mask, and the winner maps; the box case's inputs, the kept rows of filter_pts_in_boxes, get_init_objects' points
without sampling and with instance_max_pts = SAMPLE_MAX under torch.manual_seed(SAMPLE_SEED); the downsampler's maps and results.  Colours lie on the
8-bit grid k / 255 and are kept as bytes.  The file stays below tests/golden/node_pose_train.npz in size."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "lidar_prep.npz")
SAMPLE_MAX, SAMPLE_SEED = 350, 11
PROJECTION = {"shared": dict(seed=101, variant="shared", shuffle=True), "sparse": dict(seed=202, variant="sparse", shuffle=False)}
BOX_SEED, DEPTH_SEED = 303, 404


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def import_reference_datasets():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    for _ in range(64):
        try:
            dd = importlib.import_module("datasets.driving_dataset")
            px = importlib.import_module("datasets.base.pixel_source")
            ls = importlib.import_module("datasets.base.lidar_source")
            return dd, px, ls
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Anything(e.name)
        except ImportError as e:      # "cannot import name X from <stub>"
            if e.name is None or e.name not in sys.modules:
                raise
            sys.modules[e.name] = _Anything(e.name)
    raise RuntimeError("could not import the reference's dataset modules")


def ref_lidar(LS, points, timesteps, sweep_times, colors):
    """A bare lidar source that runs the reference's own methods."""
    class Lidar:
        get_lidar_rays = LS.get_lidar_rays
        find_closest_timestep = LS.find_closest_timestep
        delete_invisible_pts = LS.delete_invisible_pts
        timesteps = property(lambda self: self._timesteps)
        normalized_time = property(lambda self: self._normalized_time)
        unique_normalized_timestamps = property(lambda self: self._unique_normalized_timestamps)
        num_points = property(lambda self: self.origins.shape[0])
    s = Lidar()
    n = len(points)
    s.origins, s.directions, s.ranges = torch.zeros(n, 3), torch.from_numpy(points), torch.ones(n, 1)
    s.flows = torch.zeros(n, 3)
    s._timesteps = torch.from_numpy(timesteps)
    s._unique_normalized_timestamps = torch.from_numpy(sweep_times)
    s._normalized_time = s._unique_normalized_timestamps[s._timesteps.clamp(max=len(sweep_times) - 1)]
    s.colors = torch.from_numpy(colors).clone()
    s.visible_masks = torch.zeros(n, dtype=torch.bool)
    return s


def ref_projection_dataset(R, LS, case):
    d = R.bare_projection_dataset(case, "cpu")
    d.lidar_source = ref_lidar(LS, case["points"], case["timesteps"], case["sweep_times"], case["colors0"])
    return d


def ref_box_dataset(R, LS, case):
    d = R.bare_box_dataset(case, "cpu")
    d.lidar_source = ref_lidar(LS, case["points"], case["timesteps"], np.linspace(0, 1, R.BOX_F).astype(np.float32), case["colors"])
    return d


def record_projection(R, DD, LS, name, spec, out):
    case = R.projection_case(**spec)
    ref = R.projection_reference(case, matrix_margin=True)      # (decided also for matrices formed on another host)
    decided = ref["decided"] & ref["decided_all"]
    print(f"{name}: {len(decided)} points, {int((~decided).sum())} undecided dropped")
    case = R.keep_decided(case, decided)
    ref = R.projection_reference(case, matrix_margin=True)
    assert ref["decided"].all() and ref["decided_all"].all()
    ref = R.projection_reference(case)
    if spec["shuffle"]:
        assert np.any(np.diff(case["timesteps"]) < 0)
    d = ref_projection_dataset(R, LS, case)
    DD.project_lidar_pts_on_images(d, delete_out_of_view_points=False)
    vis = d.lidar_source.visible_masks.numpy()
    col = d.lidar_source.colors.numpy()
    assert np.array_equal(vis, ref["visible"]) and np.array_equal(col, R.expected_colors(case, ref))
    vis_all = DD.check_pts_visibility(d, torch.from_numpy(case["points"])).numpy()
    assert np.array_equal(vis_all, ref["visible_all"])
    perm, _ = R.grouped(case)
    views = R.case_views(case)
    for c, cam in enumerate(d.pixel_source.camera_data.values()):
        maps = cam.lidar_depth_maps.numpy()
        r = ref["cams"][c]
        assert maps.dtype == np.float32 and np.array_equal(maps > 0, r["winner"] >= 0)
        assert np.all(np.abs(maps - r["depth"]) <= r["edepth"]), name
        # the winner from the reference's own map: the one candidate of the pixel whose depth the map holds
        H, W = cam.HEIGHT, cam.WIDTH
        winner = np.full(maps.shape, -1, np.int64)
        collisions = occupied = 0
        for v in range(maps.shape[0]):
            b, e = views[c][1][v]
            pr = R.project(views[c][0][v][:3], case["points"][perm][b:e], W, H)
            lin = np.where(pr["valid"], pr["py"] * W + pr["px"], -1)
            for p in np.unique(lin[lin >= 0]):
                rows = np.nonzero(lin == p)[0]
                hit = rows[np.abs(pr["z"][rows] - maps[v].reshape(-1)[p]) <= pr["ez"][rows]]
                assert len(hit) == 1, (name, c, v, p, len(hit))
                assert hit[0] == rows.max(), "the reference's serial index_put_ did not keep the last row"
                winner[v].reshape(-1)[p] = perm[b + hit[0]]
                occupied += 1
                collisions += len(rows) > 1
        assert np.array_equal(winner, r["winner"])
        print(f"{name} camera {c}: {collisions} of {occupied} occupied pixels had collisions; the highest row won every one")
        out[f"{name}_cam{c}_hw"] = np.array([H, W])
        out[f"{name}_cam{c}_intrinsics"], out[f"{name}_cam{c}_c2w"], out[f"{name}_cam{c}_images"] = (
            case["cams"][c]["intrinsics"], case["cams"][c]["c2w"], R.to_u8(case["cams"][c]["images"]))
        out[f"{name}_cam{c}_lidar2img"] = views[c][0]
        out[f"{name}_cam{c}_depth"] = maps
        out[f"{name}_cam{c}_winner"] = winner.astype(np.int32)
    for k in ("points", "timesteps", "sweep_times", "frame_times"):
        out[f"{name}_{k}"] = case[k]
    out[f"{name}_colors0"] = R.to_u8(case["colors0"])
    out[f"{name}_visible"], out[f"{name}_colors"], out[f"{name}_visible_all"] = vis, R.to_u8(col), vis_all
    d2 = ref_projection_dataset(R, LS, case)
    DD.project_lidar_pts_on_images(d2, delete_out_of_view_points=True)
    assert d2.lidar_source.origins.shape[0] == int(vis.sum()) and d2.lidar_source.visible_masks is None


def record_boxes(R, DD, LS, out):
    case = R.box_case(BOX_SEED)
    F, I = case["active"].shape
    full = R.boxes(case["points"], case["poses"], case["sizes"], case["active"])
    print(f"boxes: {len(full['decided'])} points, {int((~full['decided']).sum())} undecided dropped")
    case = R.keep_decided(case, full["decided"])
    for f in range(F):      # one batched float32 inverse of the active poses gives the reference's per-box inverses, bit for bit
        for i in range(I):
            if case["active"][f, i]:
                fi, ii = np.nonzero(case["active"])
                k = int(np.nonzero((fi == f) & (ii == i))[0][0])
                batched = torch.linalg.inv(torch.from_numpy(case["poses"][fi, ii]))[k]
                assert torch.equal(batched, torch.inverse(torch.from_numpy(case["poses"][f, i]))), (f, i)
    d = ref_box_dataset(R, LS, case)
    N = len(case["points"])
    seed_pts = torch.from_numpy(case["points"])
    by_type = {}
    for node_type in ("RigidNodes", "DeformableNodes"):
        ids = [i for i in range(I) if (case["types"][i] == R.RIGID) == (node_type == "RigidNodes")]
        eligible = case["active"] & np.isin(np.arange(I), ids)[None]
        ref = R.boxes(case["points"], case["poses"], case["sizes"], eligible, R.frame_ranges(case["timesteps"], F))
        assert ref["decided"].all()
        full = DD.get_init_objects(d, node_type, instance_max_pts=10 ** 9, only_moving=False)
        want_keys = [i for _, i in sorted((int(eligible[:, i].argmax()), i) for i in ids if eligible[:, i].any())]
        assert list(full.keys()) == want_keys, (list(full.keys()), want_keys)
        recs = np.array(ref["records"], np.int64).reshape(-1, 3)
        for i in want_keys:
            sel = recs[:, 0] == i
            pts = full[i]["pts"].numpy()
            assert full[i]["num_pts"] == int(sel.sum()) == len(pts)
            assert np.all(np.abs(pts - ref["o"][sel]) <= ref["eo"][sel])
            assert np.array_equal(full[i]["colors"].numpy(), case["colors"][recs[sel, 2]])
            out[f"box_{node_type}_full_{i}_pts"] = pts
        torch.manual_seed(SAMPLE_SEED)
        sampled = DD.get_init_objects(d, node_type, instance_max_pts=SAMPLE_MAX, only_moving=True, traj_length_thres=0.5)
        out[f"box_{node_type}_full_keys"] = np.array(want_keys, np.int64)
        out[f"box_{node_type}_sampled_keys"] = np.array(list(sampled.keys()), np.int64)
        counts = {i: full[i]["num_pts"] for i in want_keys}
        print(f"boxes {node_type}: instances {want_keys} with {[counts[i] for i in want_keys]} points; after only_moving and "
              f"instance_max_pts={SAMPLE_MAX}: {list(sampled.keys())} with {[v['num_pts'] for v in sampled.values()]}")
        for i, v in sampled.items():
            out[f"box_{node_type}_sampled_{i}_pts"], out[f"box_{node_type}_sampled_{i}_colors"] = v["pts"].numpy(), R.to_u8(v["colors"].numpy())
        by_type[node_type] = (counts, sampled)
    rigid_counts, rigid_sampled = by_type["RigidNodes"]
    assert 3 not in rigid_counts and any(c > SAMPLE_MAX for c in rigid_counts.values()) and any(0 < c < SAMPLE_MAX for c in rigid_counts.values())
    deform_counts, deform_sampled = by_type["DeformableNodes"]
    assert deform_counts.get(5) == 0 and 4 in deform_counts and 4 not in deform_sampled      # the empty box; the one that stands still
    valid = {i: None for i in (0, 1, 2, 4, 5)}
    kept = DD.filter_pts_in_boxes(d, seed_pts, valid, torch.from_numpy(case["colors"]), torch.arange(N))
    ref = R.boxes(case["points"], case["poses"], case["sizes"], case["active"], None, set(valid))
    inside = np.ones(N, bool)
    inside[kept["time"].numpy()] = False
    assert np.array_equal(inside, ref["inside"]) and np.array_equal(kept["pts"].numpy(), case["points"][~inside])
    both = R.boxes(case["points"], case["poses"], case["sizes"], case["active"], None, {1, 2})
    rows12 = [r[2] for r in both["records"]]
    assert len(rows12) > len(set(rows12)), "no point inside two overlapping boxes"
    print(f"boxes filter: {int(inside.sum())} of {N} points inside; {len(rows12) - len(set(rows12))} inside both overlapping boxes")
    for k in ("points", "timesteps", "poses", "sizes", "active", "types"):
        out[f"box_{k}"] = case[k]
    out["box_colors"] = R.to_u8(case["colors"])
    out["box_filter_instances"] = np.array(sorted(valid), np.int64)
    out["box_filter_inside"] = inside


def record_depth(R, PX, out):
    for k, (H, W, factor) in enumerate(R.DEPTH_CASES):
        m = R.depth_case(DEPTH_SEED + k, H, W)
        got = PX.sparse_lidar_map_downsampler(torch.from_numpy(m), factor).numpy()
        mine, _ = R.downsample(m, factor, np.float32)
        exact, n = R.downsample(m, factor)
        assert got.shape == mine.shape == R.output_size(H, W, factor)
        assert np.array_equal(got, mine), "the float32 restatement does not give torch's bits on the host"
        assert np.all(np.abs(got - exact) <= (n + 4) * R.U * np.abs(exact) * 1.01)
        assert (got == 0).any() and (exact[0, 0] == 0)
        out[f"depth{k}_map"], out[f"depth{k}_out"] = m, got
        print(f"downsampler {H}x{W} x{factor}: {got.shape}, {int((got == 0).sum())} cells without a hit; restatement bit-equal")


def main():
    from tests import lidar_ref64 as R
    dd, px, ls = import_reference_datasets()
    DD, LS = dd.DrivingDataset, ls.SceneLidarSource
    out = {}
    for name, spec in PROJECTION.items():
        record_projection(R, DD, LS, name, spec, out)
    record_boxes(R, DD, LS, out)
    record_depth(R, px, out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "node_pose_train.npz"))


if __name__ == "__main__":
    main()
