#!/usr/bin/env python3
"""Golden vectors for the pseudo-lidar generation (bilateral_driving_amd/pseudo_lidar.py, csrc/pseudo_lidar.hip), produced by the
REFERENCE's own depth_map_to_lidar_points / pto_ang_map_vertical (generate_lidar/generate_lidar_from_depth.py:42-162) and
gen_sparse_points / pto_ang_map (generate_lidar/depth2lidar.py:41-90), called on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_pseudo_lidar.py      (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

The imports are stubbed the way scripts/gen_golden_lidar.py does it: whatever the reference's modules import and the environment lacks
(open3d, OpenCV, tqdm) becomes an empty module; the functions use none of them.

The cases come from tests/pseudo_lidar_ref64.py.  Every pixel or point that the restatement there cannot DECIDE -- one that rounding
could move across a crop face, a fov limit or a beam edge, under the reference's two float32 products in any summation order or the
device's single matrix, plus the double rounding of the angles -- is invalidated before the reference runs (a depth pixel set to 0, a
cloud row dropped), so the recorded results hold for any float32 evaluation.  As it records, the script checks the restatement against
the reference: equal counts, each emitted point the highest-index candidate of its beam, coordinates within the reference route's
bound.

tests/golden/pseudo_lidar.npz: per depth case ("front": heavy collisions, depths beyond 80, zeros, a NaN, pixels outside the crop and
the fov; "side": a camera yawed 50 degrees against the lidar, so the edge-column clamp and x < 0 are populated; "slice": slice = 2,
H = 9, downscale_when_loading = 2) the depth map, intrinsics, poses, the reference's points and the winners' linear pixels; the cloud
case (classic mode through gen_sparse_points' crop, with intensity) likewise.  The file stays below tests/golden/node_pose_train.npz."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "pseudo_lidar.npz")


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def import_reference_generators():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    for _ in range(64):
        try:
            return (importlib.import_module("generate_lidar.generate_lidar_from_depth"), importlib.import_module("generate_lidar.depth2lidar"))
        except ModuleNotFoundError as e:
            sys.modules[e.name] = _Anything(e.name)
    raise RuntimeError("could not import the reference's generate_lidar modules")


def check_against_reference(R, name, ref, got, bound, width=3):
    """got [M,3|4] float64 from the reference against the restatement's winners."""
    assert ref["decided"].all() and not ref["dirty"].any(), name
    src, cells = ref["emitted"], ref["cells"]
    assert got.dtype == np.float64 and got.shape == (len(src), width), (name, got.shape, len(src))
    err = np.abs(got[:, :3] - ref["p"][src])
    assert np.all(err <= bound[src]), (name, float((err / np.maximum(bound[src], 1e-300)).max()))
    # the winner is the HIGHEST index of its beam: no lower candidate of a collided beam explains the emitted point better
    collided = runner_up_fits = 0
    for k, c in enumerate(cells):
        cand = np.nonzero(ref["cell"] == c)[0]
        assert cand.max() == src[k]
        if len(cand) > 1:
            collided += 1
            others = cand[cand != src[k]]
            runner_up_fits += int(np.any(np.all(np.abs(got[k, :3] - ref["p"][others]) <= bound[others], axis=1)))
    assert collided > len(cells) // 3, (name, collided, len(cells))
    assert runner_up_fits <= collided // 20, (name, runner_up_fits, collided)
    print(f"{name}: {len(src)} beams emitted, {collided} with collisions (the highest index won every one; in {runner_up_fits} a lower "
          f"candidate also lies within the bound), worst coordinate error {err.max():.2e} m")
    return src


def record_depth(R, GD, name, spec, out):
    spec = dict(spec)
    case = R.street_case(spec.pop("seed"), **spec)
    ref = R.depth_reference(case)
    und = int((~ref["decided"]).sum())
    case = R.invalidate_undecided(case, ref)
    ref = R.depth_reference(case)
    stats = R.case_stats(ref)
    print(f"{name}: {case['depth'].size} pixels, {stats[2]} live, {und} undecided set to 0")
    Hi, Wi = case["depth"].shape
    got = GD.depth_map_to_lidar_points(torch.from_numpy(case["depth"]), torch.from_numpy(case["K"]), torch.from_numpy(case["c2w"]), Wi, Hi,
                                       torch.from_numpy(case["l2w"]), H=case["H"], W=case["W"], slice=case["slice"],
                                       downscale_when_loading=case["downscale"])
    src = check_against_reference(R, name, ref, got, ref["e_ref"])
    d = case["depth"]
    with np.errstate(invalid="ignore"):
        assert (d == 0).sum() > 10 and (d >= 80).sum() > 10 and np.isnan(d).any()
    assert (ref["valid"] & ~ref["live"]).sum() > 50      # outside the crop or the fov
    if name == "side":
        x, y = ref["p"][:, 0], ref["p"][:, 1]
        v = ref["valid"]
        assert (v & (x < 0)).sum() > 50 and (ref["live"] & (np.arctan2(y, x) > np.radians(45.5))).sum() > 50      # x < 0; the clamp to column 0
    for k in ("depth", "K", "c2w", "l2w"):
        out[f"{name}_{k}"] = case[k]
    out[f"{name}_points"], out[f"{name}_source"] = got, src.astype(np.int32)


def record_cloud(R, GD, D2, out):
    spec = dict(R.GOLDEN_CLOUD)
    case = R.cloud_case(spec.pop("seed"), **spec)
    ref = R.cloud_reference(case)
    print(f"cloud: {len(case['cloud'])} rows, {int((~ref['decided']).sum())} undecided dropped")
    case = R.invalidate_undecided(case, ref)
    ref = R.cloud_reference(case)
    args = types.SimpleNamespace(H=case["H"], W=case["W"], slice=case["slice"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "000000.bin")
        case["cloud"].tofile(path)
        got = D2.gen_sparse_points(path, args)
    src = check_against_reference(R, "cloud", ref, got, np.full((len(case["cloud"]), 3), 0.0), width=4)
    assert np.array_equal(got, case["cloud"][src].astype(np.float64))      # rows copied: intensity too
    assert (~ref["live"]).sum() > 100
    out["cloud_points"], out["cloud_out"], out["cloud_source"] = case["cloud"], got.astype(np.float32), src.astype(np.int32)
    # pto_ang_map_vertical called directly, no crop: the same cloud through the other row rule
    vcase = dict(case, mode="vertical", crop=None, H=16)
    vref = R.cloud_reference(vcase)
    keep = vref["decided"]
    vgot = GD.pto_ang_map_vertical(case["cloud"][keep].astype(np.float64), H=16, W=case["W"], slice=1)
    vref2 = R.cloud_reference(dict(vcase, cloud=case["cloud"][keep]))
    vsrc = np.nonzero(keep)[0][vref2["emitted"]]
    assert vgot.shape == (len(vsrc), 4) and np.array_equal(vgot, case["cloud"][vsrc].astype(np.float64))
    out["cloud_vertical_keep"], out["cloud_vertical_source"] = keep, vsrc.astype(np.int32)
    print(f"cloud, vertical rule: {len(vsrc)} beams emitted of {int(keep.sum())} decided rows")


def main():
    from tests import pseudo_lidar_ref64 as R
    GD, D2 = import_reference_generators()
    out = {}
    for name, spec in R.GOLDEN_DEPTH.items():
        record_depth(R, GD, name, spec, out)
    record_cloud(R, GD, D2, out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "node_pose_train.npz"))


if __name__ == "__main__":
    main()
