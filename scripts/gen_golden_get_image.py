#!/usr/bin/env python3
"""Golden vectors for a view's input preparation (bilateral_driving_amd/pixels.py, csrc/pixels.hip), produced by the REFERENCE's own
CameraData.get_image (datasets/base/pixel_source.py:477-657) and ScenePixelSource.prepare_novel_view_render_data (:1070-1132), called
on the CPU on bare objects that hold only the attributes they read.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_get_image.py        (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

The reference's dataset modules are imported with the missing third-party modules stubbed, the way scripts/gen_golden_lidar.py does it
(its ``import_reference_datasets`` is used as it is).

The camera comes from tests/get_image_ref64.py (``golden_inputs``): 3 frames of 12 x 20, all five masks, the egocar mask, a sparse
lidar map, ``normalized_time``.  ``get_image`` runs for every frame at the factors 1.0, 0.5 and 0.25, and
``prepare_novel_view_render_data`` for 3 poses.  The script checks the restatement against the reference as it records: integer fields,
``pixel_coords``, ``origins``, masks, the lidar map and the intrinsics bit for bit in the float32 mode, ``viewdirs``, ``direction_norm``
and the resized image within the measured bound of the float64 mode.

tests/golden/get_image.npz holds data only: the inputs (``cam_*``, ``traj``), per factor and frame the reference's outputs
(``f{factor}_{frame}_{key}``) and per pose the novel view's (``novel_{i}_{key}``)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "tests", "golden", "get_image.npz")
EXACT = ("pixel_coords", "origins", "normed_time", "img_idx", "frame_idx", "sky_masks", "dynamic_masks", "human_masks", "vehicle_masks",
         "egocar_masks", "lidar_depth_map", "cam_id", "camera_to_world", "height", "width", "intrinsics")
BOUNDED = ("viewdirs", "direction_norm", "pixels")


def bare_camera(CameraData, cam, factor):
    c = object.__new__(CameraData)
    for k, v in cam.items():
        setattr(c, k, torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) and v.ndim else int(v))
    c.load_size = tuple(cam["images"].shape[1:3])
    c.downscale_factor, c.device, c.cam_name, c.image_error_maps = factor, torch.device("cpu"), "front_camera", None
    return c


def as_numpy(d):
    return {k: (v.detach().contiguous().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items() if k != "cam_name"}


def check(R, got, exact, f32, label):
    for k, v in got.items():
        v = np.asarray(v)
        if k in BOUNDED:
            b = R.bound(f32[k], exact[k])
            err = float(np.max(np.abs(v.astype(np.float64) - exact[k])))
            assert v.shape == exact[k].shape and err <= b, (label, k, err, b)
            print(f"  {label} {k}: reference's float32 within {err:.2e} of float64 (restatement's float32: bound {b:.2e})")
        else:
            assert k in EXACT, k
            assert v.dtype == np.asarray(f32[k]).dtype and np.array_equal(v, f32[k]), (label, k)


def main():
    from tests import get_image_ref64 as R
    import gen_golden_lidar
    _, px, _ = gen_golden_lidar.import_reference_datasets()
    cam, traj = R.golden_inputs()
    out = {f"cam_{k}": v for k, v in cam.items()}
    out["traj"] = traj
    for factor in R.FACTORS:
        for frame in range(R.GOLDEN_FRAMES):
            info, cams = px.CameraData.get_image(bare_camera(px.CameraData, cam, factor), frame)
            assert cams["cam_name"] == "front_camera"
            got = {**as_numpy(info), **as_numpy(cams)}
            e_info, e_cams = R.get_image(cam, frame, factor, np.float64)
            s_info, s_cams = R.get_image(cam, frame, factor, np.float32)
            assert sorted(got) == sorted({**e_info, **e_cams})
            check(R, got, {**e_info, **e_cams}, {**s_info, **s_cams}, f"factor {factor} frame {frame}")
            for k, v in got.items():
                out[f"f{factor}_{frame}_{k}"] = np.asarray(v)
    source = type("Source", (), {})()
    source.camera_data = {0: bare_camera(px.CameraData, cam, 1.0)}
    source.num_frames, source.device = 7, torch.device("cpu")
    views = px.ScenePixelSource.prepare_novel_view_render_data(source, "waymo", torch.from_numpy(traj))
    exact, f32 = R.novel_views(cam, traj, 7, np.float64), R.novel_views(cam, traj, 7, np.float32)
    assert len(views) == R.GOLDEN_POSES
    for i, view in enumerate(views):
        got = as_numpy(view["image_infos"])
        check(R, got, exact[i], f32[i], f"novel view {i}")
        ci = view["cam_infos"]
        assert sorted(ci) == ["camera_to_world", "height", "intrinsics", "width"] and tuple(ci["height"].shape) == (1,)
        assert int(ci["height"][0]) == R.GOLDEN_H and int(ci["width"][0]) == R.GOLDEN_W and torch.equal(ci["intrinsics"], torch.from_numpy(cam["intrinsics"][0]))
        for k, v in got.items():
            out[f"novel_{i}_{k}"] = v
    out["novel_num_frames"] = np.int64(7)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")
    assert os.path.getsize(OUT) <= 256 * 1024


if __name__ == "__main__":
    main()
