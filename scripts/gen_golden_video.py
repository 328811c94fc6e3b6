#!/usr/bin/env python3
"""Golden vectors for the evaluation video frames (bilateral_driving_amd/video.py, csrc/video.hip), produced by the REFERENCE's own
``to8b``, ``depth_visualizer`` and ``layout_*`` (utils/visualization.py:19-22, 41-341, 412-497), the expressions of ``render``
(models/video_utils.py:201-227, 265-271) and ``save_concatenated_videos`` / ``save_seperate_videos`` (:703-857), called on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_video.py      (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

The reference's modules are imported with the missing third-party modules stubbed, the way scripts/gen_golden_lidar.py does it (OpenCV
for utils/visualization.py; for models/video_utils.py also scikit-image, and ``imageio`` as a module whose ``get_writer`` records what it
is given).

The inputs come from tests/video_ref64.py.  Recorded, as data only, into tests/golden/video_frames.npz:

* ``turbo8`` [256,3]: matplotlib's ``turbo`` through ``to8b`` (asserted equal from float64 and after a float32 cast);
* ``layout_<case>``: per layout case (every camera, three cameras, one camera of each of the six layouts, waymo with short side cameras,
  argoverse's two rear cameras in both orders, one nuscenes slot named twice) the reference's tiled canvas of constant images after ``to8b``;
* ``depth_in``, ``opacity_in``, ``weight_in`` and ``depth_rgb``, ``depth_rgb_bool``: ``to8b(depth_visualizer(d, o).astype(float32))``;
* ``lidar_rgb``, ``green_rgb`` with their inputs: the reference's expressions for lidar-on-image and the per-class composite;
* ``concat_<type>`` [T,Hc,Wc,3], ``concat_<type>_returned``, and per key ``separate_<type>_<key>`` [T,...] with
  ``separate_<type>_returned_<key>`` and ``separate_<type>_paths``: what the recording writers received from the two functions for
  waymo (3 cameras) and nuscenes (6 cameras).

The script checks the restatement against the reference as it records: layouts, quantiser, over-green and the pixel branch of
lidar-on-image bit-equal; depth colours under tests/video_ref64.py's rule (the counts are printed and recorded as ``*_differing``)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "tests", "golden", "video_frames.npz")


def import_reference_video(writers):
    """(utils.visualization, models.video_utils) of the reference; ``writers``: the list that every created writer is appended to."""
    import gen_golden_lidar as GL
    from tests import video_ref64 as R
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    imageio = types.ModuleType("imageio")
    imageio.get_writer = R.writer_factory(writers)
    imageio.imwrite = lambda path, image: None
    sys.modules["imageio"] = imageio
    for _ in range(64):
        try:
            vis = importlib.import_module("utils.visualization")
            vu = importlib.import_module("models.video_utils")
            return vis, vu
        except ModuleNotFoundError as e:
            sys.modules[e.name] = GL._Anything(e.name)
        except ImportError as e:      # "cannot import name X from <stub>"
            if e.name is None or e.name not in sys.modules:
                raise
            sys.modules[e.name] = GL._Anything(e.name)
    raise RuntimeError("could not import the reference's video modules")


def main():
    from tests import video_ref64 as R
    writers = []
    vis, vu = import_reference_video(writers)
    out = {}

    import matplotlib
    lut = matplotlib.colormaps["turbo"](np.arange(256))[:, :3]
    turbo8 = vis.to8b(lut.astype(np.float32))
    assert np.array_equal(turbo8, vis.to8b(lut)) and turbo8.shape == (256, 3) and turbo8.dtype == np.uint8
    out["turbo8"] = R.TURBO8 = turbo8

    # ---- layouts ----
    for label, t, names, sizes in R.layout_cases():
        imgs = R.constant_images(sizes)
        ref = vis.to8b(vis.get_layout(t)(imgs, names))
        mine = R.to8b(R.layout(t, imgs, names))
        assert ref.dtype == np.uint8 and np.array_equal(ref, mine), label
        out[f"layout_{label}"] = ref
        print(f"layout {label}: {names} -> {ref.shape}")
    for t, names, sizes in R.ERRORS:
        for fn in (lambda: vis.get_layout(t)(R.constant_images(sizes), names), lambda: R.layout(t, R.constant_images(sizes), names)):
            try:
                fn()
            except ValueError:
                continue
            raise AssertionError(("no ValueError", t, names, sizes))

    # ---- depth ----
    depth, opacity, weight = R.depth_case()
    with np.errstate(all="ignore"):
        for tag, w in (("depth_rgb", opacity), ("depth_rgb_bool", weight)):
            ref = vis.to8b(vis.depth_visualizer(depth.copy(), w.copy()).astype(np.float32))
            n = R.depth_rule(ref, depth, w)
            n32 = int(np.any(R.depth_image(depth, w, np.float32) != R.depth_image(depth, w, np.float64), axis=-1).sum())
            print(f"{tag}: the reference differs from the float64 restatement on {n} of {depth.size} pixels, the float32 mode on {n32}")
            out[tag], out[tag + "_differing"] = ref, np.int64(n)
    out.update(depth_in=depth, opacity_in=opacity, weight_in=weight)

    # ---- lidar on image and over green: the expressions of render() ----
    rgb, op, lidar = R.rgb_case(17, 23)
    with np.errstate(all="ignore"):      # the operations of render() on the same operand types: float32 * int64 + float64 * bool
        hit = (lidar > 0)[..., None]
        blended = (rgb * (1 - hit) + vis.depth_visualizer(lidar.copy(), lidar > 0) * hit).astype(np.float32)
        ref = R.to8b(blended)             # (the reference's to8b, with a NaN pixel sent to 0)
        finite = ~np.isnan(blended)
        assert blended.shape == rgb.shape and np.array_equal(ref[finite], vis.to8b(blended)[finite])
    mine = R.lidar_on_image(rgb, lidar)
    shown = lidar > 0
    assert np.array_equal(ref[~shown], mine[~shown])
    out["lidar_differing"] = np.int64(R.depth_rule(ref, lidar, shown, shown))
    out.update(lidar_rgb=ref, lidar_pixels_in=rgb, lidar_depth_in=lidar)

    alpha = torch.from_numpy(op)[..., None]      # torch's float32 ops, as render() applies them: the clamp of every rgb result first
    green = torch.tensor([0.0, 177, 64]) / 255.0
    ref = (torch.from_numpy(rgb).clamp(0., 1.) * alpha + green * (1 - alpha)).numpy()
    mine = R.over_green(rgb, op, np.float32)
    ok = ~np.isnan(ref)
    assert np.array_equal(ref.view(np.int32)[ok], mine.view(np.int32)[ok]) and np.array_equal(np.isnan(ref), np.isnan(mine))
    out.update(green_rgb=R.to8b(ref), green_float=ref, green_rgb_in=rgb, green_opacity_in=op)
    assert np.array_equal(vis.to8b(ref)[ok], out["green_rgb"][ok])

    # ---- merged frames ----
    for t, names in R.MERGED.items():
        rr = R.render_results(t, names, short_sides=False)
        num_cams, T = len(names), R.MERGED_T
        del writers[:]
        got = vu.save_concatenated_videos({k: list(v) for k, v in rr.items()}, "video.mp4", vis.get_layout(t), T, keys=list(R.MERGED_KEYS),
                                          num_cams=num_cams, verbose=False)
        assert len(writers) == 1 and writers[0].closed and len(writers[0].frames) == T and list(got) == ["concatenated_frame"]
        frames = np.stack(writers[0].frames)
        differing = 0
        for i in range(T):
            differing += R.frame_rule(frames[i], R.merged_frame(t, rr, R.MERGED_KEYS, i, num_cams))
        assert np.array_equal(got["concatenated_frame"], frames[T // 2])
        out[f"concat_{t}"], out[f"concat_{t}_returned"], out[f"concat_{t}_differing"] = frames, got["concatenated_frame"], np.int64(differing)
        print(f"concatenated {t}: {frames.shape}, {differing} pixels differ from the float64 restatement")

        del writers[:]
        got = vu.save_seperate_videos({k: list(v) for k, v in rr.items()}, "video.mp4", vis.get_layout(t), T, keys=list(R.MERGED_KEYS),
                                      num_cams=num_cams)
        assert [w.path for w in writers] == [f"video_{k}.mp4" for k in R.MERGED_KEYS]
        out[f"separate_{t}_paths"] = np.array([w.path for w in writers])
        out[f"separate_{t}_written"] = np.array([len(w.frames) for w in writers])
        out[f"separate_{t}_returned"] = np.array(list(got))
        for w, key in zip(writers, R.MERGED_KEYS):
            if not w.frames:
                assert key not in got and R.key_canvas(t, rr, key, 0, num_cams) is None, key
                continue
            frames = np.stack(w.frames)
            for i in range(T):
                R.frame_rule(frames[i], R.key_canvas(t, rr, key, i, num_cams))
            assert np.array_equal(got[key], frames[T // 2])
            out[f"separate_{t}_{key}"], out[f"separate_{t}_returned_{key}"] = frames, got[key]
        print(f"separate {t}: written {dict(zip(R.MERGED_KEYS, out[f'separate_{t}_written'].tolist()))}, returned {list(got)}")

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")
    assert os.path.getsize(OUT) <= 256 * 1024


if __name__ == "__main__":
    main()
