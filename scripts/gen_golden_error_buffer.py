#!/usr/bin/env python3
"""Golden vectors for the error-driven image sampler (bilateral_driving_amd/sampler.py, csrc/error_buffer.hip), produced by the
REFERENCE's own CameraData.update_image_error_maps (datasets/base/pixel_source.py:431-449), ScenePixelSource.update_image_error_maps
(:948-983) and ScenePixelSource.propose_training_image (:909-936), called on the CPU on bare objects that hold only the attributes
they read.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_error_buffer.py      (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

The reference's dataset modules are imported with the missing third-party modules stubbed, the way scripts/gen_golden_lidar.py does it
(its ``import_reference_datasets`` is used as it is).

The inputs come from tests/error_buffer_ref64.py (``golden_inputs``): 3 cameras x 25 frames of 5 x 7 pixels, a render that spans
[-0.2, 1.3], a dynamic opacity that straddles 0.1 and holds exactly 0.1f and its two neighbours, one camera without a dynamic pixel.
The reference receives what ``render_images`` would hand it: the render clamped to [0, 1] (models/video_utils.py:185-187).  The tensor
that the reference hands to ``torch.multinomial`` is captured by wrapping ``torch.multinomial`` for ``start_enhance_weight`` 1 and 3,
for 25 frames (2 boosted frames) and 9 frames (none), for every image and for a strided subset of candidates.

The script checks the restatement against the reference as it records: the maps within 6 * 2^-24 relative of the float64 mode (and
whether they are bit-equal to the float32 mode: ``maps_bit_equal``), the reference's float32 means within (n - 1) * 2^-24 relative of
the float64 ones (the measured distance: ``mean_rel_distance``), the captured weights within 2^-23 relative of the restatement's.

tests/golden/error_buffer.npz holds data only: the inputs (``pred``, ``gt``, ``dyn``), per camera the reference's maps (``maps``
[3,25,5,7]), its buffer (``buffer`` [75]), the captured tensors (``mn_w{weight}_f{frames}_{candidates}``), the flag and the distance."""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OUT = os.path.join(ROOT, "tests", "golden", "error_buffer.npz")


def reference_source(px, R, num_frames, weight, buffer_ratio=0.5):
    """A bare pixel source that runs the reference's own methods and properties."""
    PS = px.ScenePixelSource

    class Source:
        camera_list, num_cams, num_frames, num_imgs = PS.camera_list, PS.num_cams, PS.num_frames, PS.num_imgs
        buffer_ratio = PS.buffer_ratio
        update_image_error_maps, propose_training_image = PS.update_image_error_maps, PS.propose_training_image
        image_error_buffer, image_error_buffered = None, False
    s = Source()
    s.data_cfg = R._Cfg(range(R.CAMS), buffer_ratio, 1, weight)
    s._timesteps = torch.arange(num_frames)
    s.device = torch.device("cpu")
    s.camera_data = {}
    for c in range(R.CAMS):
        cam = object.__new__(px.CameraData)
        cam.cam_id, cam.cam_name, cam.device = c, R.CAM_NAMES[c], torch.device("cpu")
        cam.image_error_maps = torch.ones(num_frames, R.H, R.W)
        s.camera_data[c] = cam
    return s


def main():
    from tests import error_buffer_ref64 as R
    import gen_golden_lidar
    _, px, _ = gen_golden_lidar.import_reference_datasets()
    pred, gt, dyn = R.golden_inputs()
    n = R.H * R.W
    out = {"pred": pred, "gt": gt, "dyn": dyn}

    source = reference_source(px, R, R.FRAMES, None)
    source.update_image_error_maps(R.render_results(pred, gt, dyn))
    assert source.image_error_buffered
    maps = np.stack([source.camera_data[c].image_error_maps.numpy() for c in range(R.CAMS)])
    buffer = source.image_error_buffer.numpy()
    assert maps.dtype == np.float32 and maps.shape == (R.CAMS, R.FRAMES, R.H, R.W) and buffer.shape == (R.CAMS * R.FRAMES,)

    f32, f64 = R.error_map(pred, gt, dyn, np.float32), R.error_map(pred, gt, dyn, np.float64)
    rel = float(np.max(np.abs(maps.astype(np.float64) - f64) / f64))
    assert rel <= 6 * R.EPS32, rel
    bit_equal = bool(np.array_equal(maps.view(np.int32), f32.view(np.int32)))
    boosted = int(np.count_nonzero(dyn > R.DYN_THRESHOLD))
    assert boosted > 0 and not np.any(dyn[R.CAMS - 1] > R.DYN_THRESHOLD)
    assert np.any(dyn == R.DYN_THRESHOLD) and np.any(pred < 0) and np.any(pred > 1)
    print(f"maps: the reference's float32 within {rel:.2e} relative of float64 (bound {6 * R.EPS32:.2e}); bit-equal to the float32 "
          f"restatement: {bit_equal}; {boosted} boosted pixels")
    mean64 = maps.astype(np.float64).mean(axis=(2, 3))                      # [CAMS, FRAMES]; image = frame * CAMS + cam
    mean64 = mean64.T.reshape(-1)
    dist = float(np.max(np.abs(buffer.astype(np.float64) - mean64) / mean64))
    assert dist <= (n - 1) * R.EPS32, dist
    print(f"means: the reference's float32 within {dist:.2e} relative of the float64 ones (bound {(n - 1) * R.EPS32:.2e})")
    out.update(maps=maps, buffer=buffer, maps_bit_equal=np.bool_(bit_equal), mean_rel_distance=np.float64(dist))

    captured = []
    real = torch.multinomial

    def recording(inp, *args, **kwargs):
        captured.append(inp.detach().clone().numpy())
        return real(inp, *args, **kwargs)
    real_random = random.random
    torch.multinomial, random.random = recording, lambda: 0.0      # (0.0 < buffer_ratio: the weighted branch)
    try:
        for frames in (R.FRAMES, R.SHORT_FRAMES):
            for weight in R.WEIGHTS:
                s = reference_source(px, R, frames, weight)
                s.image_error_buffer, s.image_error_buffered = torch.from_numpy(buffer[:frames * R.CAMS].copy()), True
                for name, cands in R.candidate_lists(frames * R.CAMS).items():
                    del captured[:]
                    got = s.propose_training_image(cands)
                    assert len(captured) == 1 and got in cands
                    want = R.draw_weights(buffer[:frames * R.CAMS], cands, frames, R.CAMS, weight)
                    err = float(np.max(np.abs(captured[0].astype(np.float64) - want) / want))
                    assert captured[0].dtype == np.float32 and err <= 2.0 ** -23, (frames, weight, name, err)
                    print(f"multinomial input, {frames} frames, weight {weight}, {name}: {len(cands)} candidates, {err:.2e} from the restatement")
                    out[f"mn_w{weight}_f{frames}_{name}"] = captured[0]
    finally:
        torch.multinomial, random.random = real, real_random
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")
    assert os.path.getsize(OUT) <= 256 * 1024


if __name__ == "__main__":
    main()
