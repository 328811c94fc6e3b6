"""A view's input preparation on the MI355X (csrc/pixels.hip through bilateral_driving_amd/pixels.py) against the reference's recorded
results (tests/golden/get_image.npz) and the numpy restatement (tests/get_image_ref64.py, pinned to the reference by
tests/test_get_image_cpu.py).

Integer fields, ``pixel_coords``, ``origins``, the fills, the masks, the lidar map and the intrinsics are compared by bits.
``viewdirs``, ``direction_norm`` and the antialiased image are held to MEASURED bounds (get_image_ref64.bound): the float32 framework
expression -- the restatement's float32 mode, for the image also torch's own float32 resize on the host -- is first measured against
float64 on the same inputs, the kernel is allowed four times that distance, at least 1e-6 absolute; every test prints the figures.
The shapes are the smallest that cross what the kernels cross: a view of one pixel, pixel counts with every remainder modulo 4 (a
16-byte store must not run past a tail), 65 pixels (a wave's edge), 1221 pixels (a workgroup's edge with four pixels per lane), a batch
whose later views start at a flat pixel that is no multiple of four, resize tiles cut by the image's edges at every factor.

Figures measured on the MI355X (this file's own prints):
  view_fields  viewdirs at most 1.4e-07 and direction_norm at most 3.3e-07 (at scale 0.3; 1.8e-07 at scale 1) from float64 over
               every shape, bit-equal to the restatement's float32 mode; every bound is the floor, 1e-06
  resize_image at most 3.7e-07 from torch's float64 down to 1/16 (64x96 at 1/3, a step edge: torch's float32 3.5e-07, bound 1.4e-06;
               the other bounds are the floor but two step edges at 1.02e-06 and 1.03e-06), 7.4e-07 at 1/40 (163-tap windows:
               torch's float32 4.6e-07 - 6.2e-07, bounds 1.9e-06 - 2.5e-06); a constant image stays constant to 3.0e-07
  get_image    the golden cases: viewdirs 1.3e-07, direction_norm 1.5e-07, pixels 1.3e-07 from float64 (the reference's float32:
               1.1e-07, 1.5e-07, 1.1e-07)"""
import functools

import numpy as np
import pytest
import torch

from tests import get_image_ref64 as R
from tests.poison import holds_poison, poisoned_allocations

pytestmark = pytest.mark.gpu

VIEW_SHAPES = ((1, 1), (3, 5), (7, 9), (5, 13), (33, 37), (40, 64))
RESIZE_CASES = ((13, 21, 0.5), (17, 23, 0.25), (9, 9, 0.3), (31, 45, 0.125), (64, 96, 1.0 / 3.0), (70, 150, 0.5),
                (72, 100, 1.0 / 16.0), (90, 130, 1.0 / 40.0))      # the last two: windows so long that the tile is cut to 2 x 32 and to 1 x 16
MASK_FACTORS = (0.5, 0.25, 0.3, 1.0 / 3.0)
EXACT_INFO = ("pixel_coords", "origins", "normed_time", "img_idx", "frame_idx", "lidar_depth_map") + R.MASK_KEYS


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import pixels
    return pixels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().contiguous().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def distance(got, exact):
    return float(np.max(np.abs(np.asarray(got, np.float64) - exact), initial=0.0))


@functools.lru_cache(maxsize=None)
def view_ref(H, W, B, far, scale):
    """The restatement of a random batch in both modes, computed once."""
    case = R.view_case(H * 1000 + W * 10 + B, B, H, W, far)
    exact = [R.rays(case["c2w"][b], case["K"][b], scale, H, W, np.float64) for b in range(B)]
    f32 = [R.rays(case["c2w"][b], case["K"][b], scale, H, W, np.float32) for b in range(B)]
    return case, exact, f32


def check_views(got, case, exact, f32, H, W, scale, with_time, with_cam, label):
    B = len(exact)
    assert tuple(got["origins"].shape) == (B, H, W, 3) and tuple(got["direction_norm"].shape) == (B, H, W, 1)
    assert tuple(got["pixel_coords"].shape) == (B, H, W, 2) and tuple(got["intrinsics"].shape) == (B, 3, 3)
    assert ("normed_time" in got) == with_time and ("cam_id" in got) == with_cam
    worst = {"viewdirs": 0.0, "direction_norm": 0.0}
    for b in range(B):
        assert same_bits(host(got["origins"][b]), f32[b][0]) and same_bits(host(got["pixel_coords"][b]), f32[b][3])
        assert same_bits(host(got["intrinsics"][b]), R.scaled_intrinsics(case["K"][b], scale))
        assert same_bits(host(got["img_idx"][b]), np.full((H, W), case["img"][b], np.int64))
        assert same_bits(host(got["frame_idx"][b]), np.full((H, W), case["frame"][b], np.int64))
        if with_time:
            assert same_bits(host(got["normed_time"][b]), np.full((H, W), case["time"][b], np.float32))
        if with_cam:
            assert same_bits(host(got["cam_id"][b]), np.full((H, W), case["cam"][b], np.int64))
        for k, i in (("viewdirs", 1), ("direction_norm", 2)):
            bound, err = R.bound(f32[b][i], exact[b][i]), distance(host(got[k][b]), exact[b][i])
            worst[k] = max(worst[k], err)
            assert err <= bound, (label, b, k, err, bound)
            assert same_bits(host(got[k][b]), f32[b][i]), (label, b, k)      # every operation rounded on its own
    print(f"\nview_fields {label}: viewdirs {worst['viewdirs']:.2e}, direction_norm {worst['direction_norm']:.2e} from float64 "
          f"(the float32 expression: {max(distance(f[1], e[1]) for f, e in zip(f32, exact)):.2e}, {max(distance(f[2], e[2]) for f, e in zip(f32, exact)):.2e})")


def run_views(P, case, H, W, scale, with_time, with_cam):
    return P.view_fields(dev(case["c2w"]), dev(case["K"]), H, W, scale=scale, normed_time=case["time"] if with_time else None,
                         img_idx=case["img"], frame_idx=case["frame"], cam_id=case["cam"] if with_cam else None)


# ---- the reference's recorded results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", R.FACTORS)
def test_get_image_equals_the_reference(P, factor):
    z = R.golden()
    cam, _ = R.golden_camera()
    obj = R.BareCamera(cam, factor, "cuda")
    Ho, Wo = R.output_size(R.GOLDEN_H, R.GOLDEN_W, factor)
    for frame in range(R.GOLDEN_FRAMES):
        with poisoned_allocations(True, name=f"get_image x{factor} frame {frame}"):
            info, cams = P.get_image(obj, frame)
            for v in list(info.values()) + [v for v in cams.values() if isinstance(v, torch.Tensor)]:
                assert v.is_cuda and not bool(holds_poison(v).any())
        gold = {k.split("_", 2)[2]: z[k] for k in z if k.startswith(f"f{factor}_{frame}_")}
        assert list(info) == ["origins", "viewdirs", "direction_norm", "pixel_coords", "normed_time", "img_idx", "frame_idx", "pixels",
                              "sky_masks", "dynamic_masks", "human_masks", "vehicle_masks", "egocar_masks", "lidar_depth_map"]
        assert list(cams) == ["cam_id", "cam_name", "camera_to_world", "height", "width", "intrinsics"] and cams["cam_name"] == "front_camera"
        for k in EXACT_INFO:
            assert same_bits(host(info[k]), gold[k]), (factor, frame, k)
        for k in ("cam_id", "camera_to_world", "height", "width", "intrinsics"):
            assert same_bits(host(cams[k]), gold[k]), (factor, frame, k)
        assert cams["height"].dim() == 0 and cams["height"].dtype == torch.int64 and int(cams["height"]) == Ho and int(cams["width"]) == Wo
        assert cams["intrinsics"].data_ptr() != obj.intrinsics[frame].data_ptr()
        assert cams["camera_to_world"].data_ptr() == obj.cam_to_worlds[frame].data_ptr()
        exact, f32 = R.get_image(cam, frame, factor, np.float64)[0], R.get_image(cam, frame, factor, np.float32)[0]
        for k in ("viewdirs", "direction_norm", "pixels"):
            bound, err = R.bound(f32[k], exact[k]), distance(host(info[k]), exact[k])
            print(f"\nget_image x{factor} frame {frame} {k}: {err:.2e} from float64 (the float32 expression {distance(f32[k], exact[k]):.2e}, the "
                  f"reference's float32 {distance(gold[k], exact[k]):.2e}; bound {bound:.2e})")
            assert info[k].dtype == torch.float32 and tuple(info[k].shape) == exact[k].shape and info[k].is_contiguous() and err <= bound
    again = P.get_image(obj, 1)[0]
    once = P.get_image(obj, 1)[0]
    assert all(torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                           once[k].view(torch.int32) if once[k].dtype == torch.float32 else once[k]) for k in again)


def test_get_image_drops_what_the_camera_lacks_and_takes_device_indices(P):
    cam, _ = R.golden_camera()
    obj = R.BareCamera(cam, 0.5, "cuda")
    obj.sky_masks = obj.human_masks = obj.lidar_depth_maps = obj.normalized_time = None
    info, cams = P.get_image(obj, 2)
    assert list(info) == ["origins", "viewdirs", "direction_norm", "pixel_coords", "img_idx", "frame_idx", "pixels", "dynamic_masks",
                          "vehicle_masks", "egocar_masks"]
    full = P.get_image(R.BareCamera(cam, 0.5, "cuda"), 2)[0]
    assert all(torch.equal(info[k], full[k]) for k in info)
    # indices and times that live on the device are stacked there
    on_dev = R.BareCamera(cam, 0.5, "cuda")
    on_dev.normalized_time, on_dev.unique_img_idx = on_dev.normalized_time.cuda(), on_dev.unique_img_idx.cuda()
    info2, cams2 = P.get_image(on_dev, torch.tensor(2, device="cuda"))
    assert all(torch.equal(info2[k], full[k]) for k in full) and int(cams2["height"]) == 6 and int(cams2["width"]) == 10
    assert torch.equal(cams2["cam_id"], cams["cam_id"])
    # installed on a class: an object on the device takes the kernel, one on the CPU the class's own method
    class Camera(R.BareCamera):
        def get_image(self, frame_idx):
            return "former"
    P.install(Camera)
    try:
        assert Camera(cam, 1.0, "cpu").get_image(0) == "former"
        got = Camera(cam, 0.5, "cuda").get_image(2)[0]
        assert all(torch.equal(got[k], full[k]) for k in full)
    finally:
        P.uninstall()
    assert Camera(cam, 0.5, "cuda").get_image(2) == "former"


def test_novel_views_equal_the_reference(P):
    z = R.golden()
    cam, traj = R.golden_camera()
    n = int(z["novel_num_frames"])
    second = dict(cam, intrinsics=cam["intrinsics"] * np.float32(1.25))
    src = R.bare_pixel_source(cam, "cuda", n, second)
    t = dev(traj)
    with poisoned_allocations(True, name="novel views"):
        views = P.prepare_novel_view_render_data(src, "waymo", t)
        for view in views:
            assert not any(bool(holds_poison(v).any()) for v in view["image_infos"].values())
    exact = R.novel_views(cam, traj, n, np.float64)
    f32 = R.novel_views(cam, traj, n, np.float32)
    assert len(views) == R.GOLDEN_POSES
    for i, view in enumerate(views):
        info, cams = view["image_infos"], view["cam_infos"]
        assert sorted(cams) == ["camera_to_world", "height", "intrinsics", "width"] and "cam_id" not in info
        assert tuple(cams["height"].shape) == (1,) and cams["height"].dtype == torch.int64 and int(cams["height"][0]) == R.GOLDEN_H
        assert int(cams["width"][0]) == R.GOLDEN_W and cams["intrinsics"].data_ptr() == src.camera_data[0].intrinsics[0].data_ptr()
        assert cams["camera_to_world"].data_ptr() == t[i].data_ptr()
        assert sorted(info) == sorted(["origins", "viewdirs", "direction_norm", "img_idx", "frame_idx", "normed_time", "pixel_coords"])
        for k in ("pixel_coords", "origins", "normed_time", "img_idx", "frame_idx"):
            assert same_bits(host(info[k]), z[f"novel_{i}_{k}"]), (i, k)
        for k in ("viewdirs", "direction_norm"):
            bound, err = R.bound(f32[i][k], exact[i][k]), distance(host(info[k]), exact[i][k])
            print(f"\nnovel view {i} {k}: {err:.2e} from float64 (bound {bound:.2e})")
            assert err <= bound and tuple(info[k].shape) == exact[i][k].shape
    other = P.prepare_novel_view_render_data(src, "argoverse", t)      # camera 1
    assert other[0]["cam_infos"]["intrinsics"].data_ptr() == src.camera_data[1].intrinsics[0].data_ptr()
    assert not torch.equal(other[1]["image_infos"]["viewdirs"], views[1]["image_infos"]["viewdirs"])
    assert P.prepare_novel_view_render_data(src, "waymo", t[:0]) == []


# ---- view_fields ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", VIEW_SHAPES)
def test_view_fields_match_the_restatement(P, shape, B):
    H, W = shape
    case, exact, f32 = view_ref(H, W, B, 0.0, 1.0)
    with poisoned_allocations(True, name=f"view_fields {H}x{W} B={B}"):
        got = run_views(P, case, H, W, 1.0, True, True)
        assert not any(bool(holds_poison(v).any()) for v in got.values())      # no element left unwritten; the guards: on exit
    check_views(got, case, exact, f32, H, W, 1.0, True, True, f"{H}x{W} B={B}")
    again = run_views(P, case, H, W, 1.0, True, True)
    assert all(torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]) for k in got)      # determinism


@pytest.mark.parametrize("spec", [("no time, no camera", 5, 13, 3, 0.0, 1.0, False, False), ("no time", 3, 5, 3, 0.0, 1.0, False, True),
                                  ("a pose 1000 m out", 7, 9, 3, 1000.0, 1.0, True, True), ("scale 0.5", 33, 37, 3, 0.0, 0.5, True, True),
                                  ("scale 0.3", 7, 9, 1, 0.0, 0.3, True, False)])
def test_view_fields_options(P, spec):
    label, H, W, B, far, scale, with_time, with_cam = spec
    case, exact, f32 = view_ref(H, W, B, far, scale)
    with poisoned_allocations(True, name=f"view_fields {label}"):
        got = run_views(P, case, H, W, scale, with_time, with_cam)
        assert not any(bool(holds_poison(v).any()) for v in got.values())
    check_views(got, case, exact, f32, H, W, scale, with_time, with_cam, label)
    if far:
        assert float(np.linalg.norm(case["c2w"][0][:3, 3])) > 900.0


def test_view_fields_shapes_and_shared_intrinsics(P):
    H, W = 7, 9
    case, exact, f32 = view_ref(H, W, 3, 0.0, 1.0)
    shared = P.view_fields(dev(case["c2w"]), dev(case["K"][1]), H, W, normed_time=0.25, img_idx=7, frame_idx=torch.tensor([1, 2, 3]), cam_id=4)
    own = P.view_fields(dev(case["c2w"][1]), dev(case["K"][1]), H, W, normed_time=0.25, img_idx=7, frame_idx=2, cam_id=4)
    assert tuple(own["viewdirs"].shape) == (H, W, 3) and tuple(own["intrinsics"].shape) == (3, 3) and tuple(own["img_idx"].shape) == (H, W)
    assert all(torch.equal(own[k], shared[k][1]) for k in own)
    assert bool((shared["frame_idx"][2] == 3).all()) and bool((shared["img_idx"] == 7).all()) and bool((shared["normed_time"] == 0.25).all())
    on_dev = P.view_fields(dev(case["c2w"]), dev(case["K"][1:2]), H, W, normed_time=torch.full((3,), 0.25, device="cuda"),
                           img_idx=torch.tensor([7], device="cuda"), frame_idx=torch.tensor([1, 2, 3], device="cuda"), cam_id=4)
    assert all(torch.equal(on_dev[k], shared[k]) for k in shared)
    empty = P.view_fields(dev(case["c2w"]), dev(case["K"]), 0, 5, img_idx=0, frame_idx=0)
    assert tuple(empty["viewdirs"].shape) == (3, 0, 5, 3) and same_bits(host(empty["intrinsics"][2]), R.scaled_intrinsics(case["K"][2], 1.0))


# ---- the resizes --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resize_ref(H, W, factor, kind):
    img = R.image_case(kind, H, W)
    t = torch.from_numpy(img).permute(2, 0, 1)[None]
    ref32 = torch.nn.functional.interpolate(t, scale_factor=factor, mode="bicubic", antialias=True)[0].permute(1, 2, 0).numpy()
    ref64 = torch.nn.functional.interpolate(t.double(), scale_factor=factor, mode="bicubic", antialias=True)[0].permute(1, 2, 0).numpy()
    return img, ref32, ref64


@pytest.mark.parametrize("kind", ["noise", "step", "constant"])
@pytest.mark.parametrize("case", RESIZE_CASES)
def test_resize_image_matches_torch(P, case, kind):
    H, W, factor = case
    img, ref32, ref64 = resize_ref(H, W, factor, kind)
    with poisoned_allocations(True, name=f"resize_image {H}x{W} x{factor:.3f} {kind}"):
        out = P.resize_image(dev(img), factor)
        assert not bool(holds_poison(out).any())
    got = host(out)
    bound, err = R.bound(ref32, ref64), distance(got, ref64)
    print(f"\nresize_image {H}x{W} x{factor:.4f} {kind}: {err:.2e} from torch's float64 (torch's float32 {distance(ref32, ref64):.2e}, bound {bound:.2e}); "
          f"{distance(got, ref32.astype(np.float64)):.2e} from torch's float32")
    assert got.dtype == np.float32 and got.shape == ref64.shape == R.output_size(H, W, factor) + (3,) and out.is_contiguous()
    assert err <= bound
    if kind == "constant":
        assert distance(got, np.full(got.shape, 0.7)) <= bound
    assert torch.equal(P.resize_image(dev(img), factor).view(torch.int32), out.view(torch.int32))      # determinism


def test_resize_image_at_factor_one_is_the_identity(P):
    img = R.image_case("noise", 13, 21)
    with poisoned_allocations(True, name="resize_image x1"):
        out = P.resize_image(dev(img), 1.0)
    assert same_bits(host(out), img)
    with pytest.raises(NotImplementedError):
        P.resize_image(dev(img), 1.5)


@pytest.mark.parametrize("factor", MASK_FACTORS)
@pytest.mark.parametrize("n", [1, 5])
def test_resize_masks_equal_torch(P, n, factor):
    H, W = 37, 41
    masks = R.mask_case(n, H, W, seed=n)
    with poisoned_allocations(True, name=f"resize_masks {n} x{factor:.3f}"):
        outs = P.resize_masks([dev(m) for m in masks], factor)
        assert not any(bool(holds_poison(o).any()) for o in outs)
    assert len(outs) == n
    for m, o in zip(masks, outs):
        ref = torch.nn.functional.interpolate(torch.from_numpy(m)[None, None], scale_factor=factor, mode="nearest")[0, 0].numpy()
        assert same_bits(host(o), ref)
    again = P.resize_masks([dev(m) for m in masks], factor)
    assert all(torch.equal(a, o) for a, o in zip(again, outs))
