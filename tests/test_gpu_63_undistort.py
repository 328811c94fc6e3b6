"""The lens undistortion on the MI355X (csrc/undistort.hip through bilateral_driving_amd/undistort.py) against the numpy restatement
(tests/undistort_ref64.py; tests/test_undistort_cpu.py holds the restatement to known answers and shows that no 32 u or 32 v of the
fixed cases comes within 2e-5 of a rounding tie, so an ulp of host / device difference cannot flip a pixel): EQUAL, for uint8 and both
float forms, C = 3 and C = 1, three coefficient sets in one launch; bit-identical run to run; every output byte written and nothing
outside (tests.poison); strided sources; the lidar projection with an ``undistort`` camera; the loaders on files."""
import numpy as np
import pytest
import torch

from tests import lidar_ref64 as LR
from tests import undistort_ref64 as R
from tests.poison import holds_poison, poisoned_allocations

pytestmark = pytest.mark.gpu

KINDS = ("uint8", "unit", "mask")


@pytest.fixture(scope="module")
def UD():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import undistort
    return undistort


@pytest.fixture(scope="module")
def frames():
    return {c: R.frames_case(c) for c in (1, 3)}


@pytest.fixture(scope="module")
def reference(frames):
    """{(case, channels, kind): the restatement's result}: computed once, never changed"""
    out = {}
    for name in R.CASES:
        K, dist, new_K = R.case(name)
        for c in (1, 3):
            for kind in KINDS:
                out[name, c, kind] = R.undistort(frames[c], K, dist, new_K, kind)
                out[name, c, kind].setflags(write=False)
    return out


def bits(t):
    t = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(t).view(np.uint8)


@pytest.mark.parametrize("channels", (3, 1))
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_the_restatement(UD, frames, reference, name, channels):
    K, dist, new_K = R.case(name)
    src = frames[channels]
    for kind in KINDS:
        with poisoned_allocations(True, name=f"undistort {name} C={channels} {kind}") as pz:
            got = UD.undistort_images(src, K, dist, new_K, out=kind)      # a host array: uploaded
            again = UD.undistort_images(torch.from_numpy(src).cuda(), torch.from_numpy(K), torch.from_numpy(dist), new_K, out=kind)
            if kind != "uint8":      # (the byte poison 0x7F is also a value: the next test covers the uint8 form)
                assert not bool(holds_poison(got).any()) and not bool(holds_poison(again).any())      # every element written
        assert got.is_cuda and tuple(got.shape) == src.shape and got.dtype == (torch.uint8 if kind == "uint8" else torch.float32)
        want = reference[name, channels, kind]
        assert np.array_equal(bits(got), bits(want)), (name, channels, kind, int((got.cpu().numpy() != want).sum()))
        assert np.array_equal(bits(again), bits(got))      # two runs, one from a device tensor: the same bits
    assert len(pz.records) >= 2


def test_every_output_byte_is_written_over_byte_poison(UD, frames):
    """uint8 poison is the byte 0x7F, which is also a legitimate value: the output is written over two different fills instead."""
    K, dist, new_K = R.case("pin+shift")
    src = torch.from_numpy(frames[3]).cuda()
    want = R.undistort(frames[3], K, dist, new_K)
    outs = []
    for int_bodies in (True, False):      # bodies of 0x7F, then of zeros
        with poisoned_allocations(int_bodies, name="undistort byte fill"):
            outs.append(UD.undistort_images(src, K, dist, new_K).cpu().numpy())
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)


@pytest.mark.parametrize("channels", (3, 1))
def test_three_frames_carry_three_coefficient_sets_in_one_launch(UD, frames, reference, channels):
    names = ("barrel", "pincushion", "pin+shift")
    Ks = np.stack([R.case(n)[0] for n in names])
    dists = np.stack([R.case(n)[1] for n in names])
    new_Ks = np.stack([R.K if R.case(n)[2] is None else R.case(n)[2] for n in names])
    for kind in KINDS:
        with poisoned_allocations(True, name=f"undistort three sets {kind}"):
            got = UD.undistort_images(torch.from_numpy(frames[channels]).cuda(), Ks, dists, new_Ks, out=kind)
        got = got.cpu().numpy()
        for f, n in enumerate(names):
            assert np.array_equal(bits(got[f]), bits(reference[n, channels, kind][f])), (n, kind)
    assert len({got[f].tobytes() for f in range(3)}) == 3


def test_projective_new_matrix_takes_the_division(UD, frames):
    """The kernel skips the division by _w for an affine new matrix (a wave-uniform branch); with a perspective row it divides."""
    K, dist, _ = R.case("barrel")
    new_K = K.copy()
    new_K[2] = [1e-3, -2e-3, 1.0]
    u, v = R.source_map(R.H, R.W, K, dist, new_K)
    assert R.classify(u, v, R.H, R.W)["tie_margin"] >= 1e-6
    for c in (1, 3):
        with poisoned_allocations(True, name="undistort projective"):
            got = UD.undistort_images(frames[c], K, dist, new_K, out="unit")
        assert np.array_equal(bits(got), bits(R.undistort(frames[c], K, dist, new_K, "unit")))


def test_single_frames_and_shapes(UD, frames, reference):
    K, dist, new_K = R.case("pincushion")
    one = UD.undistort_images(frames[3][1], K, dist, out="unit")      # [H,W,3]
    assert tuple(one.shape) == (R.H, R.W, 3) and np.array_equal(bits(one), bits(reference["pincushion", 3, "unit"][1]))
    one = UD.undistort_images(torch.from_numpy(frames[1][2]), K, dist, out="mask")      # [H,W]
    assert tuple(one.shape) == (R.H, R.W) and np.array_equal(bits(one), bits(reference["pincushion", 1, "mask"][2]))
    stack = UD.undistort_images(frames[1][:2], K, dist)      # [F,H,W]
    assert tuple(stack.shape) == (2, R.H, R.W) and np.array_equal(stack.cpu().numpy(), reference["pincushion", 1, "uint8"][:2])


def test_a_host_stack_is_staged_in_pieces(UD, frames, reference, monkeypatch):
    K, dist, new_K = R.case("barrel")
    per_frame = R.H * R.W * 3
    calls = []
    lib = UD.L.lib()

    class Counting:
        def __getattr__(self, name):
            return getattr(lib, name)

        def bds_undistort(self, *a):
            calls.append(a[0])      # the frames of this launch
            return lib.bds_undistort(*a)
    proxy = Counting()
    monkeypatch.setattr(UD, "STAGE_BYTES", 2 * per_frame + 5)      # two frames per piece: pieces of 2 and 1
    monkeypatch.setattr(UD.L, "lib", lambda: proxy)
    got = UD.undistort_images(frames[3], K, dist, out="unit")
    assert calls == [2, 1]
    calls.clear()
    on_device = UD.undistort_images(torch.from_numpy(frames[3]).cuda(), K, dist, out="unit")      # already there: one launch
    assert calls == [3]
    monkeypatch.undo()
    assert np.array_equal(bits(got), bits(reference["barrel", 3, "unit"])) and np.array_equal(bits(on_device), bits(got))


def test_a_strided_source_is_made_contiguous_not_misread(UD, frames, reference):
    K, dist, new_K = R.case("pincushion")
    for c in (1, 3):
        src = torch.from_numpy(frames[c]).cuda()
        wide = torch.zeros((R.F, R.H, 2 * R.W) + ((3,) if c == 3 else ()), dtype=torch.uint8, device="cuda")
        wide[:, :, ::2] = src
        view = wide[:, :, ::2]      # every second column
        assert not view.is_contiguous()
        got = UD.undistort_images(view, K, dist)
        assert np.array_equal(got.cpu().numpy(), reference["pincushion", c, "uint8"])
    planes = torch.from_numpy(frames[3]).cuda().permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)      # channel-first storage
    assert not planes.is_contiguous()
    assert np.array_equal(UD.undistort_images(planes, K, dist).cpu().numpy(), reference["pincushion", 3, "uint8"])
    host_view = frames[3][::-1]      # a host array with a negative stride, frames reversed
    got = UD.undistort_images(host_view, K, dist)
    assert np.array_equal(got.cpu().numpy(), reference["pincushion", 3, "uint8"][::-1])


# ---- the lidar projection ---------------------------------------------------------------------------------------------------------------
def undistort_dataset(device, flag=True):
    pc = LR.golden_projection_case("shared")
    d = LR.bare_projection_dataset(pc, device)
    for c, cam in d.pixel_source.camera_data.items():
        cam.distortions = torch.tensor([[-0.05 + 0.01 * f, 0.01, 0.001, -0.0005 * (c + 1), 0.0] for f in range(len(cam))])
    d.pixel_source.camera_data[1].undistort = flag
    return pc, d


def restated_matrices(cam):
    out = []
    for f in range(len(cam)):
        K = cam.intrinsics[f].cpu().numpy().astype(np.float64)
        M = R.optimal_new_camera_matrix(K, cam.distortions[f].cpu().numpy().astype(np.float64), (cam.WIDTH, cam.HEIGHT), 1.0)
        K4 = torch.nn.functional.pad(torch.from_numpy(M).float(), (0, 1, 0, 1))
        K4[3, 3] = 1.0
        out.append(K4 @ cam.cam_to_worlds[f].cpu().float().inverse())
    return torch.stack(out)


def snapshot(d):
    ls = d.lidar_source
    return ([cam.lidar_depth_maps.clone() for cam in d.pixel_source.camera_data.values()], ls.colors.clone(), ls.deleted,
            ls.origins.clone(), ls.timesteps.clone())


def test_projection_without_an_undistort_camera_is_lidars_bit_for_bit(UD):
    from bilateral_driving_amd import lidar
    _, a = undistort_dataset("cuda", flag=False)
    _, b = undistort_dataset("cuda", flag=False)
    lidar.project_lidar_pts_on_images(a)
    with poisoned_allocations(True, name="undistort projection, no undistort camera"):
        UD.project_lidar_pts_on_images(b)
    sa, sb = snapshot(a), snapshot(b)
    for x, y in zip(sa[0], sb[0]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(sa[1].view(torch.int32), sb[1].view(torch.int32)) and sa[2] == sb[2] and torch.equal(sa[3], sb[3]) and torch.equal(sa[4], sb[4])


def test_projection_with_an_undistort_camera_uses_the_optimal_matrix(UD):
    from bilateral_driving_amd import lidar
    pc, d = undistort_dataset("cuda")
    with pytest.raises(NotImplementedError):
        lidar.project_lidar_pts_on_images(d)
    ls, ps = d.lidar_source, d.pixel_source
    # the expected result: lidar.project_points per camera, matrices from the restatement's new K for camera 1
    dev = torch.device("cuda")
    uniq = ls.unique_normalized_timestamps
    perm, offsets = lidar.group_by_timestep(ls.timesteps, uniq.shape[0])
    x = (ls.origins + ls.directions * ls.ranges).float()[perm].contiguous()
    visible = torch.zeros(len(x), dtype=torch.uint8, device=dev)
    colors = ls.colors.float()[perm].contiguous()
    want_depth, all_ranges = [], {}
    for c, cam in ps.camera_data.items():
        F = len(cam)
        closest = torch.argmin(torch.abs(uniq[None, :] - ps.normalized_time[:F][:, None]), dim=1)
        ranges = torch.stack([offsets[closest], offsets[closest + 1]], dim=1)
        all_ranges[c] = ranges
        mats = restated_matrices(cam) if c == 1 else lidar.camera_matrices(cam)
        want_depth.append(lidar.project_points(x, mats, ranges, cam.WIDTH, cam.HEIGHT, cam.images[:F], visible, colors)[0])
    want_colors = torch.empty_like(colors)
    want_colors[perm] = colors
    want_visible = torch.empty_like(visible)
    want_visible[perm] = visible
    with poisoned_allocations(True, name="undistort projection"):
        UD.project_lidar_pts_on_images(d, delete_out_of_view_points=False)
    # the product's optimal matrix equals the restatement's to 1e-12, far below a float32 ulp: the float32 matrices are the same bits
    assert torch.equal(UD.camera_matrices(ps.camera_data[1]), restated_matrices(ps.camera_data[1]))
    for cam, want in zip(ps.camera_data.values(), want_depth):
        assert torch.equal(cam.lidar_depth_maps.view(torch.int32), want.view(torch.int32))
    assert torch.equal(ls.visible_masks, want_visible.bool()) and torch.equal(ls.colors.view(torch.int32), want_colors.view(torch.int32))
    # and the new matrix matters: camera 1's maps differ from the raw intrinsics' maps
    raw = lidar.project_points(x, lidar.camera_matrices(ps.camera_data[1]), all_ranges[1], ps.camera_data[1].WIDTH, ps.camera_data[1].HEIGHT)[0]
    assert not torch.equal(raw, ps.camera_data[1].lidar_depth_maps) and int((ps.camera_data[1].lidar_depth_maps > 0).sum()) > 100


# ---- the loaders --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", (True, False))
def test_loaders_set_the_references_attributes(UD, tmp_path, monkeypatch, capsys, flag):
    from PIL import Image
    paths = R.write_camera_files(tmp_path)
    monkeypatch.chdir(tmp_path)
    ego_dir = tmp_path / "data" / "ego_masks" / "tiny"
    ego_dir.mkdir(parents=True)
    g = np.random.default_rng(9)
    Image.fromarray(((g.random((20, 26)) < 0.5) * 255).astype(np.uint8)).save(str(ego_dir / "0.png"))

    class CameraData(R.BareLoaderCamera):
        pass
    UD.install(CameraData)
    try:
        cam = CameraData(paths, torch.device("cuda"), flag)
        cam.dataset_name = "tiny"
        with poisoned_allocations(True, name=f"undistort loaders undistort={flag}"):
            cam.load_images()
            cam.load_egocar_mask()
            cam.load_dynamic_masks()
            cam.load_sky_masks()
    finally:
        UD.uninstall()
    assert "load_images" not in CameraData.__dict__
    said = capsys.readouterr().out
    for what in ("rgb", "dynamic mask", "human mask", "vehicle mask", "sky mask"):
        assert (f"undistorting {what}" in said) == flag
    h, w = cam.load_size
    F = len(paths["img"])

    def read(fname, mode, filt):
        return np.array(Image.open(fname).convert(mode).resize((w, h), filt))
    K, dist = cam.intrinsics.numpy().astype(np.float64), cam.distortions.numpy().astype(np.float64)

    def expect(stack, kind, Ks=K, ds=dist):
        stack = np.stack(stack)
        if flag:
            return R.undistort(stack, Ks, ds, None, kind)
        return stack.astype(np.float32) / np.float32(255) if kind == "unit" else (stack > 0).astype(np.float32)
    want = {"images": expect([read(p, "RGB", Image.BILINEAR) for p in paths["img"]], "unit"),
            "dynamic_masks": expect([read(p, "L", Image.BILINEAR) for p in paths["dynamic_mask"]], "mask"),
            "human_masks": expect([read(p, "L", Image.BILINEAR) for p in paths["human_mask"]], "mask"),
            "vehicle_masks": expect([read(p, "L", Image.BILINEAR) for p in paths["vehicle_mask"]], "mask"),
            "sky_masks": expect([read(p, "L", Image.NEAREST) for p in paths["sky_mask"]], "mask"),
            "egocar_mask": expect([read(str(ego_dir / "0.png"), "L", Image.BILINEAR)], "mask", K[:1], dist[:1])[0]}      # frame 0's intrinsics
    for name, ref in want.items():
        got = getattr(cam, name)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape, name
        assert np.array_equal(bits(got), bits(ref)), name
    assert tuple(cam.images.shape) == (F, h, w, 3) and tuple(cam.egocar_mask.shape) == (h, w) and tuple(cam.sky_masks.shape) == (F, h, w)
