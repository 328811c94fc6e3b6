"""The evaluation video frames on the MI355X (csrc/video.hip through bilateral_driving_amd/video.py) against the numpy restatement
(tests/video_ref64.py) and the reference's recorded results (tests/golden/video_frames.npz), both pinned to the reference by
tests/test_video_cpu.py.  No test reads the reference tree.

Bounds.  RGB, GRAY, OVER_GREEN, the pixel branch of LIDAR_ON_IMAGE and the layouts are bit-equal to the golden and the restatement.
A depth colour stands under the rule of tests/video_ref64.py: it may differ from the float64 restatement by exactly one table index,
only where the float64 value 256 s lies within 2^-10 of an integer, on at most 0.1 % of a case's pixels; every other pixel is bit-equal.
The shapes: one panel of 1 x 1, 5 x 7 and 17 x 23 (3 Wc = 69 bytes per row: rows start at every byte phase, and 391 pixels leave a
three-pixel tail), from 16-byte aligned bases, from bases one element off and from non-contiguous views; every recorded layout at 4 x 6;
panels that overlap, in both orders; 70 panels (two bands); one 135 x 240, 3-camera, 3-key merged frame.

Figures measured on the MI355X (this file's own prints): the kernel's depth colours differ from the float64 restatement on 0 pixels of
every one-panel case (1, 35 and 391 pixels; float, bool and absent weight; the lidar map), on 0 of 192 692 depth pixels of the
135 x 240 merged frame, and on 0 pixels of the reference's recorded waymo and nuscenes frames."""
import functools

import numpy as np
import pytest
import torch

from tests import video_ref64 as R
from tests.poison import poisoned_allocations

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (5, 7), (17, 23))


@pytest.fixture(scope="module")
def V():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import video
    return video


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().contiguous().numpy()


def offset_view(a, off):
    """``a`` on the device at a base ``off`` elements behind a fresh allocation's."""
    d = dev(a)
    flat = torch.zeros(d.numel() + off, dtype=d.dtype, device="cuda")
    flat[off:] = d.reshape(-1)
    return flat[off:].view(d.shape)


def strided_view(a):
    """``a`` on the device as a non-contiguous view: every second column of a wider tensor."""
    d = dev(a)
    wide = torch.zeros(d.shape[:1] + (2 * d.shape[1],) + d.shape[2:], dtype=d.dtype, device="cuda")
    wide[:, ::2] = d
    v = wide[:, ::2]
    assert not v.is_contiguous() or d.shape[1] == 1
    return v


PLACE = {"aligned": dev, "offset": lambda a: offset_view(a, 1), "strided": strided_view}


@functools.lru_cache(maxsize=None)
def case(h, w):
    """One size's sources and the restatement of every kind, computed once and left unchanged."""
    rgb, op, lidar = R.rgb_case(h, w)
    depth, opacity, weight = R.depth_case(h, w)
    shown = lidar > 0
    want = {"rgb": R.to8b(rgb), "gray": R.to8b(np.stack([op] * 3, -1)), "gray_bool": R.to8b(np.stack([weight] * 3, -1)),
            "gray_u8": R.to8b(np.stack([(255 * op).astype(np.uint8)] * 3, -1)),
            "green": R.to8b(R.over_green(rgb, op, np.float32)), "lidar": R.lidar_on_image(rgb, lidar)}
    out = dict(rgb=rgb, op=op, lidar=lidar, depth=depth, opacity=opacity, weight=weight, shown=shown, want=want)
    for a in list(out.values())[:-1] + list(want.values()):
        a.setflags(write=False)
    return out


# ---- 1. one panel of every kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", sorted(PLACE))
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_one_panel_of_every_kind(V, size, place):
    h, w = size
    c, put, g = case(h, w), PLACE[place], R.golden()
    label = f"{h}x{w} {place}"
    got = V.to8b(put(c["rgb"]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3) and got.is_cuda
    assert np.array_equal(host(got), c["want"]["rgb"]), label
    assert np.array_equal(host(V.to8b(put(c["op"]))), c["want"]["gray"][..., 0]), label                   # [h,w] in, [h,w] out
    assert np.array_equal(host(V.to8b(put(c["op"][..., None]))), c["want"]["gray"][..., :1]), label
    assert np.array_equal(host(V._one(V.GRAY, put(c["weight"]))), c["want"]["gray_bool"]), label          # bool: 0 or 255
    assert np.array_equal(host(V._one(V.GRAY, put((255 * c["op"]).astype(np.uint8)))), c["want"]["gray_u8"]), label
    assert np.array_equal(host(V.over_green(put(c["rgb"]), put(c["op"]))), c["want"]["green"]), label
    assert np.array_equal(host(V.over_green(put(c["rgb"]), put(c["op"][..., None]))), c["want"]["green"]), label
    lidar = host(V.lidar_on_image(put(c["rgb"]), put(c["lidar"])))
    assert np.array_equal(lidar[~c["shown"]], c["want"]["lidar"][~c["shown"]]), label                     # the pixel branch: bit-equal
    counts = {"lidar": R.depth_rule(lidar, c["lidar"], c["shown"], c["shown"])}
    for tag, wgt in (("opacity", c["opacity"]), ("bool", c["weight"]), ("none", None)):
        got = host(V.depth_visualizer(put(c["depth"]), None if wgt is None else put(wgt)))
        counts[tag] = R.depth_rule(got, c["depth"], wgt)
        if (h, w) == (17, 23) and tag != "none":
            assert R.depth_rule(g["depth_rgb" if tag == "opacity" else "depth_rgb_bool"], c["depth"], wgt) == 0      # the reference's record
    print(f"\ndepth colours {label}: pixels differing from the float64 restatement {counts} of {h * w}")
    if (h, w) == (17, 23):
        assert np.array_equal(c["want"]["green"], g["green_rgb"]) and np.array_equal(lidar[~c["shown"]], g["lidar_rgb"][~c["shown"]])


# ---- 2. the layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,dataset_type,names,sizes", R.layout_cases(), ids=[c[0] for c in R.layout_cases()])
def test_layouts_equal_the_references_canvases(V, label, dataset_type, names, sizes):
    imgs = [dev(i) for i in R.constant_images(sizes)]
    want = R.golden()[f"layout_{label}"]
    with poisoned_allocations(True, name=f"layout_{label}") as pz:
        got = V.FrameComposer(dataset_type, ["rgbs"]).key_frame("rgbs", {"rgbs": imgs}, names)
        assert len(pz.records) == 1
        pz.check_guards()
        canvas = host(got)
    assert np.array_equal(canvas, want), label      # (with it: no poison left, unfilled pixels 0)
    assert np.array_equal(canvas, R.to8b(R.layout(dataset_type, R.constant_images(sizes), names)))


def test_overlapping_panels_the_later_one_wins_and_unfilled_pixels_are_zero(V):
    h, w = 5, 7
    a, b = np.full((h, w, 3), 0.25, np.float32), np.full((h, w), 0.75, np.float32)
    Hc, Wc = 9, 11      # 33 bytes per row
    for order in ((0, 1), (1, 0)):
        specs = [(V.RGB, a, (1, 1)), (V.GRAY, b, (3, 4))]
        panels = [V._panel(specs[k][0], dev(specs[k][1]), None, "cuda", V.Rect(0, specs[k][2][0], specs[k][2][1], h, w, 0)) for k in order]
        with poisoned_allocations(True, name="overlap") as pz:
            canvas = V._launch(panels, Hc, Wc, torch.device("cuda"))
            pz.check_guards()
            got = host(canvas)
        want = np.zeros((Hc, Wc, 3), np.uint8)
        for k in order:
            y, x = specs[k][2]
            want[y:y + h, x:x + w] = 63 if k == 0 else 191
        assert np.array_equal(got, want), order
        assert (got[0] == 0).all() and (got[:, 0] == 0).all() and got[3, 4, 0] == (191 if order[-1] == 1 else 63)
    with poisoned_allocations(True, name="no panel") as pz:      # no panel at all: a zeroed canvas, every byte written
        got = host(V._launch([], 3, 5, torch.device("cuda")))
        pz.check_guards()
    assert got.shape == (3, 5, 3) and (got == 0).all()
    assert tuple(V._launch([], 0, 5, torch.device("cuda")).shape) == (0, 5, 3)


def test_seventy_panels_take_two_bands_and_a_source_row_offset(V):
    rng = np.random.default_rng(70)
    h, w, Wc, n = 3, 5, 7, 70      # 21 bytes per row: the bands' edges fall on every byte phase
    imgs = [rng.uniform(-0.1, 1.1, (h + 2, w, 3)).astype(np.float32) for _ in range(n)]
    panels = [V._panel(V.RGB, dev(im), None, "cuda", V.Rect(0, 2 * k, k % 3, h, w, 1 + k % 2)) for k, im in enumerate(imgs)]
    Hc = 2 * (n - 1) + h + 1
    want = np.zeros((Hc, Wc, 3), np.uint8)
    for k, im in enumerate(imgs):      # each overlaps the one before by a row: the later one wins
        want[2 * k:2 * k + h, k % 3:k % 3 + w] = R.to8b(im[1 + k % 2:1 + k % 2 + h])
    with poisoned_allocations(True, name="bands") as pz:
        got = host(V._launch(panels, Hc, Wc, torch.device("cuda")))
        pz.check_guards()
    assert np.array_equal(got, want)
    from bilateral_driving_amd import _lib as L
    with pytest.raises(L.BdsError):      # 65 panels on one row: BDS_ECAPACITY
        V._launch([panels[0]._replace(rect=V.Rect(0, 0, 0, h, w, 0))] * 65, Hc, Wc, torch.device("cuda"))


# ---- 3. merged frames --------------------------------------------------------------------------------------------------------------------
def on_device(rr, unsqueeze=False):
    """``render_results`` with every array on the device, as the trainer holds them ([h,w,1] maps with ``unsqueeze``)."""
    return {k: (list(v) if k == "cam_names" else [dev(a)[..., None] if (unsqueeze and a.ndim == 2) else dev(a) for a in v]) for k, v in rr.items()}


@pytest.mark.parametrize("dataset_type", sorted(R.MERGED))
def test_save_functions_write_the_references_frames(V, dataset_type):
    g = R.golden()
    names = R.MERGED[dataset_type]
    rr = R.render_results(dataset_type, names)
    num_cams, T = len(names), R.MERGED_T
    want = [R.merged_frame(dataset_type, rr, R.MERGED_KEYS, i, num_cams) for i in range(T)]
    runs = []
    for results in (on_device(rr, unsqueeze=True), rr):      # device tensors; the numpy lists of the unmodified render: uploaded
        log = []
        got = V.save_concatenated_videos(results, "video.mp4", f"layout_{dataset_type}", T, keys=list(R.MERGED_KEYS), num_cams=num_cams,
                                         verbose=False, writer_factory=R.writer_factory(log))
        assert len(log) == 1 and log[0].closed and log[0].path == "video.mp4" and len(log[0].frames) == T and list(got) == ["concatenated_frame"]
        differing = sum(R.frame_rule(log[0].frames[i], want[i]) for i in range(T))
        recorded = sum(int(np.any(log[0].frames[i] != g[f"concat_{dataset_type}"][i], axis=-1).sum()) for i in range(T))
        assert np.array_equal(got["concatenated_frame"], log[0].frames[T // 2]) and got["concatenated_frame"].dtype == np.uint8
        runs.append(np.stack(log[0].frames))
        print(f"\nconcatenated {dataset_type}: {differing} depth pixels differ from the float64 restatement, {recorded} from the reference's frames")
        assert recorded <= differing      # (the reference's record stands 0 pixels from the restatement: tests/test_video_cpu.py)
    assert np.array_equal(runs[0], runs[1])
    log = []
    got = V.save_seperate_videos(on_device(rr), "video.mp4", f"layout_{dataset_type}", T, keys=list(R.MERGED_KEYS), num_cams=num_cams,
                                 writer_factory=R.writer_factory(log))
    assert [w.path for w in log] == list(g[f"separate_{dataset_type}_paths"])
    assert [len(w.frames) for w in log] == list(g[f"separate_{dataset_type}_written"]) and list(got) == list(g[f"separate_{dataset_type}_returned"])
    for wr, key in zip(log, R.MERGED_KEYS):
        for i, frame in enumerate(wr.frames):
            n = R.frame_rule(frame, R.key_canvas(dataset_type, rr, key, i, num_cams))
            assert int(np.any(frame != g[f"separate_{dataset_type}_{key}"][i], axis=-1).sum()) <= n
        if wr.frames:
            assert np.array_equal(got[key], wr.frames[T // 2])
            assert g[f"separate_{dataset_type}_returned_{key}"].shape == got[key].shape


def test_save_images_writes_the_views_and_the_raw_depths(V, tmp_path):
    names = R.MERGED["waymo"]
    rr = R.render_results("waymo", names, T=1)
    images, log = [], []
    path = str(tmp_path / "video.mp4")
    V.save_seperate_videos(on_device(rr, unsqueeze=True), path, "waymo", 1, keys=["rgbs", "depths"], num_cams=3, save_images=True,
                           writer_factory=R.writer_factory(log), image_writer=lambda p, im: images.append((p, im)))
    assert [p for p, _ in images] == [str(tmp_path / f"video_{k}/000_{j:03d}.png") for k in ("rgbs", "depths") for j in range(3)]
    assert all(np.array_equal(im, R.to8b(rr["rgbs"][j])) for j, (_, im) in enumerate(images[:3]))
    for j, (_, im) in enumerate(images[3:]):
        R.depth_rule(im, rr["depths"][j], rr["opacities"][j])
        assert np.array_equal(np.load(tmp_path / "video_depths_np" / f"000_{j:03d}.npy"), rr["depths"][j])      # [h,w] from the [h,w,1] map


@functools.lru_cache(maxsize=None)
def big_case():
    names, keys = R.MERGED["waymo"], ["rgbs", "depths", "Dynamic_depths"]
    rr = R.render_results("waymo", R.CAMS["waymo"][1:4], T=1, h=135, w=240, seed=54)
    return names, keys, rr, R.merged_frame("waymo", rr, keys, 0, 3)


def test_merged_frame_135_by_240_and_two_runs_give_the_same_bits(V):
    names, keys, rr, want = big_case()
    results = on_device(rr)
    composer = V.FrameComposer("waymo", keys)
    with poisoned_allocations(True, name="merged") as pz:
        a = composer.frame(results, names)
        assert len(pz.records) == 1      # the canvas: nothing else is allocated, nothing uploaded
        pz.check_guards()
        first = host(a)
    assert first.shape == (3 * 134, 3 * 240 - 1, 3) == want[0].shape
    n = R.frame_rule(first, want)
    print(f"\nmerged 135 x 240, 3 cameras, 3 keys: {n} of {int(want[1].sum())} depth pixels differ from the float64 restatement")
    for c in range(3):      # the band itself, per map
        R.depth_rule(host(V.depth_visualizer(results["depths"][c], results["opacities"][c])), rr["depths"][c], rr["opacities"][c])
    second = host(composer.frame(results, names))
    assert np.array_equal(first, second)
    small = on_device(R.render_results("nuscenes", R.MERGED["nuscenes"], T=1))
    c2 = V.FrameComposer("nuscenes", R.MERGED_KEYS)
    assert np.array_equal(host(c2.frame(small, R.MERGED["nuscenes"])), host(c2.frame(small, R.MERGED["nuscenes"])))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise(V):
    from bilateral_driving_amd import _lib as L
    rgb, gray = torch.rand(5, 7, 3), torch.rand(5, 7)
    for fn in (lambda: V.to8b(rgb), lambda: V.depth_visualizer(gray.cuda(), gray), lambda: V.over_green(rgb.cuda(), gray),
               lambda: V.FrameComposer("kitti", ["rgbs"]).frame({"rgbs": [rgb, rgb.cuda()]}, ["CAM_LEFT", "CAM_RIGHT"])):
        with pytest.raises(L.BdsError):
            fn()
    with pytest.raises(ValueError):
        V.FrameComposer("kitti", ["rgbs"]).frame({"rgbs": [rgb.cuda(), rgb.cuda()[:, :6]]}, ["CAM_LEFT", "CAM_RIGHT"])
