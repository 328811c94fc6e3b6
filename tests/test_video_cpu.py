"""The evaluation video frames (bilateral_driving_amd/video.py, csrc/video.hip) on the CPU: the numpy restatement
(tests/video_ref64.py) against the reference's recorded results (tests/golden/video_frames.npz, scripts/gen_golden_video.py),
``plan_layout``'s rectangles against the recorded canvases, the colour table against matplotlib, the pixel formulas on the host
(tests/hostmath_video_shim.hip) against the restatement, the C entry's signature and argument checks, the kernel's resources, the seam
and the key rules of ``FrameComposer`` with a fake launch.

Bounds.  Layouts, quantiser, over-green and the pixel branch of lidar-on-image are bit-equal.  A depth colour stands under the rule of
tests/video_ref64.py (one table index, only within 2^-10 of an integer 256 s, at most 0.1 % of a case's pixels); the host shim's
``vf_depth_index`` is held to the same rule against the float64 mode and, where the host's logf and numpy's agree, is bit-equal to the
float32 mode."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from bilateral_driving_amd import video as V
from tests import video_ref64 as R
from tests.util import build_shim, declared_signatures, kernel_resources, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def paint(plan, imgs_u8):
    """The canvas that ``plan``'s rectangles give, painted on the host in their order."""
    canvas = np.zeros((plan.height, plan.width, 3), np.uint8)
    for r in plan.rects:
        canvas[r.y:r.y + r.h, r.x:r.x + r.w] = imgs_u8[r.index][r.row0:r.row0 + r.h, :r.w]
    return canvas


# ---- 1. the restatement and plan_layout against the golden ---------------------------------------------------------------------------
@pytest.mark.parametrize("label,dataset_type,names,sizes", R.layout_cases(), ids=[c[0] for c in R.layout_cases()])
def test_layouts_equal_the_references_canvases(label, dataset_type, names, sizes):
    want = R.golden()[f"layout_{label}"]
    imgs = R.constant_images(sizes)
    assert np.array_equal(R.to8b(R.layout(dataset_type, imgs, names)), want)
    plan = V.plan_layout(dataset_type, names, sizes)
    assert (plan.height, plan.width, 3) == want.shape
    assert np.array_equal(paint(plan, [R.to8b(i) for i in imgs]), want)
    assert all(0 <= r.y and r.y + r.h <= plan.height and 0 <= r.x and r.x + r.w <= plan.width and r.row0 == 0 for r in plan.rects)
    assert V.plan_layout(dataset_type, tuple(names), [list(s) for s in sizes]) is plan      # cached per (type, names, sizes)


def test_layout_quirks_and_errors():
    g = R.golden()
    assert g["layout_nuplan_one"].shape == (R.H, R.W, 3) and g["layout_nuscenes_one"].shape == (R.H - 1, R.W - 1, 3)      # min:max+1 / min:max
    short = V.plan_layout("waymo", R.CAMS["waymo"], [R.size_of("waymo", n, True) for n in R.CAMS["waymo"]])
    assert short.rects[0].y == R.H - R.WAYMO_SIDE_H and short.rects[2].y == 0                                               # bottom-aligned
    centre = V.plan_layout("argoverse", R.CAMS["argoverse"], [R.size_of("argoverse", n) for n in R.CAMS["argoverse"]]).rects[1]
    assert (centre.h, centre.w) == (R.H, R.H) and centre.x == R.W                                                            # cropped to landscape_height rows
    assert len(V.plan_layout("kitti", ["CAM_RIGHT", "CAM_LEFT", "CAM_UNKNOWN"], [(4, 6)] * 3).rects) == 2                    # an unknown name is ignored
    for dataset_type, names, sizes in R.ERRORS:
        with pytest.raises(ValueError):
            R.layout(dataset_type, R.constant_images(sizes), names)
        with pytest.raises(ValueError):
            V.plan_layout(dataset_type, names, sizes)
    with pytest.raises(ValueError):
        V.plan_layout("carla", ["a"], [(4, 6)])
    with pytest.raises(IndexError):
        V.plan_layout("nuscenes", ["CAM_FRONT", "CAM_BACK"], [(4, 6)])


def test_restatement_equals_the_references_colours():
    g = R.golden()
    depth, opacity, weight = R.depth_case()
    for a, b in ((depth, g["depth_in"]), (opacity, g["opacity_in"]), (weight, g["weight_in"])):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.isnan(depth).any() and (depth == 0).any() and (depth < 0).any() and (depth == 4).any() and (depth == 120).any() and (depth == 1e10).any()
    assert (opacity == 0).any() and (opacity == 1).any()
    for tag, w in (("depth_rgb", opacity), ("depth_rgb_bool", weight)):
        n = R.depth_rule(g[tag], depth, w)
        print(f"\n{tag}: the reference differs from the float64 restatement on {n} of {depth.size} pixels")
        assert n == int(g[tag + "_differing"])
    rgb, op, lidar = R.rgb_case(17, 23)
    assert np.array_equal(rgb, g["lidar_pixels_in"], equal_nan=True) and np.array_equal(lidar, g["lidar_depth_in"])
    shown = lidar > 0
    mine = R.lidar_on_image(rgb, lidar)
    assert 0 < shown.sum() < shown.size and np.array_equal(mine[~shown], g["lidar_rgb"][~shown])
    R.depth_rule(g["lidar_rgb"], lidar, shown, shown)
    assert np.array_equal(R.to8b(R.over_green(rgb, op, np.float32)), g["green_rgb"])
    ok = ~np.isnan(g["green_float"])
    assert np.array_equal(R.over_green(rgb, op, np.float32).view(np.int32)[ok], g["green_float"].view(np.int32)[ok])


@pytest.mark.parametrize("dataset_type", sorted(R.MERGED))
def test_restatement_equals_the_references_merged_frames(dataset_type):
    g = R.golden()
    names = R.MERGED[dataset_type]
    rr = R.render_results(dataset_type, names)
    frames = g[f"concat_{dataset_type}"]
    assert frames.shape[0] == R.MERGED_T and np.array_equal(g[f"concat_{dataset_type}_returned"], frames[R.MERGED_T // 2])
    for i in range(R.MERGED_T):
        R.frame_rule(frames[i], R.merged_frame(dataset_type, rr, R.MERGED_KEYS, i, len(names)))
    assert list(g[f"separate_{dataset_type}_paths"]) == [f"video_{k}.mp4" for k in R.MERGED_KEYS]
    assert list(g[f"separate_{dataset_type}_returned"]) == R.MERGED_KEYS[:-1]          # gt_sky_masks: the mask rule finds no list
    assert list(g[f"separate_{dataset_type}_written"]) == [R.MERGED_T] * 5 + [0]
    for key in R.MERGED_KEYS[:-1]:
        for i in range(R.MERGED_T):
            R.frame_rule(g[f"separate_{dataset_type}_{key}"][i], R.key_canvas(dataset_type, rr, key, i, len(names)))


def test_turbo_table_equals_matplotlibs():
    table = R.golden()["turbo8"]
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert table[0].tolist() == [48, 18, 59] and table[255].tolist() == [122, 4, 2]
    try:
        import matplotlib
    except ImportError:      # (the table is then held by the golden's record alone)
        return
    lut = matplotlib.colormaps["turbo"](np.arange(256))[:, :3]
    assert np.array_equal(table, R.to8b(lut)) and np.array_equal(table, (255 * np.clip(lut, 0, 1)).astype(np.uint8))


# ---- 2. the header on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("video")
    vp, n = ctypes.c_void_p, ctypes.c_int64
    for name, args in (("hm_vf_to8b", [n, vp, vp]), ("hm_vf_depth_index", [n, vp, vp, vp]), ("hm_vf_turbo", [n, vp, vp]),
                       ("hm_vf_over_green", [n, vp, vp, vp]), ("hm_vf_lidar_shows_depth", [n, vp, vp]), ("hm_vf_constants", [vp])):
        getattr(h, name).argtypes, getattr(h, name).restype = args, None
    return h


def shim_index(shim, depth, weight):
    depth, weight = np.ascontiguousarray(depth, np.float32), np.ascontiguousarray(weight, np.float32)
    out = np.zeros(depth.shape, np.int32)
    shim.hm_vf_depth_index(depth.size, depth.ctypes.data, weight.ctypes.data, out.ctypes.data)
    return out


def shim_turbo(shim, index):
    index = np.ascontiguousarray(index, np.int32)
    out = np.zeros(index.shape + (3,), np.uint8)
    shim.hm_vf_turbo(index.size, index.ctypes.data, out.ctypes.data)
    return out


def test_host_quantiser_and_composite_equal_the_restatement_bit_for_bit(shim):
    g = R.golden()
    one, zero = np.float32(1), np.float32(0)
    edge = np.float32([-1e30, -0.2, -1e-45, -0.0, 0.0, 1e-45, 1 / 255, np.nextafter(np.float32(1 / 255), zero), 0.5, 254.999 / 255,
                       np.nextafter(one, zero), 1.0, np.nextafter(one, np.float32(2)), 1.3, 1e30, np.inf, -np.inf, np.nan])
    x = np.concatenate([edge, np.arange(256, dtype=np.float32) / np.float32(255), np.random.default_rng(1).uniform(-0.1, 1.1, 4096).astype(np.float32)])
    out = np.zeros(x.shape, np.uint8)
    shim.hm_vf_to8b(x.size, x.ctypes.data, out.ctypes.data)
    assert np.array_equal(out, R.to8b(x))
    finite = ~np.isnan(x)
    assert np.array_equal(out[finite], (255 * np.clip(x[finite], 0, 1)).astype(np.uint8)) and out[~finite].tolist() == [0]      # the reference's to8b; a NaN: 0
    assert out[:len(edge)].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 127, 254, 254, 255, 255, 255, 255, 255, 0, 0]
    consts = np.zeros(5, np.float32)
    shim.hm_vf_constants(consts.ctypes.data)
    assert np.array_equal(consts, np.float32([min(R.LO, R.HI), abs(R.HI - R.LO), *R.GREEN]))      # formed in float64, rounded once
    rgb, op = g["green_rgb_in"], g["green_opacity_in"]
    got = np.zeros(rgb.shape, np.float32)
    shim.hm_vf_over_green(op.size, rgb.ctypes.data, op.ctypes.data, got.ctypes.data)
    want = R.over_green(rgb, op, np.float32)
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.int32)[ok], want.view(np.int32)[ok]) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.int32)[ok], g["green_float"].view(np.int32)[ok])      # the reference's own composite
    d = np.float32([-1.0, -0.0, 0.0, 1e-45, 3.0, np.inf, np.nan])
    shows = np.zeros(d.shape, np.uint8)
    shim.hm_vf_lidar_shows_depth(d.size, d.ctypes.data, shows.ctypes.data)
    assert shows.tolist() == [0, 0, 0, 1, 1, 1, 0]
    table = shim_turbo(shim, np.arange(-1, 256))
    assert np.array_equal(table[1:], g["turbo8"]) and table[0].tolist() == [0, 0, 0]      # kTurbo8, and black for "bad"


def test_host_depth_index_stands_under_the_depth_rule(shim):
    g = R.golden()
    depth, opacity, weight = R.depth_case()
    for w, tag in ((opacity, "depth_rgb"), (weight, "depth_rgb_bool")):
        idx = shim_index(shim, depth, w)
        n = R.depth_rule(shim_turbo(shim, idx), depth, w)
        n_ref = int(np.any(shim_turbo(shim, idx) != g[tag], axis=-1).sum())
        print(f"\nhost vf_depth_index, {tag}: {n} of {depth.size} pixels differ from the float64 restatement, {n_ref} from the reference's record")
        assert (idx[np.isnan(depth) | (depth < 0)] == 0).all()      # nan_to_num
    big = np.exp(np.random.default_rng(3).uniform(np.log(2.0), np.log(200.0), (135, 240))).astype(np.float32)
    wbig = np.random.default_rng(4).uniform(0, 1, big.shape).astype(np.float32)
    n = R.depth_rule(shim_turbo(shim, shim_index(shim, big, wbig)), big, wbig)
    n32 = int((shim_index(shim, big, wbig) != R.depth_index(big, wbig, np.float32)).sum())
    print(f"\nhost vf_depth_index, 135 x 240: {n} pixels differ from the float64 restatement, {n32} from the float32 mode")
    # the edges of the curve and of the weight
    d = np.float32([0.0, -3.0, np.nan, 4.0, 120.0, 1e10, np.inf, 10.0, 10.0, 10.0, 10.0, 10.0, 0.0])
    w = np.float32([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.nan, np.inf, -1.0, 0.0, 2.0, np.inf])
    idx = shim_index(shim, d, w)
    assert np.array_equal(idx, R.depth_index(d, w, np.float32)) and np.array_equal(idx, R.depth_index(d, w, np.float64))
    assert idx.tolist() == [255, 0, 0, 255, 0, 0, 0, R.BAD, 255, 0, 0, 255, 255]
    assert shim_index(shim, np.float32([1e10]), np.float32([np.inf])).tolist() == [R.BAD]      # 0 * inf: matplotlib's "bad"


# ---- 3. the C entry -----------------------------------------------------------------------------------------------------------------------
def test_entry_resolves_with_the_declared_signature():
    full = open(os.path.join(ROOT, "include", "bds.h")).read()
    decl = {k: v for k, v in declared_signatures().items() if k.startswith("bds_video")}
    assert sorted(decl) == ["bds_video_frame"]
    ret, args = decl["bds_video_frame"]
    res, argtypes = L._SIGS["bds_video_frame"]
    assert res is ret is ctypes.c_int and len(argtypes) == len(args) == 6
    assert argtypes == [ctypes.c_int, ctypes.POINTER(L.BdsVideoPanel), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib = L.lib()
    assert list(lib.bds_video_frame.argtypes) == argtypes
    assert ctypes.sizeof(L.BdsVideoPanel) == 56 and L.BdsVideoPanel.dst_y.offset == 36
    assert "video.hip" in B.SOURCES
    assert lib.bds_abi_version() == L.ABI_VERSION == 7      # (what each version changed: include/bds.h)
    for cite in ("models/video_utils.py:703-768", ":771-857", "utils/visualization.py:19-22", ":201-227", ":265-271"):
        assert cite in full, cite
    kernel = open(os.path.join(B.CSRC, "video.hip")).read()
    header = open(os.path.join(B.CSRC, "video_math.h")).read().split("namespace bds {", 1)[1]
    assert "atomic" not in kernel.split("namespace bds {", 1)[1]      # no atomics: bit-identical run to run
    assert "logf" not in kernel and "255.0f" not in kernel             # the formulas are stated in the header only
    assert header.count("logf(") == 1 and header.count("255.0f *") == 1 and "__logf" not in header
    assert (V.RGB, V.GRAY, V.DEPTH, V.OVER_GREEN, V.LIDAR_ON_IMAGE) == tuple(
        int(full.split(f"#define BDS_VIDEO_{n} ")[1].split()[0]) for n in ("RGB", "GRAY", "DEPTH", "OVER_GREEN", "LIDAR_ON_IMAGE"))


def test_video_kernel_resources():
    res = {short_name(k): v for k, v in kernel_resources("video.hip").items()}
    assert sorted(res) == ["video_frame_kernel"], list(res)
    for k, v in res.items():
        print(f"\n{k}: occupancy {v['Occupancy']} waves/SIMD, {v['VGPRs']} VGPRs, static LDS {v['LDS Size']} bytes")
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 8, (k, v)      # a stream-bound pass: nothing spilled, every wave slot usable


def test_entry_rejects_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first

    def call(n=1, Hc=8, Wc=9, canvas=p, **kw):
        table = (L.BdsVideoPanel * 2)()
        base = dict(src0=p, src1=None, kind=V.RGB, flags=0, src_h=4, src_w=5, src_row0=0, dst_y=1, dst_x=2, dst_h=4, dst_w=5, reserved=0)
        for k, v in {**base, **kw}.items():
            setattr(table[0], k, v)
        return lib.bds_video_frame(n, table, Hc, Wc, canvas, None)
    # nothing to do: 0
    assert lib.bds_video_frame(0, None, 0, 0, None, None) == 0 and lib.bds_video_frame(0, None, 0, 7, None, None) == 0
    assert call(Hc=0, dst_y=0, dst_h=0) == 0
    for kw in (dict(n=-1), dict(Hc=-1), dict(Wc=-1), dict(Hc=1 << 15, Wc=1 << 15), dict(canvas=None), dict(canvas=p + 2),
               dict(kind=-1), dict(kind=5), dict(flags=4), dict(flags=V.SRC0_BYTES), dict(kind=V.GRAY, flags=V.SRC1_BYTES), dict(reserved=1),
               dict(src0=None), dict(src0=p + 2), dict(kind=V.GRAY, src0=p + 1), dict(kind=V.GRAY, src1=p),
               dict(kind=V.OVER_GREEN), dict(kind=V.LIDAR_ON_IMAGE), dict(kind=V.DEPTH, src1=p + 1), dict(kind=V.OVER_GREEN, src1=p + 2),
               dict(src_h=-1), dict(src_w=-1), dict(src_h=1 << 15, src_w=1 << 15), dict(src_row0=-1), dict(src_row0=1), dict(dst_w=6),
               dict(dst_y=-1), dict(dst_x=-1), dict(dst_h=-1), dict(dst_w=-1), dict(dst_y=5), dict(dst_x=5)):
        assert call(**kw) == L.BDS_EINVAL == -1, kw
    assert lib.bds_video_frame(1, None, 8, 9, p, None) == L.BDS_EINVAL
    # more than 64 panels on one row: refused before any launch
    table = (L.BdsVideoPanel * 65)()
    for t in table:
        t.src0, t.kind, t.src_h, t.src_w, t.dst_h, t.dst_w = p, V.GRAY, 1, 1, 1, 1
    assert lib.bds_video_frame(65, table, 1, 1, p, None) == L.BDS_ECAPACITY == -4


def test_python_refuses_cpu_tensors_and_bad_shapes():
    import bilateral_driving_amd
    assert bilateral_driving_amd.video is V
    rgb, gray = torch.rand(5, 7, 3), torch.rand(5, 7)
    for fn in (lambda: V.to8b(rgb), lambda: V.to8b(gray), lambda: V.depth_visualizer(gray, gray), lambda: V.over_green(rgb, gray),
               lambda: V.lidar_on_image(rgb, gray),
               lambda: V.FrameComposer("nuscenes", ["rgbs"]).frame({"rgbs": [rgb], "cam_names": ["CAM_FRONT"]}, ["CAM_FRONT"])):
        with pytest.raises(L.BdsError):
            fn()
    for fn in (lambda: V.over_green(rgb, gray[:4]), lambda: V.depth_visualizer(rgb, gray), lambda: V.lidar_on_image(gray, gray),
               lambda: V.over_green(rgb, None)):
        with pytest.raises(ValueError):
            fn()
    with pytest.raises(ValueError):
        V._dataset_type(lambda imgs, names: None)
    vis = types.SimpleNamespace(layout_nuplan=lambda imgs, names: None)
    vis.layout_nuplan.__name__ = "layout_nuplan"
    assert V._dataset_type(vis.layout_nuplan) == "nuplan" and V._dataset_type("kitti") == "kitti"


# ---- 4. the seam --------------------------------------------------------------------------------------------------------------------------
def test_install_and_uninstall_put_back_what_was_there():
    module = types.ModuleType("video_utils_stand_in")
    former = module.save_concatenated_videos = lambda *a, **k: "former"
    V.install(module)
    V.install(module)      # (twice: the former function is still the one remembered)
    assert module.save_concatenated_videos is V.save_concatenated_videos and module.save_seperate_videos is V.save_seperate_videos
    other = types.ModuleType("another")
    V.install(other)
    V.uninstall(other)
    assert not hasattr(other, "save_concatenated_videos") and module.save_seperate_videos is V.save_seperate_videos
    V.uninstall()
    assert module.save_concatenated_videos is former and not hasattr(module, "save_seperate_videos")


# ---- 5. the key rules, with a fake launch ---------------------------------------------------------------------------------------------------
@pytest.fixture
def launches(monkeypatch):
    log = []

    def fake(panels, Hc, Wc, device):
        log.append((list(panels), Hc, Wc))
        return torch.zeros(Hc, Wc, 3, dtype=torch.uint8)
    monkeypatch.setattr(V, "_launch", fake)
    monkeypatch.setattr(V, "_default_device", lambda: torch.device("cpu"))      # where numpy lists would be uploaded to
    return log


def host_paint(panels, Hc, Wc):
    """What the kernel would write, from the restatement: the panels painted in order."""
    canvas = np.zeros((Hc, Wc, 3), np.uint8)
    for p in panels:
        a, b = p.src0.numpy(), None if p.src1 is None else p.src1.numpy()
        if p.kind == V.RGB:
            img = R.to8b(a)
        elif p.kind == V.GRAY:
            img = R.to8b(np.stack([a, a, a], -1))
        else:
            assert p.kind == V.DEPTH
            img = R.depth_image(a, b)
        r = p.rect
        canvas[r.y:r.y + r.h, r.x:r.x + r.w] = img[r.row0:r.row0 + r.h, :r.w]
    return canvas


@pytest.mark.parametrize("dataset_type", sorted(R.MERGED))
def test_frame_composer_follows_the_references_key_rules(dataset_type, launches):
    names = R.MERGED[dataset_type]
    rr = R.render_results(dataset_type, names)
    composer = V.FrameComposer(dataset_type, R.MERGED_KEYS, device="cpu")
    for i in range(R.MERGED_T):
        del launches[:]
        composer.frame(rr, names, i * len(names))
        assert len(launches) == 1                                      # one launch per finished frame
        panels, Hc, Wc = launches[0]
        want = R.merged_frame(dataset_type, rr, R.MERGED_KEYS, i, len(names))[0]
        assert (Hc, Wc, 3) == want.shape == R.golden()[f"concat_{dataset_type}"][i].shape
        assert np.array_equal(host_paint(panels, Hc, Wc), want)
        assert [p.kind for p in panels] == [k for k in (V.RGB, V.RGB, V.DEPTH, V.DEPTH, V.GRAY) for _ in names]      # gt_sky_masks: skipped
        depth_panels = [p for p in panels if p.kind == V.DEPTH]
        assert all(np.array_equal(p.src1.numpy(), rr["opacities"][i * len(names) + c]) for c, p in enumerate(depth_panels[:len(names)]))
        assert all(np.array_equal(p.src1.numpy(), rr["Dynamic_opacities"][i * len(names) + c]) for c, p in enumerate(depth_panels[len(names):]))
        assert all(np.array_equal(p.src0.numpy(), rr["RigidNodes_opacities"][i * len(names) + c]) for c, p in enumerate(panels[-len(names):]))
        assert all(p.rect.y + p.rect.h <= Hc and p.rect.x + p.rect.w <= Wc for p in panels)


def test_key_rules_skip_and_fall_back_as_the_reference(launches):
    names = ["CAM_FRONT", "CAM_BACK"]
    rr = R.render_results("nuscenes", names, T=1)
    rr["median_depths"], rr["lidar_on_images"], rr["Background_depths"], rr["empty_rgbs"] = rr["depths"], [a.astype(np.float64) for a in rr["rgbs"]], rr["depths"], []
    composer = V.FrameComposer("nuscenes", ["rgbs"], device="cpu")
    at = slice(0, 2)
    assert V.key_sources(rr, "absent_rgbs", at) is None and V.key_sources(rr, "empty_rgbs", at) is None
    assert V.key_sources(rr, "Background_depths", at) is None                      # no Background_opacities: skipped
    assert V.key_sources(rr, "SMPLNodes_mask", at) is None and V.key_sources(rr, "gt_sky_masks", at) is None
    median = V.key_sources(rr, "median_depths", at)                                 # falls back to ``opacities``
    assert [k for k, _, _ in median] == [V.DEPTH] * 2 and all(o is rr["opacities"][c] for c, (_, _, o) in enumerate(median))
    assert [k for k, _, _ in V.key_sources(rr, "Dynamic_mask", at)] == [V.GRAY] * 2
    assert V.key_sources(rr, "Dynamic_mask", at)[1][1] is rr["Dynamic_opacities"][1]
    assert composer.key_frame("absent_rgbs", rr, names) is None and composer.key_frame("gt_sky_masks", rr, names) is None and not launches
    composer.key_frame("lidar_on_images", rr, names)
    panels, Hc, Wc = launches[-1]
    assert all(p.src0.dtype == torch.float32 for p in panels) and (Hc, Wc) == (2 * R.H - 1, R.W - 1)      # float64 lists are shown as float32
    # [h,w,1] device-style maps and bool weights are taken as they are
    rr["opacities"] = [torch.from_numpy(o)[..., None] > 0.5 for o in rr["opacities"]]
    composer.key_frame("depths", rr, names)
    assert all(p.src1.dtype == torch.uint8 and p.src1.dim() == 2 for p in launches[-1][0])
    with pytest.raises(ValueError):
        V.FrameComposer("nuscenes", ["absent_rgbs", "gt_sky_masks"], device="cpu").frame(rr, names)      # nothing to concatenate
    with pytest.raises(IndexError):
        composer.key_frame("rgbs", rr, names, first=2)      # past the lists' end: the reference's imgs[0]


def test_save_functions_write_what_the_composer_gives(launches):
    names = R.MERGED["waymo"]
    rr = R.render_results("waymo", names)
    log = []
    got = V.save_concatenated_videos(rr, "out/video.mp4", "waymo", R.MERGED_T, keys=R.MERGED_KEYS, num_cams=3, verbose=False,
                                     writer_factory=R.writer_factory(log))
    assert len(log) == 1 and log[0].path == "out/video.mp4" and log[0].kw == {"mode": "I", "fps": 10} and log[0].closed
    assert len(log[0].frames) == R.MERGED_T == len(launches) and got["concatenated_frame"].shape == log[0].frames[1].shape
    del log[:], launches[:]
    got = V.save_seperate_videos(rr, "out/video.mp4", "waymo", 1, keys=R.MERGED_KEYS + ["absent_rgbs"], num_cams=3, writer_factory=R.writer_factory(log))
    assert [w.path for w in log] == [f"out/video_{k}.mp4" for k in R.MERGED_KEYS + ["absent_rgbs"]] and all(w.kw == {"mode": "I"} for w in log)
    assert list(got) == R.MERGED_KEYS[:-1] and [len(w.frames) for w in log] == [1] * 5 + [0, 0]
    assert [w.closed for w in log] == [True] * 6 + [False]      # as in the reference: a key that is absent leaves its writer open
