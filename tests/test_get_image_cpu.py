"""A view's input preparation (bilateral_driving_amd/pixels.py, csrc/pixels.hip) on the CPU: the numpy restatement
(tests/get_image_ref64.py) against the reference's recorded results (tests/golden/get_image.npz, scripts/gen_golden_get_image.py), the
device math on the host (tests/hostmath_pixels_shim.hip) against both, the resize windows against torch's own host kernels at awkward
factors, the kernels' resources, and the C entries' signatures and argument checks.

What is compared how.  Integer fields, ``pixel_coords``, ``origins``, the fills, the masks, the lidar map and the intrinsics are
compared by bits with the restatement's float32 mode.  ``viewdirs``, ``direction_norm`` and the antialiased image are held to the
measured bound of tests/get_image_ref64.py (``bound``): four times the distance of the float32 framework expression from float64 on
the same inputs, at least 1e-6; each test prints the figures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from tests import get_image_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_INFO = ("pixel_coords", "origins", "normed_time", "img_idx", "frame_idx", "lidar_depth_map") + R.MASK_KEYS
EXACT_CAM = ("cam_id", "camera_to_world", "height", "width", "intrinsics")
BOUNDED = ("viewdirs", "direction_norm", "pixels")
RESIZE_CASES = ((13, 21, 0.5), (17, 23, 0.25), (9, 9, 0.3), (31, 45, 0.125), (12, 20, 1.0 / 3.0), (10, 14, 0.7))
AWKWARD = (0.3, 1.0 / 3.0, 0.7, 0.125)


def module():
    from bilateral_driving_amd import pixels
    return pixels


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the restatement against the reference's recorded results -----------------------------------------------------------------------
@pytest.mark.parametrize("factor", R.FACTORS)
def test_restatement_equals_the_references_get_image(factor):
    z = R.golden()
    cam, _ = R.golden_camera()
    for frame in range(R.GOLDEN_FRAMES):
        exact = {**R.get_image(cam, frame, factor, np.float64)[0], **R.get_image(cam, frame, factor, np.float64)[1]}
        f32 = {**R.get_image(cam, frame, factor, np.float32)[0], **R.get_image(cam, frame, factor, np.float32)[1]}
        keys = sorted(k.split("_", 2)[2] for k in z if k.startswith(f"f{factor}_{frame}_"))
        assert keys == sorted(EXACT_INFO + EXACT_CAM + BOUNDED)
        for k in EXACT_INFO + EXACT_CAM:
            assert same_bits(z[f"f{factor}_{frame}_{k}"], f32[k]), (factor, frame, k)
        Ho, Wo = R.output_size(R.GOLDEN_H, R.GOLDEN_W, factor)
        assert int(z[f"f{factor}_{frame}_height"]) == Ho and int(z[f"f{factor}_{frame}_width"]) == Wo
        for k in BOUNDED:
            gold = z[f"f{factor}_{frame}_{k}"]
            b, err = R.bound(f32[k], exact[k]), float(np.max(np.abs(gold.astype(np.float64) - exact[k])))
            print(f"\nget_image factor {factor} frame {frame} {k}: the reference's float32 {err:.2e} from float64, bound {b:.2e}")
            assert gold.dtype == np.float32 and gold.shape == exact[k].shape and err <= b


def test_restatement_equals_the_references_novel_views():
    z = R.golden()
    cam, traj = R.golden_camera()
    n = int(z["novel_num_frames"])
    exact, f32 = R.novel_views(cam, traj, n, np.float64), R.novel_views(cam, traj, n, np.float32)
    assert len(traj) == R.GOLDEN_POSES
    for i in range(len(traj)):
        for k in ("pixel_coords", "origins", "normed_time", "img_idx", "frame_idx"):
            assert same_bits(z[f"novel_{i}_{k}"], f32[i][k]), (i, k)
        for k in ("viewdirs", "direction_norm"):
            err = float(np.max(np.abs(z[f"novel_{i}_{k}"].astype(np.float64) - exact[i][k])))
            assert err <= R.bound(f32[i][k], exact[i][k])
    assert [int(z[f"novel_{i}_frame_idx"][0, 0]) for i in range(3)] == [0, 3, 6]


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("pixels")
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    h.hm_px_view.argtypes = [vp, vp, ctypes.c_float, ci, ci, vp, vp, vp, vp, vp]
    h.hm_px_view.restype = None
    h.hm_px_aa_window.argtypes = [ci, cd, ci, vp, vp]
    h.hm_px_aa_max_taps.argtypes = [cd]
    h.hm_px_resize_aa.argtypes = [ci, ci, ci, ci, cd, vp, vp]
    h.hm_px_resize_aa.restype = None
    h.hm_px_resize_nearest.argtypes = [ci, ci, ci, ci, cd, vp, vp]
    h.hm_px_resize_nearest.restype = None
    return h


def shim_view(shim, c2w, K, scale, H, W):
    c2w, K = np.ascontiguousarray(c2w, np.float32), np.ascontiguousarray(K, np.float32)
    o, v, n, c = (np.zeros((H, W, k), np.float32) for k in (3, 3, 1, 2))
    intr = np.zeros((3, 3), np.float32)
    shim.hm_px_view(c2w.ctypes.data, K.ctypes.data, scale, H, W, o.ctypes.data, v.ctypes.data, n.ctypes.data, c.ctypes.data, intr.ctypes.data)
    return {"origins": o, "viewdirs": v, "direction_norm": n, "pixel_coords": c, "intrinsics": intr}


def shim_resize(shim, img, factor):
    H, W = img.shape[:2]
    Ho, Wo = R.output_size(H, W, factor)
    img, out = np.ascontiguousarray(img, np.float32), np.zeros((Ho, Wo, 3), np.float32)
    shim.hm_px_resize_aa(H, W, Ho, Wo, factor, img.ctypes.data, out.ctypes.data)
    return out


def shim_nearest(shim, mask, factor):
    H, W = mask.shape
    Ho, Wo = R.output_size(H, W, factor)
    mask, out = np.ascontiguousarray(mask, np.float32), np.zeros((Ho, Wo), np.float32)
    shim.hm_px_resize_nearest(H, W, Ho, Wo, factor, mask.ctypes.data, out.ctypes.data)
    return out


@pytest.mark.parametrize("factor", R.FACTORS)
def test_host_fields_equal_the_reference(shim, factor):
    z = R.golden()
    cam, _ = R.golden_camera()
    Ho, Wo = R.output_size(R.GOLDEN_H, R.GOLDEN_W, factor)
    for frame in range(R.GOLDEN_FRAMES):
        got = shim_view(shim, cam["cam_to_worlds"][frame], cam["intrinsics"][frame], factor, Ho, Wo)
        for k in ("origins", "pixel_coords", "intrinsics"):
            assert same_bits(got[k], z[f"f{factor}_{frame}_{k}"]), (frame, k)
        exact = R.rays(cam["cam_to_worlds"][frame], cam["intrinsics"][frame], factor, Ho, Wo, np.float64)
        f32 = R.rays(cam["cam_to_worlds"][frame], cam["intrinsics"][frame], factor, Ho, Wo, np.float32)
        for k, e, s in (("viewdirs", exact[1], f32[1]), ("direction_norm", exact[2], f32[2])):
            b, err = R.bound(s, e), float(np.max(np.abs(got[k].astype(np.float64) - e)))
            to_ref = float(np.max(np.abs(got[k].astype(np.float64) - z[f"f{factor}_{frame}_{k}"])))
            print(f"\nshim factor {factor} frame {frame} {k}: {err:.2e} from float64 (bound {b:.2e}), {to_ref:.2e} from the reference's float32")
            assert err <= b
            assert same_bits(got[k], s)      # every operation rounded on its own: the restatement's float32 bits


@pytest.mark.parametrize("spec", [(1, 1, 1.0, 0.0), (3, 5, 1.0, 0.0), (5, 13, 0.5, 0.0), (33, 37, 0.25, 0.0), (7, 9, 1.0, 1000.0)])
def test_host_fields_match_the_restatement_on_random_views(shim, spec):
    H, W, scale, far = spec
    case = R.view_case(H * 100 + W, 2, H, W, far)
    for b in range(2):
        got = shim_view(shim, case["c2w"][b], case["K"][b], scale, H, W)
        o, v, n, c = R.rays(case["c2w"][b], case["K"][b], scale, H, W, np.float32)
        assert same_bits(got["origins"], o) and same_bits(got["pixel_coords"], c) and same_bits(got["viewdirs"], v) and same_bits(got["direction_norm"], n)
        assert same_bits(got["intrinsics"], R.scaled_intrinsics(case["K"][b], scale))
        e = R.rays(case["c2w"][b], case["K"][b], scale, H, W, np.float64)
        assert np.max(np.abs(got["viewdirs"] - e[1])) <= R.bound(v, e[1]) and np.max(np.abs(got["direction_norm"] - e[2])) <= R.bound(n, e[2])
        assert np.all(np.abs(np.linalg.norm(got["viewdirs"].astype(np.float64), axis=-1) - 1) < 1e-6)


@pytest.mark.parametrize("case", RESIZE_CASES)
@pytest.mark.parametrize("kind", ["noise", "step", "constant"])
def test_host_resize_matches_the_restatement_and_torch(shim, case, kind):
    H, W, factor = case
    img = R.image_case(kind, H, W)
    got = shim_resize(shim, img, factor)
    exact, f32 = R.resize_aa(img, factor, np.float64), R.resize_aa(img, factor, np.float32)
    t = torch.from_numpy(img).permute(2, 0, 1)[None]
    ref32 = torch.nn.functional.interpolate(t, scale_factor=factor, mode="bicubic", antialias=True)[0].permute(1, 2, 0).numpy()
    ref64 = torch.nn.functional.interpolate(t.double(), scale_factor=factor, mode="bicubic", antialias=True)[0].permute(1, 2, 0).numpy()
    assert got.shape == ref32.shape == exact.shape
    assert np.max(np.abs(exact - ref64)) <= 1e-12      # the restatement is torch's resize
    b = max(R.bound(ref32, ref64), R.bound(f32, exact))
    err = float(np.max(np.abs(got.astype(np.float64) - exact)))
    print(f"\nresize {H}x{W} x{factor:.4f} {kind}: shim {err:.2e} from float64; torch's float32 {np.max(np.abs(ref32 - ref64)):.2e}, "
          f"the restatement's float32 {np.max(np.abs(f32 - exact)):.2e}; bound {b:.2e}")
    assert err <= b
    assert same_bits(got, f32)      # tap by tap, no fused multiply-add
    if kind == "constant":
        assert np.max(np.abs(got.astype(np.float64) - 0.7)) <= b


def test_host_resize_of_the_golden_images(shim):
    z = R.golden()
    cam, _ = R.golden_camera()
    for factor in R.FACTORS[1:]:
        for frame in range(R.GOLDEN_FRAMES):
            got = shim_resize(shim, cam["images"][frame], factor)
            exact, f32 = R.resize_aa(cam["images"][frame], factor, np.float64), R.resize_aa(cam["images"][frame], factor, np.float32)
            b = R.bound(f32, exact)
            assert np.max(np.abs(got.astype(np.float64) - exact)) <= b
            assert np.max(np.abs(got.astype(np.float64) - z[f"f{factor}_{frame}_pixels"])) <= 2 * b      # both within b of float64
            for attr, key in zip(R.MASKS, R.MASK_KEYS):
                m = cam[attr] if attr == "egocar_mask" else cam[attr][frame]
                assert same_bits(shim_nearest(shim, m, factor), z[f"f{factor}_{frame}_{key}"])
    img = cam["images"][0]
    assert same_bits(shim_resize(shim, img, 1.0), img)      # factor 1: the identity


@pytest.mark.parametrize("factor", AWKWARD)
def test_windows_equal_torchs_at_awkward_factors(shim, factor):
    """The resize of an impulse shows a window's support and weights: column i of the result of e_j is weight (i, j)."""
    n_in = 41
    n_out = int(np.floor(n_in * factor))
    eye = torch.eye(n_in, dtype=torch.float64)[None, None]                    # rows: impulses along the width
    ref = torch.nn.functional.interpolate(eye, scale_factor=(1.0, factor), mode="bicubic", antialias=True, recompute_scale_factor=False)[0, 0].numpy()
    cap = shim.hm_px_aa_max_taps(factor)
    for i in range(n_out):
        lo, w = R.aa_window(i, R.axis_scale(factor, np.float64), n_in, np.float64)
        mine = np.zeros(n_in)
        mine[lo:lo + len(w)] = w
        assert np.max(np.abs(mine - ref[:, i])) <= 1e-12, (factor, i)
        lo32, w32 = R.aa_window(i, R.axis_scale(factor, np.float32), n_in, np.float32)
        slo, sw = ctypes.c_int(0), np.zeros(cap, np.float32)
        n = shim.hm_px_aa_window(i, factor, n_in, ctypes.byref(slo), sw.ctypes.data)
        assert n == len(w32) <= cap and slo.value == lo32 and same_bits(sw[:n], w32)
        # float32 weights: the centre c <= n_in, its difference from the tap and the scale are each rounded to 2^-24 relative, so a
        # weight's argument moves by at most 4 * 2^-24 * n_in and the weight by the cubic's steepest slope (1.39 < 1.5) times that; a
        # window cut one tap otherwise than in float64 differs there by a weight that small
        dev = np.zeros(n_in)
        dev[lo32:lo32 + n] = sw[:n]
        assert np.max(np.abs(dev - ref[:, i])) <= 1.5 * 4 * 2.0 ** -24 * n_in, (factor, i)
    masks = R.mask_case(1, 37, n_in)[0]
    t = torch.nn.functional.interpolate(torch.from_numpy(masks)[None, None], scale_factor=factor, mode="nearest")[0, 0].numpy()
    assert same_bits(shim_nearest(shim, masks, factor), t) and same_bits(R.resize_nearest(masks, factor), t)


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_pixels_kernel_resources():
    assert "pixels.hip" in B.SOURCES
    res = {short_name(k): v for k, v in kernel_resources("pixels.hip").items()}
    want = ["view_fields_kernel", "image_resize_aa_kernel", "masks_resize_nearest_kernel"]
    assert sorted(res) == sorted(want), list(res)
    for k in want:
        print(f"\n{k}: occupancy {res[k]['Occupancy']} waves/SIMD, {res[k]['VGPRs']} VGPRs, static LDS {res[k]['LDS Size']} bytes")
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["Occupancy"] >= 8, (k, res[k])
    src = open(os.path.join(B.CSRC, "pixels.hip")).read()
    assert "atomic" not in src.split("namespace bds {", 1)[1]      # no atomics: bit-identical run to run


def test_entries_resolve_with_the_declared_signatures():
    full = open(os.path.join(ROOT, "include", "bds.h")).read()
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_view_fields|bds_image_resize_aa|bds_masks_resize_nearest", k)}
    assert sorted(decl) == ["bds_image_resize_aa", "bds_masks_resize_nearest", "bds_view_fields"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    P = module()
    assert f"#define BDS_PIXELS_MAX_MASKS {P.MAX_MASKS}\n" in hdr and P.MAX_MASKS == 5
    assert f"#define BDS_PIXELS_MAX_SCALE {P.MAX_SCALE}\n" in hdr
    assert lib.bds_abi_version() == L.ABI_VERSION == 7      # (what each version changed: include/bds.h)
    for cite in ("datasets/base/pixel_source.py:477-657", "pixel_source.py:38-75", ":1070-1132", ":492-502", ":520-579"):
        assert cite in full, cite
    for path in (os.path.join(B.CSRC, "pixels.hip"), os.path.join(B.CSRC, "pixels_math.h")):
        assert "datasets/base/pixel_source.py:477-657" in open(path).read(), path


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first

    def fields(B=2, H=12, W=20, c2w=p, K=p, nK=1, scale=1.0, t=p, ids=p, o=p, v=p, n=p, c=p, to=p, im=p, fr=p, cm=p, ko=p):
        return lib.bds_view_fields(B, H, W, c2w, K, nK, scale, t, ids, o, v, n, c, to, im, fr, cm, ko, None)
    assert fields(B=0) == 0 and fields(H=0) == 0 and fields(W=0) == 0
    assert lib.bds_view_fields(0, 0, 0, None, None, 0, 0.0, *([None] * 12)) == 0
    for kw in (dict(B=-1), dict(B=65536), dict(H=-1), dict(W=-2), dict(c2w=None), dict(K=None), dict(nK=0), dict(nK=3), dict(scale=0.0),
               dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(t=None), dict(ids=None), dict(ids=None, to=None),
               dict(c2w=p + 2), dict(K=p + 1), dict(t=p + 2), dict(ids=p + 4), dict(o=p + 4), dict(v=p + 8), dict(n=p + 4), dict(c=p + 8),
               dict(to=p + 4), dict(im=p + 8), dict(fr=p + 8), dict(cm=p + 8), dict(ko=p + 2), dict(B=4, H=1 << 15, W=1 << 14),
               dict(B=1, H=1 << 16, W=1 << 15)):
        assert fields(**kw) == L.BDS_EINVAL, kw

    def image(H=12, W=20, s=0.5, src=p, dst=p):
        return lib.bds_image_resize_aa(H, W, s, src, dst, None)
    assert image(H=0) == 0 and image(H=1, W=1) == 0      # floor(1 * 0.5) = 0: nothing to write
    for kw in (dict(s=1.5), dict(s=1.0000001), dict(s=0.0), dict(s=-0.5), dict(s=float("nan")), dict(src=None), dict(dst=None), dict(H=-1),
               dict(W=-1), dict(src=p + 2), dict(dst=p + 1), dict(H=1 << 15, W=1 << 15),
               dict(s=1.0 / 513, H=2048, W=2048), dict(s=1e-3, H=4096, W=4096)):
        assert image(**kw) == L.BDS_EINVAL, kw

    def masks(n=5, H=12, W=20, s=0.5, src=None, dst=None):
        src = (ctypes.c_void_p * 8)(*([p] * 8)) if src is None else src
        dst = (ctypes.c_void_p * 8)(*([p] * 8)) if dst is None else dst
        return lib.bds_masks_resize_nearest(n, H, W, s, src, dst, None)
    assert masks(n=0) == 0 and masks(H=0) == 0 and masks(H=1) == 0
    holes = (ctypes.c_void_p * 8)(p, p, None, p, p, p, p, p)
    for kw in (dict(n=6), dict(n=-1), dict(s=2.0), dict(s=0.0), dict(s=float("nan")), dict(H=-1), dict(src=holes), dict(dst=holes),
               dict(H=1 << 16, W=1 << 15)):
        assert masks(**kw) == L.BDS_EINVAL, kw
    assert lib.bds_masks_resize_nearest(2, 12, 20, 0.5, None, None, None) == L.BDS_EINVAL


def test_python_checks_arguments_and_refuses_cpu_tensors():
    P = module()
    import bilateral_driving_amd
    assert bilateral_driving_amd.pixels is P
    cam, traj = R.golden_camera()
    c2w, K = torch.from_numpy(cam["cam_to_worlds"]), torch.from_numpy(cam["intrinsics"])
    with pytest.raises(L.BdsError):
        P.view_fields(c2w, K, 12, 20, img_idx=[0, 1, 2], frame_idx=[0, 1, 2])
    with pytest.raises(L.BdsError):
        P.resize_image(torch.rand(12, 20, 3), 0.5)
    with pytest.raises(L.BdsError):
        P.resize_masks([torch.rand(12, 20)], 0.5)
    with pytest.raises(L.BdsError):
        P.get_image(R.BareCamera(cam, 1.0, "cpu"), 0)
    with pytest.raises(L.BdsError):
        P.prepare_novel_view_render_data(R.bare_pixel_source(cam, "cpu", 7), "waymo", torch.from_numpy(traj))
    with pytest.raises(NotImplementedError):
        P.resize_image(torch.rand(12, 20, 3), 2.0)
    with pytest.raises(NotImplementedError):
        P.resize_masks([torch.rand(12, 20)], 1.5)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1.0 / 513, 1e-4):
        with pytest.raises(ValueError):
            P.resize_image(torch.rand(12, 20, 3), bad)
    assert P.MAX_SCALE == 512
    for args in ((torch.rand(12, 20), 0.5), (torch.rand(12, 20, 4), 0.5)):
        with pytest.raises(ValueError):
            P.resize_image(*args)
    with pytest.raises(ValueError):
        P.resize_masks([torch.rand(12, 20)] * 6, 0.5)
    with pytest.raises(ValueError):
        P.resize_masks([torch.rand(12, 20), torch.rand(12, 21)], 0.5)
    assert P.resize_masks([], 0.5) == []
    for kw in (dict(c2w=c2w[:, :3]), dict(K=K[:2]), dict(K=K[:, :2]), dict(H=-1), dict(scale=0.0), dict(scale=float("nan"))):
        a = {"c2w": c2w, "K": K, "H": 12, "scale": 1.0, **kw}
        with pytest.raises(ValueError):
            P.view_fields(a["c2w"], a["K"], a["H"], 20, scale=a["scale"], img_idx=0, frame_idx=0)

    # install / uninstall: an object on the CPU keeps the class's own method
    class Camera:
        def get_image(self, frame_idx):
            return "former"

    class Source:
        def prepare_novel_view_render_data(self, dataset_type, traj):
            return "former"
    former = Camera.__dict__["get_image"]
    P.install(Camera, Source)
    P.install(Camera, Source)      # (twice: the former function is still the one remembered)
    assert Camera.__dict__["get_image"] is not former and Camera.get_image.__wrapped__ is P.get_image
    cpu_cam = Camera()
    cpu_cam.cam_to_worlds = c2w
    assert cpu_cam.get_image(0) == "former"
    src = Source()
    src.camera_data = {0: cpu_cam}
    assert src.prepare_novel_view_render_data("waymo", None) == "former"
    class Derived(Camera):      # inherits get_image: a CPU object still reaches it
        pass
    P.install(Derived)
    inherited = Derived()
    inherited.cam_to_worlds = c2w
    assert "get_image" in Derived.__dict__ and inherited.get_image(0) == "former"
    P.uninstall(Derived)
    assert "get_image" not in Derived.__dict__ and inherited.get_image(0) == "former"

    class Bare:
        pass
    P.install(Bare)
    assert Bare.get_image.__wrapped__ is P.get_image
    P.uninstall()
    assert Camera.__dict__["get_image"] is former and Source().prepare_novel_view_render_data("waymo", None) == "former"
    assert "get_image" not in Bare.__dict__
