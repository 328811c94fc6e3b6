"""The lens undistortion (bilateral_driving_amd/undistort.py, csrc/undistort.hip) on the CPU: the header's map and taps on the host
(tests/hostmath_undistort_shim.hip) against the numpy restatement (tests/undistort_ref64.py) bit for bit, known answers that do not
lean on the restatement, ``optimal_new_camera_matrix``, the kernel's resources, the C entry's signature and argument checks, and the
seam.  OpenCV is not installed: nothing here is compared with OpenCV itself (parity unpinned).

The fixed cases (undistort_ref64.CASES at F = 3, H = 37, W = 53) are the GPU test's; what they hold is asserted here from the float64
map: every 32 u and 32 v stays at least 2e-5 from a rounding tie (asserted >= 1e-6: an ulp of host / device difference cannot flip a
pixel), "zero" has 89 partial pixels (the last row and column), "pincushion" 126 partial and 265 fully outside, "pin+shift" source
coordinates down to -64 px with 20 live pixels at sx = -1 and 31 / 9 / 8 pixels at sy = -1 / sx = W - 1 / sy = H - 1.

``optimal_new_camera_matrix``: the restatement's re-distortion residual of the 81 grid points (the undistorted points pushed through
the forward model again, in pixels) is 4.4e-07 px for the mild set (-0.05, 0.01, 0.001, -0.0005, 0) at 53 x 37, 0.015 px for "pincushion" and 0.10 px for "barrel": that is how
far OpenCV's five fixed iterations are from the model's inverse, not an error of either implementation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from tests import lidar_ref64 as LR
from tests import undistort_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources

MILD = (-0.05, 0.01, 0.001, -0.0005, 0.0)
KINDS = {"uint8": 0, "unit": 1, "mask": 2}


def table(K, dist, new_K=None, frames=None):
    from bilateral_driving_amd import undistort
    return np.ascontiguousarray(undistort.camera_table(K, dist, new_K, frames))


@pytest.fixture(scope="module")
def shim():
    h = build_shim("undistort")
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    h.hm_ud_map.argtypes = [vp, ci, ci, vp, vp]
    h.hm_ud_map.restype = None
    h.hm_ud_taps.argtypes = [ll, vp, vp, vp]
    h.hm_ud_taps.restype = None
    h.hm_ud_frames.argtypes = [ci, ci, ci, ci, vp, vp, ci, vp]
    h.hm_ud_frames.restype = None
    return h


def shim_frames(shim, frames, cams, kind):
    frames = np.ascontiguousarray(frames)
    F, H, W = frames.shape[:3]
    C = 1 if frames.ndim == 3 else 3
    out = np.full(frames.shape, 77, np.uint8) if kind == "uint8" else np.full(frames.shape, np.nan, np.float32)
    cams = np.ascontiguousarray(cams)
    assert cams.shape == (F, 18)
    shim.hm_ud_frames(F, H, W, C, frames.ctypes.data, cams.ctypes.data, KINDS[kind], out.ctypes.data)
    return out


def shim_taps(shim, u, v):
    u, v = np.ascontiguousarray(u, np.float64).ravel(), np.ascontiguousarray(v, np.float64).ravel()
    t = np.zeros((len(u), 6), np.int32)
    shim.hm_ud_taps(len(u), u.ctypes.data, v.ctypes.data, t.ctypes.data)
    return t


# ---- the fixed cases hold what they were chosen to hold (the restatement alone) ----------------------------------------------------------
def test_fixed_cases_hold_every_class_of_pixel():
    seen = {}
    for name in R.CASES:
        K, dist, new_K = R.case(name)
        u, v = R.source_map(R.H, R.W, K, dist, new_K)
        c = seen[name] = R.classify(u, v, R.H, R.W)
        print(f"\nundistort case {name}: {c}")
        assert c["tie_margin"] >= 1e-6, (name, c)
        sx, sy, _, _, _ = R.taps(u, v)
        c["any"] = (int((sx == -1).sum()), int((sy == -1).sum()), int((sx == R.W - 1).sum()), int((sy == R.H - 1).sum()))
    assert min(c["tie_margin"] for c in seen.values()) >= 2e-5
    assert seen["zero"]["partial"] == 89 and seen["zero"]["right"] == R.H and seen["zero"]["bottom"] == R.W and seen["zero"]["outside"] == 0
    assert seen["barrel"]["partial"] == 0 and seen["barrel"]["outside"] == 0
    assert seen["pincushion"]["partial"] == 126 and seen["pincushion"]["outside"] == 265
    ps = seen["pin+shift"]
    assert -64.0 <= ps["min_source"] < -63.0 and ps["left"] == 20 and ps["any"][1:] == (31, 9, 8)
    # non-zero counts of every class among the live pixels, so that a changed constant cannot silently empty one
    for edge in ("left", "top", "right", "bottom"):
        assert sum(c[edge] for c in seen.values()) > 0 and seen["pincushion"][edge] > 0, edge
    assert ps["left"] > 0 and ps["top"] > 0 and ps["right"] > 0 and all(n > 0 for n in ps["any"])
    assert seen["pincushion"]["negative_fixed"] > 0 and ps["negative_fixed"] > 1000 and ps["outside"] > 0


# ---- the header on the host against the restatement, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_host_map_and_taps_equal_the_restatement(shim, name):
    K, dist, new_K = R.case(name)
    cam = table(K, dist, new_K)
    assert cam.shape == (1, 18) and np.array_equal(cam[0, :9], [K[0, 0], K[1, 1], K[0, 2], K[1, 2], *dist])
    assert np.array_equal(cam[0, 9:], np.linalg.inv(K if new_K is None else new_K).reshape(9))
    u, v = np.zeros((R.H, R.W)), np.zeros((R.H, R.W))
    shim.hm_ud_map(cam.ctypes.data, R.H, R.W, u.ctypes.data, v.ctypes.data)
    ru, rv = R.source_map(R.H, R.W, K, dist, new_K)
    assert np.array_equal(u.view(np.int64), ru.view(np.int64)) and np.array_equal(v.view(np.int64), rv.view(np.int64))
    t = shim_taps(shim, u, v)
    sx, sy, _, _, ws = R.taps(ru, rv)
    want = np.stack([sx.ravel(), sy.ravel()] + [w.ravel() for w in ws], axis=1)
    assert np.array_equal(t.astype(np.int64), want)
    assert np.all(t[:, 2:].sum(axis=1) == 32768)


def test_host_taps_on_ties_negatives_and_saturation(shim):
    u = np.array([1 / 64, 3 / 64, -1 / 64, -3 / 64, -1.0, -1 / 32, -33 / 32, 5.25, -0.75, 1e12, -1e12, np.nan, 2.0 ** 26, -2.0 ** 26 - 1,
                  67108863.96875, np.inf, -np.inf])
    v = np.zeros_like(u)
    t = shim_taps(shim, u, v)
    sx, sy, ax, ay, ws = R.taps(u, v)
    assert np.array_equal(t[:, 0], sx) and np.array_equal(t[:, 1], sy)
    for k in range(4):
        assert np.array_equal(t[:, 2 + k], ws[k])
    # known answers: half to even (0.5 -> 0, 1.5 -> 2, -0.5 -> -0, -1.5 -> -2), floor and rest of a negative, saturation
    iu = t[:, 0].astype(np.int64) * 32 + (32 - t[:, 2] // 1024)      # w00 = (32 - ax) 1024 at ay = 0
    assert list(iu[:9]) == [0, 2, 0, -2, -32, -1, -33, 168, -24]
    assert list(t[:9, 0]) == [0, 0, 0, -1, -1, -1, -2, 5, -1]
    assert t[9, 0] == (2 ** 31 - 1) >> 5 and t[10, 0] == -2 ** 26 and t[11, 0] == -2 ** 26 and t[15, 0] == (2 ** 31 - 1) >> 5 and t[16, 0] == -2 ** 26
    assert t[12, 0] == (2 ** 31 - 1) >> 5 and t[13, 0] == -2 ** 26 and t[14, 0] == 67108863 and t[14, 2] == 1024      # ax = 31


@pytest.mark.parametrize("channels", (1, 3))
def test_host_frames_equal_the_restatement(shim, channels):
    frames = R.frames_case(channels)
    for name in R.CASES:
        K, dist, new_K = R.case(name)
        cams = table(K, dist, new_K, R.F)
        for kind in KINDS:
            got = shim_frames(shim, frames, cams, kind)
            want = R.undistort(frames, K, dist, new_K, kind)
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, kind)
    # three frames with three coefficient sets in one call
    names = ("barrel", "pincushion", "pin+shift")
    Ks = np.stack([R.case(n)[0] for n in names])
    dists = np.stack([R.case(n)[1] for n in names])
    new_Ks = np.stack([R.K if R.case(n)[2] is None else R.case(n)[2] for n in names])
    got = shim_frames(shim, frames, table(Ks, dists, new_Ks), "uint8")
    for f, n in enumerate(names):
        assert np.array_equal(got[f], R.undistort(frames[f:f + 1], *R.case(n))[0]), n
    assert len({got[f].tobytes() for f in range(3)}) == 3


def test_unit_form_is_the_hosts_division_by_255():
    """The reference divides the uint8 stack by 255 with torch on the host: float32(value) / float32(255), correctly rounded."""
    want = (torch.arange(256, dtype=torch.uint8) / 255).numpy()
    assert np.array_equal(want, np.arange(256, dtype=np.float32) / np.float32(255))
    img = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert np.array_equal(R.undistort(img, R.K, R.COEFFS["zero"], None, "unit").ravel(), want)
    # the header forms the quotient without a division: the same float32 for every value
    shim = build_shim("undistort")
    got = np.zeros(256, np.float32)
    shim.hm_ud_unit_table(ctypes.c_void_p(got.ctypes.data))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_projective_new_matrix_takes_the_division(shim):
    """An affine new matrix (last row 0 0 1) skips the division by _w = 1; a new matrix with a perspective row must not."""
    K, dist, _ = R.case("barrel")
    new_K = K.copy()
    new_K[2] = [1e-3, -2e-3, 1.0]
    cam = table(K, dist, new_K)
    assert cam[0, 15] != 0.0 and cam[0, 16] != 0.0
    u, v = np.zeros((R.H, R.W)), np.zeros((R.H, R.W))
    shim.hm_ud_map(cam.ctypes.data, R.H, R.W, u.ctypes.data, v.ctypes.data)
    ru, rv = R.source_map(R.H, R.W, K, dist, new_K)
    assert np.array_equal(u.view(np.int64), ru.view(np.int64)) and np.array_equal(v.view(np.int64), rv.view(np.int64))
    frames = R.frames_case(3)
    assert np.array_equal(shim_frames(shim, frames, table(K, dist, new_K, R.F), "uint8"), R.undistort(frames, K, dist, new_K))


# ---- known answers that do not lean on the restatement ----------------------------------------------------------------------------------
def test_zero_distortion_is_the_identity_copy(shim):
    K, dist, _ = R.case("zero")
    for channels in (1, 3):
        frames = R.frames_case(channels)
        cams = table(K, dist, None, R.F)
        assert np.array_equal(shim_frames(shim, frames, cams, "uint8"), frames)
        assert np.array_equal(shim_frames(shim, frames, cams, "mask"), (frames > 0).astype(np.float32))
        assert np.array_equal(shim_frames(shim, frames, cams, "unit"), frames.astype(np.float32) / np.float32(255))
    u, v = np.zeros((R.H, R.W)), np.zeros((R.H, R.W))
    shim.hm_ud_map(table(K, dist).ctypes.data, R.H, R.W, u.ctypes.data, v.ctypes.data)
    t = shim_taps(shim, u, v)
    assert np.all(t[:, 2] == 32768) and np.all(t[:, 3:] == 0)      # ax = ay = 0 at every pixel
    jj, ii = np.meshgrid(np.arange(R.W), np.arange(R.H))
    assert np.array_equal(t[:, 0], jj.ravel()) and np.array_equal(t[:, 1], ii.ravel())


def test_shifted_new_matrix_is_a_shift_with_a_zero_border(shim):
    K, dist, _ = R.case("zero")
    new_K = K.copy()
    new_K[0, 2] += 3.0      # output column j reads source column j - 3
    new_K[1, 2] -= 2.0      # output row i reads source row i + 2
    for channels in (1, 3):
        frames = R.frames_case(channels)
        got = shim_frames(shim, frames, table(K, dist, new_K, R.F), "uint8")
        want = np.zeros_like(frames)
        want[:, :R.H - 2, 3:] = frames[:, 2:, :R.W - 3]
        assert np.array_equal(got, want)


def test_half_pixel_shift_of_a_two_valued_column_image(shim):
    K, dist, _ = R.case("zero")
    new_K = K.copy()
    new_K[0, 2] -= 0.5      # output column j reads source column j + 0.5
    for a, b in ((10, 21), (0, 255), (255, 254), (7, 7), (0, 1), (200, 3)):
        img = np.empty((1, R.H, R.W), np.uint8)
        img[:, :, 0::2], img[:, :, 1::2] = a, b
        got = shim_frames(shim, img, table(K, dist, new_K), "uint8")
        assert np.all(got[0, :, :R.W - 1] == (a + b + 1) >> 1), (a, b)
        last = a if (R.W - 1) % 2 == 0 else b      # the last column's right tap is the border's 0
        assert np.all(got[0, :, R.W - 1] == (last + 1) >> 1)


def ramp():
    jj, ii = np.meshgrid(np.arange(R.W), np.arange(R.H))
    img = (2 * jj + 3 * ii).astype(np.uint8)      # adjacent differences 2 and 3 levels; at most 2 * 52 + 3 * 36 = 212
    assert int((2 * jj + 3 * ii).max()) <= 255
    return img


def test_ramp_is_within_one_level_of_double_bilinear_interpolation(shim):
    """On a linear ramp with adjacent differences <= 4 levels the 1/64-px rounding of each coordinate moves the value by at most
    4 / 64 = 0.0625, both axes 0.125; the weights are exact; the final rounding adds at most 0.5: within 1 level of bilinear
    interpolation at the double position.  "barrel" keeps every tap of every pixel inside the image, so the whole frame is held to
    scipy.ndimage.map_coordinates(order=1, mode="constant").  Under "pincushion" the same holds for the pixels whose four taps are
    inside and for those fully outside (0 on both sides); a partial pixel blends with the border's 0, where scipy's mode "constant"
    does not interpolate, and is left to the restatement."""
    from scipy import ndimage
    img = ramp()
    worst = {}
    for name in ("barrel", "pincushion"):
        K, dist, new_K = R.case(name)
        got = shim_frames(shim, img[None], table(K, dist, new_K), "uint8")[0].astype(np.float64)
        u, v = R.source_map(R.H, R.W, K, dist, new_K)
        want = ndimage.map_coordinates(img.astype(np.float64), [v, u], order=1, mode="constant", cval=0.0)
        sx, sy, _, _, _ = R.taps(u, v)
        inside = (sx >= 0) & (sx + 1 < R.W) & (sy >= 0) & (sy + 1 < R.H)
        gone = (sx >= R.W) | (sx + 1 < 0) | (sy >= R.H) | (sy + 1 < 0)
        held = inside | gone
        if name == "barrel":
            assert held.all() and inside.all()
        else:
            assert gone.sum() == 265 and (~held).sum() == 126
        worst[name] = float(np.abs(got - want)[held].max())
        assert np.all(got[gone] == 0) and np.all(want[gone] == 0)
        assert worst[name] <= 1.0, worst
    print(f"\nundistort ramp: worst distance from double bilinear interpolation {worst} levels (bound 1, derived 0.625)")


# ---- optimal_new_camera_matrix ----------------------------------------------------------------------------------------------------
def test_optimal_new_camera_matrix_at_zero_distortion_returns_K():
    from bilateral_driving_amd import undistort
    for size in ((R.W, R.H), (960, 640), (1920, 1280)):
        for alpha in (1.0, 0.0, 0.3):
            M = undistort.optimal_new_camera_matrix(R.K, R.COEFFS["zero"], size, alpha)
            assert M.dtype == np.float64 and M.shape == (3, 3)
            assert np.all(np.abs(M - R.K) <= 1e-12 * np.abs(R.K).max()), (size, alpha, M)      # ((W - 1) / inner.w: W / inner.w would give fx W / (W - 1))


@pytest.mark.parametrize("coeffs", (MILD, R.COEFFS["barrel"], R.COEFFS["pincushion"]))
def test_optimal_new_camera_matrix_equals_the_restatement(coeffs):
    from bilateral_driving_amd import undistort
    for size, K in (((R.W, R.H), R.K), ((960, 640), np.array([[1030.0, 0, 481.3], [0, 1028.5, 322.9], [0, 0, 1]]))):
        for alpha in (1.0, 0.0):
            got = undistort.optimal_new_camera_matrix(torch.from_numpy(K).float(), torch.tensor(coeffs, dtype=torch.float64), size, alpha)
            want = R.optimal_new_camera_matrix(K.astype(np.float32).astype(np.float64), np.array(coeffs), size, alpha)
            nz = want != 0
            assert np.array_equal(got == 0, want == 0) and np.all(np.abs(got[nz] - want[nz]) <= 1e-12 * np.abs(want[nz])), (size, alpha)
            assert got[2, 2] == 1.0 and got[0, 1] == 0.0 and got[1, 0] == 0.0
        print(f"\noptimal matrix {coeffs} {size}: re-distortion residual {R.redistortion_residual(K, coeffs, size):.3g} px")
    with pytest.raises(ValueError):
        undistort.optimal_new_camera_matrix(np.eye(4), coeffs, (R.W, R.H))
    with pytest.raises(ValueError):
        undistort.optimal_new_camera_matrix(R.K, coeffs[:4], (R.W, R.H))


def test_outer_rectangle_shows_the_whole_source_and_inner_only_valid_pixels():
    """What alpha means, checked on the map itself: under the alpha = 1 matrix the 81 grid points of the source all land inside the
    new image (to the iteration's residual), under alpha = 0 every border pixel of the new image reads inside the source."""
    from bilateral_driving_amd import undistort
    K, dist, _ = R.case("barrel")
    M0 = undistort.optimal_new_camera_matrix(K, dist, (R.W, R.H), 0.0)
    u, v = R.source_map(R.H, R.W, K, dist, M0)
    edge = np.ones((R.H, R.W), bool)
    edge[1:-1, 1:-1] = False
    tol = 0.5      # the inner rectangle is taken from 9 points per edge, not from every pixel
    assert u[edge].min() >= -tol and u[edge].max() <= R.W - 1 + tol and v[edge].min() >= -tol and v[edge].max() <= R.H - 1 + tol
    M1 = undistort.optimal_new_camera_matrix(K, dist, (R.W, R.H), 1.0)
    pu, pv = R.grid_points(R.W, R.H)
    x, y = R.undistort_points(pu, pv, K, dist)
    nu, nv = M1[0, 0] * x + M1[0, 2], M1[1, 1] * y + M1[1, 2]
    assert nu.min() >= -1e-9 and nu.max() <= R.W - 1 + 1e-9 and nv.min() >= -1e-9 and nv.max() <= R.H - 1 + 1e-9
    assert abs(nu.min()) < 1e-9 and abs(nu.max() - (R.W - 1)) < 1e-9      # the outer rectangle is tight


# ---- resources, signature and argument validation ---------------------------------------------------------------------------------------
def test_undistort_kernel_resources():
    res = kernel_resources("undistort.hip")
    assert len(res) == 6 and all(k.startswith("undistort_kernel") for k in res), list(res)      # C in (1, 3) x three output forms
    for k, r in res.items():
        print(f"\n{k}: occupancy {r['Occupancy']} waves/SIMD, {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs")
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= 8, (k, r)
    assert "undistort.hip" in B.SOURCES


def test_entry_resolves_with_the_declared_signature():
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_undistort\w*", k)}
    assert sorted(decl) == ["bds_undistort"]
    ret, args = decl["bds_undistort"]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert ret is ci and args == [ci, ci, ci, ci, vp, vp, ci, vp, vp]
    lib = L.lib()
    assert L._SIGS["bds_undistort"] == (ret, args) and lib.bds_undistort.argtypes == args
    hdr = header()
    from bilateral_driving_amd import undistort
    for macro, value in (("BDS_UNDISTORT_UINT8", undistort.KINDS["uint8"]), ("BDS_UNDISTORT_UNIT", undistort.KINDS["unit"]),
                         ("BDS_UNDISTORT_MASK", undistort.KINDS["mask"])):
        assert f"#define {macro} {value}\n" in hdr, macro
    assert lib.bds_abi_version() == L.ABI_VERSION == 7 and "#define BDS_ABI_VERSION 7 " in hdr      # entries are only added
    full = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bds.h")).read()
    assert "pixel_source.py:249-256,273-278,296-303,319-326,342-349,366-373" in full
    assert undistort.MAX_EXTENT == 32767


def test_entry_rejects_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first

    def call(F=3, H=37, W=53, C=3, src=p, cams=p, kind=0, out=p):
        return lib.bds_undistort(F, H, W, C, src, cams, kind, out, None)
    for kw in (dict(src=None), dict(cams=None), dict(out=None), dict(F=0), dict(F=-1), dict(H=0), dict(W=0), dict(H=-5), dict(W=-5), dict(C=0),
               dict(C=2), dict(C=4), dict(C=-1), dict(kind=3), dict(kind=-1), dict(H=32768), dict(W=32768), dict(H=1 << 30), dict(cams=p + 4),
               dict(kind=1, out=p + 2), dict(kind=2, out=p + 1)):
        assert call(**kw) == L.BDS_EINVAL, kw


def test_python_checks_arguments_and_refuses_the_cpu():
    import bilateral_driving_amd
    from bilateral_driving_amd import undistort
    assert bilateral_driving_amd.undistort is undistort
    img = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)
    dist = np.zeros(5)
    with pytest.raises(L.BdsError):
        undistort.undistort_images(img, R.K, dist, device="cpu")
    with pytest.raises(L.BdsError):
        undistort.undistort_images(img.numpy(), R.K, dist, device=torch.device("cpu"))
    if not torch.cuda.is_available():
        with pytest.raises(L.BdsError):
            undistort.undistort_images(img, R.K, dist)
    for bad in (dict(src=img.float()), dict(src=torch.zeros(2, 8, 9, 2, dtype=torch.uint8)), dict(src=torch.zeros(5, dtype=torch.uint8)),
                dict(src=torch.zeros(1, 2, 8, 9, 3, dtype=torch.uint8)), dict(out="float"), dict(K=np.eye(4)), dict(dist=np.zeros(4)),
                dict(K=np.stack([R.K] * 3)), dict(dist=np.zeros((5, 5))), dict(new_K=np.zeros((3, 3))), dict(new_K=np.stack([R.K] * 3)),
                dict(src=torch.zeros(2, 0, 9, 3, dtype=torch.uint8))):
        kw = dict(src=img, K=R.K, dist=dist, new_K=None, out="uint8", device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            undistort.undistort_images(kw.pop("src"), kw.pop("K"), kw.pop("dist"), **kw)
    t = undistort.camera_table(torch.from_numpy(R.K).float(), torch.zeros(4, 5), None, 4)
    assert t.shape == (4, 18) and t.dtype == np.float64 and np.array_equal(t[0], t[3])
    assert undistort.STAGE_BYTES == 256 << 20


# ---- the seam ---------------------------------------------------------------------------------------------------------------------------
def test_install_and_uninstall_restore_the_classes_exactly():
    from bilateral_driving_amd import lidar, undistort

    class CameraData:
        def load_images(self):
            return "former"

        def load_sky_masks(self):
            return "former sky"

    class Base:
        def project_lidar_pts_on_images(self):
            return "base"

    class DrivingDataset(Base):
        pass

    cam_before, ds_before = dict(CameraData.__dict__), dict(DrivingDataset.__dict__)
    lidar.install(DrivingDataset)
    after_lidar = dict(DrivingDataset.__dict__)
    assert DrivingDataset.__dict__["project_lidar_pts_on_images"] is lidar.project_lidar_pts_on_images
    undistort.install(CameraData, DrivingDataset)      # (after lidar.install: the documented order)
    undistort.install(CameraData)                      # (twice: the former methods are still the ones remembered)
    for name in ("load_images", "load_egocar_mask", "load_dynamic_masks", "load_sky_masks"):
        assert CameraData.__dict__[name] is getattr(undistort, name)
    assert DrivingDataset.__dict__["project_lidar_pts_on_images"] is undistort.project_lidar_pts_on_images
    undistort.uninstall()
    assert dict(CameraData.__dict__) == cam_before and dict(DrivingDataset.__dict__) == after_lidar
    assert "load_egocar_mask" not in CameraData.__dict__ and CameraData().load_images() == "former"
    lidar.uninstall(DrivingDataset)
    assert dict(DrivingDataset.__dict__) == ds_before and DrivingDataset().project_lidar_pts_on_images() == "base"
    undistort.install(None, DrivingDataset)
    undistort.uninstall(DrivingDataset)
    assert dict(DrivingDataset.__dict__) == ds_before


def undistort_dataset(device):
    """tests.lidar_ref64's bare dataset with camera 1 set to ``undistort`` and mild per-frame coefficients"""
    pc = LR.golden_projection_case("shared")
    d = LR.bare_projection_dataset(pc, device)
    for c, cam in d.pixel_source.camera_data.items():
        cam.distortions = torch.tensor([[-0.05 + 0.01 * f, 0.01, 0.001, -0.0005 * (c + 1), 0.0] for f in range(len(cam))])
    d.pixel_source.camera_data[1].undistort = True
    return pc, d


def restated_matrices(cam):
    """``pad(new K) @ inverse(c2w)`` in float32, the new K from the restatement"""
    out = []
    for f in range(len(cam)):
        K = cam.intrinsics[f].cpu().numpy().astype(np.float64)
        M = R.optimal_new_camera_matrix(K, cam.distortions[f].cpu().numpy().astype(np.float64), (cam.WIDTH, cam.HEIGHT), 1.0)
        K4 = np.zeros((4, 4), np.float32)
        K4[:3, :3] = M.astype(np.float32)
        K4[3, 3] = 1.0
        out.append(torch.from_numpy(K4) @ cam.cam_to_worlds[f].cpu().float().inverse())
    return torch.stack(out)


def test_an_undistort_camera_is_served_and_lidar_keeps_refusing_it():
    from bilateral_driving_amd import lidar, undistort
    pc, d = undistort_dataset("cpu")
    with pytest.raises(NotImplementedError, match="undistort.install"):
        lidar.project_lidar_pts_on_images(d)
    cams = d.pixel_source.camera_data
    # a camera without ``undistort`` takes lidar's own matrices, one with it the optimal new matrix of every frame
    assert torch.equal(undistort.camera_matrices(cams[0]), lidar.camera_matrices(cams[0]))
    got, want = undistort.camera_matrices(cams[1]), restated_matrices(cams[1])
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(cams[1]), 4, 4)
    assert torch.allclose(got, want, rtol=1e-6, atol=0) or float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())
    assert not torch.equal(got, lidar.camera_matrices(cams[1])) and not torch.equal(got[0], got[1])      # per frame
    # the method gets past the refusal: on a host without a GPU it ends at the product's "no CPU path", nowhere earlier
    if not torch.cuda.is_available():
        with pytest.raises(L.BdsError):
            undistort.project_lidar_pts_on_images(d)


def test_loaders_refuse_a_cpu_camera(tmp_path):
    from bilateral_driving_amd import undistort
    cam = R.BareLoaderCamera(R.write_camera_files(tmp_path), torch.device("cpu"), True)
    for name in ("load_images", "load_dynamic_masks", "load_sky_masks"):
        with pytest.raises(L.BdsError):
            getattr(undistort, name)(cam)
    undistort.load_egocar_mask(cam)      # no file for this camera: None, as the reference
    assert cam.egocar_mask is None
