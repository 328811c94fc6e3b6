"""Evaluation image metrics (bilateral_driving_amd/metrics.py, csrc/metrics.hip) on the CPU: the float64 restatement
(tests/metrics_ref64.py) against known answers, the device math on the host (tests/hostmath_metrics_shim.hip) against that restatement
element by element, the new kernels' resources, and the C entries' signatures and argument checks.

The shim's map is held to twice the float32 restatement's own worst element error against float64 plus 1e-6 (metrics_ref64.bound).
Measured over the 21 cases (printed by the test): the float32 restatement's worst element error is 1.2e-4 (an image flat to 1e-3:
uxx - ux ux cancels), the shim's 3.0e-8 everywhere -- it takes the window sums in double and rounds S once."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from tests import metrics_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources

C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- the restatement against known answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identical_images_score_one_and_infinity(dtype):
    pred, _ = R.make_images(17, 23, "noise")
    f = R.frame(pred, pred, {"all": np.ones((17, 23), bool)}, dtype)
    assert f["ssim"] == 1.0 and f["all_ssim"] == 1.0 and np.all(f["ssim_map"] == 1.0)
    assert f["psnr"] == math.inf and f["all_psnr"] == math.inf


@pytest.mark.parametrize("c,d", [(0.5, 0.1), (0.25, -0.2), (0.0, 1.0)])
def test_constant_offset_on_a_constant_image_has_the_closed_form(c, d):
    gt = np.full((9, 12, 3), c, np.float64)
    pred = gt + d
    f = R.frame(pred, gt, {}, np.float64)
    S = (2 * c * (c + d) + C1) / (c * c + (c + d) ** 2 + C1)          # zero variances: the second factor is C2 / C2
    assert abs(f["ssim"] - S) < 1e-12 and np.abs(f["ssim_map"] - S).max() < 1e-12
    assert abs(f["psnr"] - -20 * math.log10(abs(d))) < 1e-9


def test_reflect_is_scipys_and_the_mean_is_cropped():
    x = np.arange(7.0)
    got = R.uniform_filter(x, size=7)           # d c b a | a b c d | d c b a
    assert abs(got[0] - (x[[2, 1, 0, 0, 1, 2, 3]].sum() / 7)) < 1e-12 and abs(got[6] - (x[[3, 4, 5, 6, 6, 5, 4]].sum() / 7)) < 1e-12
    pred, gt = R.make_images(7, 7, "noise")
    f = R.frame(pred, gt, {}, np.float64)
    assert abs(f["ssim"] - f["ssim_map"][3, 3].mean()) < 1e-15      # the cropped region of a 7x7 image is one pixel


def test_masked_values_are_the_uncropped_mean_and_the_mask_psnr():
    pred, gt, masks, r64, _ = R.case(17, 23, "noise")
    S, occ = r64["ssim_map"], ~masks["sky_masks"]
    assert abs(r64["occupied_ssim"] - S[occ].mean()) < 1e-15 and abs(r64["masked_ssim"] - S[masks["dynamic_masks"]].mean()) < 1e-15
    d = pred.astype(np.float64)[occ] - gt.astype(np.float64)[occ]
    assert abs(r64["occupied_psnr"] - -10 * math.log10((d * d).mean())) < 1e-9
    assert "x_ssim" not in R.frame(pred, gt, {"x": np.zeros((17, 23), bool)}, np.float64)      # an empty mask gives no entry


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("metrics")
    h.hm_metrics_map.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    h.hm_metrics_reflect.argtypes = [ctypes.c_int] * 2
    h.hm_metrics_psnr.argtypes = [ctypes.c_double] * 2
    h.hm_metrics_psnr.restype = ctypes.c_double
    return h


def test_host_reflect_and_psnr(shim):
    for n in (7, 8, 23):
        pad = np.pad(np.arange(n), (n, n), mode="symmetric")       # numpy's "symmetric" is scipy's "reflect"
        assert [shim.hm_metrics_reflect(i, n) for i in range(-n, 2 * n)] == pad.tolist()
        assert shim.hm_metrics_reflect(-n - 5, n) in range(n) and shim.hm_metrics_reflect(2 * n + 5, n) in range(n)   # clamped, in bounds
    assert shim.hm_metrics_psnr(0.0, 12.0) == math.inf and abs(shim.hm_metrics_psnr(0.12, 12.0) - 20.0) < 1e-12


def test_host_math_map_matches_float64_everywhere(shim):
    worst = (0.0, 0.0, 0.0)
    for H, W in R.SHAPES:
        for kind in R.KINDS:
            pred, gt, _, r64, r32 = R.case(H, W, kind)
            got = np.zeros((H, W, 3), np.float32)
            shim.hm_metrics_map(H, W, pred.ctypes.data, gt.ctypes.data, got.ctypes.data)
            bound, e32 = R.bound(r64, r32, "ssim_map")
            err = float(np.abs(got.astype(np.float64) - r64["ssim_map"]).max())       # border rows and columns included
            print(f"\nmetrics shim {H}x{W} {kind}: float32 restatement {e32:.3e}, bound {bound:.3e}, shim {err:.3e}")
            assert err <= bound, (H, W, kind, err, bound)
            worst = max(worst, (err / bound, err, e32))
    print(f"\nmetrics shim worst ratio to the bound {worst[0]:.3f} (error {worst[1]:.3e}, float32 restatement {worst[2]:.3e})")


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_metrics_kernel_resources():
    res = kernel_resources("metrics.hip")
    for prefix in ("metrics_tile_kernel", "metrics_reduce_kernel"):
        ks = [k for k in res if k.startswith(prefix)]
        assert len(ks) == 1, (prefix, list(res))
        assert res[ks[0]]["ScratchSize"] == 0, (ks[0], res[ks[0]])
        assert 0 < res[ks[0]]["LDS Size"] <= 64 * 1024, (ks[0], res[ks[0]])       # the static limit of a workgroup
        assert res[ks[0]]["Occupancy"] >= 4, (ks[0], res[ks[0]])


def test_entries_resolve_with_the_declared_signatures():
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_image_metrics\w*", k)}
    assert sorted(decl) == ["bds_image_metrics", "bds_image_metrics_workspace_bytes"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    assert "BDS_IMAGE_METRICS_ROW 14" in hdr
    from bilateral_driving_amd import metrics
    assert metrics.ROW == 14 and lib.bds_abi_version() == L.ABI_VERSION == 7


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first

    def run(H=17, W=23, pred=p, gt=p, masks=(None,) * 4, inv=0, kind=0, out=p, ws=p, nb=1 << 30):
        return lib.bds_image_metrics(H, W, pred, gt, *masks, inv, kind, None, out, ws, nb, None)

    for H, W in ((6, 23), (17, 6), (0, 0), (-1, 23), (17, (1 << 19) + 1)):
        assert run(H=H, W=W) == L.BDS_EINVAL and lib.bds_image_metrics_workspace_bytes(H, W) == 0, (H, W)
    assert run(pred=None) == L.BDS_EINVAL and run(gt=None) == L.BDS_EINVAL and run(out=None) == L.BDS_EINVAL
    assert run(out=p + 4) == L.BDS_EINVAL and run(ws=None) == L.BDS_EINVAL and run(ws=p + 8) == L.BDS_EINVAL
    assert run(kind=2) == L.BDS_EINVAL and run(inv=16) == L.BDS_EINVAL and run(inv=-1) == L.BDS_EINVAL
    assert run(inv=1) == L.BDS_EINVAL                                       # an invert bit on an unused slot
    assert run(masks=(p + 1, None, None, None), kind=1) == L.BDS_EINVAL      # a misaligned float mask
    need = lib.bds_image_metrics_workspace_bytes(17, 23)
    assert need >= 2 * 2 * 16 * 8 and run(nb=need - 1) == L.BDS_EWORKSPACE
    assert lib.bds_image_metrics_workspace_bytes(1080, 1920) >= 68 * 120 * 16 * 8


def test_python_checks_shapes_and_refuses_cpu_tensors():
    from bilateral_driving_amd import metrics
    img = torch.rand(17, 23, 3)
    with pytest.raises(L.BdsError):
        metrics.image_metrics(img, img)
    with pytest.raises(L.BdsError):
        metrics.compute_psnr(img, img)
    with pytest.raises(L.BdsError):
        metrics.frame_metrics(img, {"pixels": img})
    for bad in (torch.rand(6, 23, 3), torch.rand(17, 6, 3)):
        with pytest.raises(ValueError):
            metrics.image_metrics(bad, bad)
    with pytest.raises(ValueError):
        metrics.image_metrics(torch.rand(17, 23, 4), torch.rand(17, 23, 4))
    with pytest.raises(ValueError):
        metrics.image_metrics(img, torch.rand(17, 24, 3))
    with pytest.raises(ValueError):
        metrics.image_metrics(img, img, {"m": torch.ones(17, 24)})
    import bilateral_driving_amd
    assert bilateral_driving_amd.metrics is metrics
