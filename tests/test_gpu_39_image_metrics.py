"""Evaluation image metrics on the MI355X (csrc/metrics.hip through bilateral_driving_amd/metrics.py) against the float64 restatement of
the reference's frame scoring (tests/metrics_ref64.py: scipy's uniform_filter, the filter skimage calls, and torch's compute_psnr).

Shapes are chosen where the kernel can go wrong: 7x7 (every pixel reflects on all sides, the cropped region is one pixel), 7x40 and
40x7 (the minimum extent one way), 16x16 (exactly one tile), 17x23 (partial tiles both ways), 33x19 (one pixel past a tile boundary),
64x96 (several whole tiles); images are uniform noise plus Gaussian error, a smooth sinusoid plus small error, and an image flat to
1e-3 (where uxx - ux ux cancels in float32).  The bound is not fixed: per case and per value the float32 restatement's own distance
from float64 is measured, and the kernel is held to twice that plus 1e-6 (PSNR in dB) -- metrics_ref64.bound."""
import math

import numpy as np
import pytest
import torch

from tests import metrics_ref64 as R

pytestmark = pytest.mark.gpu

PREFIX = {"sky_masks": "occupied", "dynamic_masks": "masked", "human_masks": "human", "vehicle_masks": "vehicle"}
SCALARS = ("psnr", "ssim") + tuple(f"{p}_{m}" for p in PREFIX.values() for m in ("psnr", "ssim"))


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import metrics
    return metrics


def dev(a):
    return torch.as_tensor(a).cuda()


def infos(gt, masks, as_type=torch.float32):
    return {"pixels": dev(gt), **{k: dev(v).to(as_type) for k, v in masks.items()}}


# ---- the map and the ten scalars ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_map_and_scalars_match_float64_within_the_float32_restatements_error(M, H, W, kind):
    pred, gt, masks, r64, r32 = R.case(H, W, kind)
    named = {PREFIX[k]: dev(v) for k, v in masks.items()}
    got = M.image_metrics(dev(pred), dev(gt), named, return_map=True, invert=("occupied",))
    smap = got["ssim_map"]
    assert smap.shape == (H, W, 3) and smap.dtype == torch.float32 and got["psnr"].dtype == torch.float64 and got["psnr"].is_cuda
    bound, e32 = R.bound(r64, r32, "ssim_map")
    err = float(np.abs(smap.cpu().numpy().astype(np.float64) - r64["ssim_map"]).max())      # border rows and columns included
    print(f"\nimage metrics {H}x{W} {kind}: map float32 restatement {e32:.3e}, bound {bound:.3e}, kernel {err:.3e}")
    assert err <= bound, ("ssim_map", err, bound)
    for p in PREFIX.values():
        assert float(got[f"{p}_valid"]) == 1.0
    for k in SCALARS:
        bound, e32 = R.bound(r64, r32, k)
        err = abs(float(got[k]) - r64[k])
        print(f"image metrics {H}x{W} {kind}: {k} float32 restatement {e32:.3e}, bound {bound:.3e}, kernel {err:.3e}")
        assert err <= bound, (k, float(got[k]), r64[k], bound)
    # the frame form under the reference's key names, and its PSNR entry point, give the same values
    fm = M.frame_metrics(dev(pred), infos(gt, masks))
    assert sorted(fm) == sorted(SCALARS) and all(fm[k] == float(got[k]) for k in SCALARS)
    assert abs(M.compute_psnr(dev(pred), dev(gt)) - r64["psnr"]) <= R.bound(r64, r32, "psnr")[0]


def test_identical_images_and_a_constant_offset(M):
    pred, _ = R.make_images(17, 23, "noise")
    got = M.image_metrics(dev(pred), dev(pred), {"all": torch.ones(17, 23, dtype=torch.bool, device="cuda")}, return_map=True)
    assert float(got["psnr"]) == math.inf and float(got["all_psnr"]) == math.inf
    assert float(got["ssim"]) == 1.0 and float(got["all_ssim"]) == 1.0 and bool((got["ssim_map"] == 1.0).all())
    c, d = 0.5, 0.125        # (exact in float32)
    gt = torch.full((9, 12, 3), c, device="cuda")
    got = M.image_metrics(gt + d, gt)
    S = (2 * c * (c + d) + 1e-4) / (c * c + (c + d) ** 2 + 1e-4)
    assert abs(float(got["ssim"]) - S) <= 1e-6 and abs(float(got["psnr"]) - -20 * math.log10(d)) <= 1e-9
    assert abs(M.compute_psnr(gt + d, gt) - -20 * math.log10(d)) <= 1e-9
    assert abs(M.compute_psnr((gt + d)[:2, :5], gt[:2, :5]) - -20 * math.log10(d)) <= 1e-9      # any shape, as image[mask]


# ---- masks --------------------------------------------------------------------------------------------------------------------------
def rows_equal(a, b):
    return all(torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)) for k in a if k != "ssim_map") and a.keys() == b.keys()


def test_mask_element_types_give_the_same_bits(M):
    pred, gt, masks, _, _ = R.case(33, 19, "noise")
    p, g = dev(pred), dev(gt)
    named = {PREFIX[k]: dev(v) for k, v in masks.items()}
    as_bool = M.image_metrics(p, g, named)
    as_u8 = M.image_metrics(p, g, {k: v.to(torch.uint8) * 3 for k, v in named.items()})          # non-zero = true
    as_f32 = M.image_metrics(p, g, {k: v.float() for k, v in named.items()})
    mixed = M.image_metrics(p, g, {k: (v.float() if i % 2 else v.double()) for i, (k, v) in enumerate(named.items())})
    assert rows_equal(as_bool, as_u8) and rows_equal(as_bool, as_f32) and rows_equal(as_bool, mixed)


def test_inverted_slot_equals_the_explicit_complement(M):
    pred, gt, masks, _, _ = R.case(33, 19, "smooth")
    p, g, sky = dev(pred), dev(gt), dev(masks["sky_masks"])
    for cast in (lambda t: t, lambda t: t.float()):
        a = M.image_metrics(p, g, {"occupied": cast(sky)}, invert=("occupied",))
        b = M.image_metrics(p, g, {"occupied": cast(~sky)})
        assert rows_equal(a, b)


def test_full_single_border_and_empty_masks(M):
    H, W = 17, 23
    pred, gt, _, r64, r32 = R.case(H, W, "noise")
    p, g = dev(pred), dev(gt)
    full = np.ones((H, W), bool)
    one = np.zeros((H, W), bool)
    one[5, 17] = True
    border = np.zeros((H, W), bool)
    border[0, 0] = border[2, 10] = border[H - 1, W - 3] = border[8, W - 1] = True       # all within the 3-pixel border
    named = {"full": full, "one": one, "border": border, "none": np.zeros((H, W), bool)}
    got = M.image_metrics(p, g, {k: dev(v) for k, v in named.items()}, return_map=True)
    f64, f32 = R.frame(pred, gt, named, np.float64), R.frame(pred, gt, named, np.float32)
    for k in ("full", "one", "border"):
        assert float(got[f"{k}_valid"]) == 1.0
        for m in ("psnr", "ssim"):
            assert abs(float(got[f"{k}_{m}"]) - f64[f"{k}_{m}"]) <= R.bound(f64, f32, f"{k}_{m}")[0], (k, m)
    # all true: the masked PSNR is the full PSNR, and the masked SSIM is the UNCROPPED map mean, not the cropped ssim
    assert abs(float(got["full_psnr"]) - float(got["psnr"])) <= 1e-9
    smap = got["ssim_map"].double()
    assert abs(float(got["full_ssim"]) - float(smap.mean())) <= 1e-12
    assert abs(float(got["ssim"]) - float(smap[3:-3, 3:-3].mean())) <= 1e-12
    assert abs(float(got["full_ssim"]) - float(got["ssim"])) > 1e-4
    assert abs(float(got["one_ssim"]) - float(smap[5, 17].mean())) <= 1e-12
    # all false: the flag is 0, the values are NaN, frame_metrics omits the keys
    assert float(got["none_valid"]) == 0.0 and math.isnan(float(got["none_psnr"])) and math.isnan(float(got["none_ssim"]))
    fm = M.frame_metrics(p, {"pixels": g, "human_masks": dev(named["none"]), "vehicle_masks": dev(one).float()})
    assert sorted(fm) == ["psnr", "ssim", "vehicle_psnr", "vehicle_ssim"]
    assert M.frame_metrics(p, {"pixels": g, "sky_masks": dev(full)}).keys() == {"psnr", "ssim"}        # all sky: nothing occupied
    # get_numpy's squeeze: [1,H,W,3] renders and [H,W,1] masks
    fs = M.frame_metrics(p[None], {"pixels": g[None], "vehicle_masks": dev(one).float()[..., None]})
    assert fs == {k: fm[k] for k in fs}


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 96), (270, 480)])
def test_two_calls_give_bit_equal_outputs(M, H, W):
    pred, gt = R.make_images(H, W, "noise", seed=3)
    masks = {PREFIX[k]: dev(v) for k, v in R.make_masks(H, W, seed=3).items()}
    p, g = dev(pred), dev(gt)
    a = M.image_metrics(p, g, masks, return_map=True, invert=("occupied",))
    b = M.image_metrics(p, g, masks, return_map=True, invert=("occupied",))
    assert rows_equal(a, b) and torch.equal(a["ssim_map"], b["ssim_map"])
    assert all(math.isfinite(float(a[k])) for k in SCALARS)


# ---- the accumulator ---------------------------------------------------------------------------------------------------------------------
def test_accumulator_means_leave_out_empty_frames(M):
    H, W, F = 17, 23, 5
    acc = M.MetricAccumulator(F)
    per_frame = []
    for i in range(F):
        pred, gt = R.make_images(H, W, ("noise", "smooth")[i % 2], seed=10 + i)
        masks = R.make_masks(H, W, seed=10 + i)
        del masks["vehicle_masks"]                          # a key absent from every frame
        masks["dynamic_masks"][:] = False                   # a key empty on every frame
        if i == 2:
            masks["human_masks"][:] = False                 # one frame without humans
        acc.add(dev(pred), infos(gt, masks, torch.float32 if i % 2 else torch.bool))
        per_frame.append((R.reference_frame(pred, gt, masks, np.float64), R.reference_frame(pred, gt, masks, np.float32)))
    assert len(acc) == F
    res = acc.results()
    assert sorted(res) == sorted(SCALARS)
    assert res["masked_psnr"] == -1 and res["masked_ssim"] == -1 and res["vehicle_psnr"] == -1 and res["vehicle_ssim"] == -1
    for k in ("psnr", "ssim", "occupied_psnr", "occupied_ssim", "human_psnr", "human_ssim"):
        v64 = [f64[k] for f64, _ in per_frame if k in f64]
        v32 = [f32[k] for _, f32 in per_frame if k in f32]
        assert len(v64) == (4 if k.startswith("human") else 5)
        bound = 2 * abs(R.non_zero_mean(v32) - R.non_zero_mean(v64)) + R.FLOOR
        assert abs(res[k] - R.non_zero_mean(v64)) <= bound, (k, res[k], R.non_zero_mean(v64), bound)
    frames = acc.per_frame()
    assert "human_psnr" not in frames[2] and "human_psnr" in frames[1]
    with pytest.raises(IndexError):
        acc.add(dev(pred), infos(gt, masks))
    assert M.MetricAccumulator(3).results() == {k: -1 for k in SCALARS}


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors(M):
    from bilateral_driving_amd import _lib as L
    img = torch.rand(17, 23, 3, device="cuda")
    for bad in (torch.rand(6, 23, 3, device="cuda"), torch.rand(17, 6, 3, device="cuda")):
        with pytest.raises(ValueError):
            M.image_metrics(bad, bad)
        with pytest.raises(ValueError):
            M.frame_metrics(bad, {"pixels": bad})
    with pytest.raises(ValueError):
        M.image_metrics(torch.rand(17, 23, 4, device="cuda"), torch.rand(17, 23, 4, device="cuda"))
    with pytest.raises(ValueError):
        M.image_metrics(img, torch.rand(17, 24, 3, device="cuda"))
    with pytest.raises(ValueError):
        M.image_metrics(img, img, {"m": torch.ones(23, 17, device="cuda")})
    with pytest.raises(ValueError):
        M.image_metrics(img, img, {str(i): torch.ones(17, 23, device="cuda") for i in range(5)})
    with pytest.raises(L.BdsError):
        M.image_metrics(img.cpu(), img.cpu())
    with pytest.raises(L.BdsError):
        M.image_metrics(img, img, {"m": torch.ones(17, 23)})
    ws = torch.empty(16, dtype=torch.uint8, device="cuda")
    row = torch.empty(14, dtype=torch.float64, device="cuda")
    assert L.lib().bds_image_metrics(6, 23, L.ptr(img), L.ptr(img), None, None, None, None, 0, 0, None, L.ptr(row), L.ptr(ws), 16,
                                     L.stream()) == L.BDS_EINVAL
    assert L.lib().bds_image_metrics(17, 23, L.ptr(img), L.ptr(img), None, None, None, None, 0, 0, None, L.ptr(row), L.ptr(ws), 16,
                                     L.stream()) == L.BDS_EWORKSPACE
