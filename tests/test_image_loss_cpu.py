"""The fused image loss (bilateral_driving_amd/losses.py ``image_terms`` / ``install``, the image-loss section of csrc/loss.hip) on the
CPU: the float64 restatement (tests/image_loss_ref64.py) against float64 autograd of the framework expressions and against the golden
the reference's own DepthLoss / binary_cross_entropy / safe_binary_cross_entropy produced (scripts/gen_golden_image_loss.py); the device
math on the host (tests/hostmath_image_loss_shim.hip) against the restatement, which is where the GPU test's FLOOR is measured; the
exact SafeBCE and depth cases; the C entries' argument checks; and the install seam on a stand-in with BasicTrainer's layout.

Measured here (printed by the tests; error = largest difference over the tensor's largest reference magnitude): over the GPU test's
cases the host shim against float64 is at most 5.98e-7 (the entropy and the sky terms: sums of float32 logarithms; the gradients stay
below 3e-7), so FLOOR = 6.0e-7; the float32 framework expression's own error on the same cases is at most 2.1e-7.  Against the
reference-generated golden (the reference's float32 run) the float32 framework expression is bit-equal (the same operations) and the
float64 restatement is within 1.9e-7 of the tensor's largest entry; both are held to 5e-7, four float32 epsilons."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import losses
from tests import image_loss_ref64 as R
from tests.util import build_shim, declared_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "image_loss.npz")
CASES = R.gpu_cases()
KINDS = {None: 0, "bce": 1, "safe_bce": 2}
TYPES = {"l1": 0, "l2": 1, "smooth_l1": 2}
REDUCTIONS = {"mean_on_hit": 0, "mean_on_hw": 1, "sum": 2}


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_ref64_matches_float64_autograd_and_the_inputs_keep_off_the_kinks(case):
    H, W, seed, o = CASES[case]
    d = R.make(H, W, seed)
    e = R.errors(R.ref(d, o), R.run(d, o))
    assert max(e.values()) <= 1e-12, e
    if o["depth"] is not None:
        n = int(R.depth_set(d, o)[0].sum())
        assert n >= 16 or H * W < 256, n                     # (the one-row, one-column and one-pixel shapes cannot hold 16 returns)
        assert R.kink_margin(d, o) >= 1e-3, R.kink_margin(d, o)
        lidar = d["lidar"][d["lidar"] > 0]
        assert H * W < 1000 or ((lidar <= 0.01).any() and (lidar >= 80).any() and 0.2 < len(lidar) / (H * W) < 0.4)
    a = (d["rgb"] - d["pixels"]).abs()
    assert a.min() >= 1e-3 and (d["dyn"] - 0.2).abs().min() >= 1e-3 and ((d["opacity"] - 0.1).abs().min() >= 1e-3) and ((d["opacity"] - 0.9).abs().min() >= 1e-3)
    e32 = R.errors(R.run(d, o, dtype=torch.float32), R.ref(d, o))
    assert R.within(e32, R.bounds(e32)) and max(e32.values()) < 1e-5, e32      # the reference alone meets the bound


def _close(got, ref, name):
    # the golden is the reference's own float32 run: 5e-7 of the tensor's largest entry (measured: 0 and 1.9e-7, see the docstring)
    np.testing.assert_allclose(got, ref, rtol=0, atol=5e-7 * max(float(np.abs(ref).max()), 1e-30), err_msg=name)


def _golden_terms():
    """[(name, options with that one term on, index of the term, gradient name, golden value, golden gradient)]"""
    z = np.load(GOLD)
    d = {k: torch.from_numpy(z[k]) for k in ("rgb", "pixels", "opacity", "depth", "sky", "lidar", "ego")}
    d["dyn"] = torch.zeros_like(d["opacity"])
    off = dict(mask=None, depth=None, entropy=False, smoothness=False, dyn=False)
    out = [("rgb", R.options(**off), 0, "rgb", z["rgb_value"], z["rgb_grad"])]
    for kind in ("bce", "safe_bce"):
        out.append(("mask " + kind, R.options(**dict(off, mask=kind)), 1, "opacity", z[f"mask_{kind}_value"], z[f"mask_{kind}_grad"]))
    cases = [str(c).split(",") for c in z["depth_cases"]]
    assert [(t, bool(int(n)), bool(int(i))) for t, n, i, r in cases[:12]] == R.DEPTH_FORMS and [c[3] for c in cases] == ["mean_on_hit"] * 12 + ["mean_on_hw", "sum"]
    for k, (t, n, i, r) in enumerate(cases):
        out.append((f"depth {t} {n} {i} {r}", R.options(**dict(off, depth=(t, bool(int(n)), bool(int(i))), reduction=r)), 2, "depth",
                    z[f"depth_{k}_value"], z[f"depth_{k}_grad"]))
    return d, out


def test_ref64_and_the_float32_expression_match_the_reference_golden():
    d, entries = _golden_terms()
    assert d["rgb"].shape == (24, 40, 3) and d["ego"].any() and len(entries) == 17
    worst = worst64 = 0.0
    for name, o, k, g, value, grad in entries:
        terms, grads = R.ref(d, o)
        t32, g32 = R.run(d, o, dtype=torch.float32)
        worst = max(worst, R.err(t32[k], value), R.err(g32[g], grad))
        worst64 = max(worst64, R.err(value, terms[k]), R.err(grad, grads[g]))
        for got_t, got_g in ((terms, grads), (t32, g32)):
            _close(got_t[k], value, name)
            _close(got_g[g], grad, name + " gradient")
    print(f"\nimage loss: float32 expression against the golden, worst {worst:.3e}; the float64 restatement {worst64:.3e}")


# ---- the device math on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("image_loss")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    head = [ci, ci] + [vp] * 8 + [ci, ctypes.c_double, ci, ci, ci, cf, ci, ci, ci, cf, vp]
    h.hm_image_loss_fwd.argtypes = head + [vp, vp]
    h.hm_image_loss_bwd.argtypes = head + [vp] * 5
    h.hm_image_loss_fwd.restype = h.hm_image_loss_bwd.restype = None
    return h


def shim_run(h, d, o, v6=R.V6, w6=R.W6):
    """The host shim on inputs ``d`` under options ``o`` -> (terms, grads) in ``R.run``'s layout (a gradient no term reaches: zeros)."""
    a = {k: np.ascontiguousarray(v.numpy(), np.float32) for k, v in d.items()}
    H, W = a["sky"].shape
    p = lambda k, on=True: a[k].ctypes.data if on else None
    need_o, need_d = o["mask"] is not None or o["entropy"], o["depth"] is not None or o["smoothness"]
    t, n, i = o["depth"] or ("l1", False, False)
    w, v = np.array(w6, np.float32), np.array(v6, np.float32)
    head = (H, W, p("rgb"), p("pixels"), p("opacity", need_o), p("depth", need_d), p("sky", o["mask"] is not None), p("lidar", o["depth"] is not None),
            p("ego", o["ego"]), p("dyn", o["dyn"]), KINDS[o["mask"]], o["limit"], TYPES[t], int(n), int(i), o["max_depth"], REDUCTIONS[o["reduction"]],
            int(o["entropy"]), int(o["smoothness"]), o["threshold"], w.ctypes.data)
    terms, sums = np.zeros(6, np.float32), np.zeros(9, np.float32)
    h.hm_image_loss_fwd(*head, terms.ctypes.data, sums.ctypes.data)
    g = {k: np.full_like(a[k], np.nan) for k in R.GRADS}
    h.hm_image_loss_bwd(*head, sums.ctypes.data, v.ctypes.data, g["rgb"].ctypes.data, g["opacity"].ctypes.data if need_o else None,
                        g["depth"].ctypes.data if need_d else None)
    if not need_o:
        g["opacity"][:] = 0
    if not need_d:
        g["depth"][:] = 0
    return terms, g


@pytest.mark.parametrize("case", list(CASES))
def test_host_math_matches_float64_within_the_floor(shim, case):
    H, W, seed, o = CASES[case]
    d = R.make(H, W, seed)
    ref = R.ref(d, o)
    e32 = R.errors(R.run(d, o, dtype=torch.float32), ref)
    e = R.errors(shim_run(shim, d, o), ref)
    print(f"\nimage loss shim {case}: float32 framework vs float64 {max(e32.values()):.3e}, shim {max(e.values()):.3e} ({max(e, key=e.get)})")
    assert max(e.values()) <= R.FLOOR, e


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
def _tiny(n, **kw):
    """A 1 x n view of plain values, every entry overridable."""
    d = dict(rgb=torch.full((1, n, 3), 0.5), pixels=torch.full((1, n, 3), 0.25), opacity=torch.full((1, n, 1), 0.5), depth=torch.full((1, n, 1), 10.0),
             sky=torch.zeros(1, n), lidar=torch.full((1, n), 12.0), ego=torch.zeros(1, n), dyn=torch.zeros(1, n, 1))
    for k, v in kw.items():
        d[k] = torch.tensor(v, dtype=torch.float32).reshape(d[k].shape)
    return d


ONLY = dict(mask=None, depth=None, entropy=False, smoothness=False, dyn=False, ego=False)


def test_safe_bce_exact_cases(shim):
    x = [0.0, 1.0, 1.000001, -1e-7, 0.95, 0.999, 0.05, 0.5]
    sky = [1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0]            # y = 1 - sky: 0, 1, 0, 1, 0, 0, 1, 1
    d = _tiny(8, opacity=x, sky=sky)
    o = R.options(**dict(ONLY, mask="safe_bce"))
    terms, g = shim_run(shim, d, o)
    t32, g32 = R.run(d, o, dtype=torch.float32)
    got, want = g["opacity"].reshape(-1), g32["opacity"].reshape(-1)
    k = R.V6[1] * R.W6[1] / 8
    assert got[0] == 0 and got[1] == 0                                               # x == y exactly: no gradient
    assert got[2] != 0 and got[3] != 0                                               # beyond the forward's clip: the gradient is present
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=0)                         # ... and the reference expression's
    np.testing.assert_allclose(got[2], k / 0.1, rtol=2e-6)                           # y = 0, x clipped to 1, then to 1 - limit: 1 / limit
    np.testing.assert_allclose(got[3], -k / 0.1, rtol=2e-6)                          # y = 1, x clipped to 0, then to limit: -1 / limit
    np.testing.assert_allclose(got[4:6], k / 0.1, rtol=2e-6)                         # y = 0, 1 - limit < x < 1: 1 / limit
    np.testing.assert_allclose(got[6], -k / 0.1, rtol=2e-6)                          # y = 1, x < limit: -1 / limit
    np.testing.assert_allclose(terms[1], t32[1], rtol=1e-6)
    np.testing.assert_allclose(terms[1], R.W6[1] * (-5 * np.log(0.1) - np.log(0.5)) / 8, rtol=1e-6)


def test_bce_at_the_log_clamps_matches_torch(shim):
    d = _tiny(6, opacity=[0.0, 1.0, 0.0, 1.0, 1e-9, 1 - 1e-7], sky=[1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    o = R.options(**dict(ONLY, mask="bce"))
    terms, g = shim_run(shim, d, o)
    t32, g32 = R.run(d, o, dtype=torch.float32)
    np.testing.assert_allclose(terms[1], t32[1], rtol=1e-6)
    np.testing.assert_allclose(g["opacity"], g32["opacity"], rtol=2e-6)


def test_depth_exact_cases(shim):
    empty = _tiny(4, lidar=[0.0, 0.005, 80.0, 95.0])
    for r, want in (("mean_on_hit", np.nan), ("sum", 0.0), ("mean_on_hw", 0.0)):
        o = R.options(**dict(ONLY, depth=("l1", False, False), reduction=r))
        terms, g = shim_run(shim, empty, o)
        assert np.array_equal(terms[2], np.float32(want), equal_nan=True) and not g["depth"].any() and not np.isnan(g["depth"]).any(), (r, terms)
        t32, g32 = R.run(empty, o, dtype=torch.float32)
        assert np.array_equal(t32[2], np.float32(want), equal_nan=True) and not g32["depth"].any()
    # pred beyond max_depth under normalize: in the valid set (it counts, its error is taken of the clamped value), gradient zero
    d = _tiny(3, depth=[85.0, 40.0, 5e-5], lidar=[60.0, 60.0, 60.0])
    o = R.options(**dict(ONLY, depth=("l1", True, False)))
    terms, g = shim_run(shim, d, o)
    t32, g32 = R.run(d, o, dtype=torch.float32)
    assert g["depth"].reshape(-1)[0] == 0 and g["depth"].reshape(-1)[2] == 0 and g["depth"].reshape(-1)[1] != 0
    np.testing.assert_allclose(terms[2], R.W6[2] * ((1 - 0.75) + (0.75 - 0.5)) / 2, rtol=1e-6)      # (pred 5e-5 is outside the set)
    np.testing.assert_allclose(g["depth"], g32["depth"], rtol=2e-6)
    # smooth_l1 on both sides of |e| = 1
    d = _tiny(4, depth=[12.5, 11.5, 14.0, 9.0], lidar=[12.0] * 4)
    o = R.options(**dict(ONLY, depth=("smooth_l1", False, False), reduction="sum"))
    terms, g = shim_run(shim, d, o)
    k = R.V6[2] * R.W6[2]
    np.testing.assert_allclose(terms[2], R.W6[2] * (0.125 + 0.125 + 1.5 + 2.5), rtol=1e-6)
    np.testing.assert_allclose(g["depth"].reshape(-1), [0.5 * k, -0.5 * k, k, -k], rtol=1e-6)


def test_one_row_has_a_nan_smoothness_term_and_a_finite_gradient(shim):
    d = R.make(1, 9, 3)
    o = R.options(**dict(ONLY, smoothness=True))
    terms, g = shim_run(shim, d, o)
    t64, g64 = R.ref(d, o)
    assert np.isnan(terms[4]) and np.isnan(t64[4]) and np.isfinite(g["depth"]).all()
    assert R.err(g["depth"], g64["depth"]) <= R.FLOOR


# ---- the two older option sets: losses.pixel_loss and losses.reg_losses ---------------------------------------------------------------
# The math under those two names is this file's math at two option sets.  Held here, without a GPU, to the oracle the GPU tests of the two
# names use (oracle/loss_oracle.py, float64) at THEIR bounds: pixel_loss 3e-6 of max(1, |term|) and 3e-6 of a gradient's largest entry
# (tests/test_gpu_00_bilagrid_parity.py test_pixel_loss_matches_reference_goldens), reg_losses rtol 2e-5 / atol 1e-7 on the terms and 2e-5 of
# a gradient's norm (tests/test_gpu_29_losses_random_sweep.py).  Inputs as tests/test_gpu_47_poisoned_memory.py _pixel_loss_case and
# tests/test_gpu_06_reg_losses.py build them.
OLD_SET_SHAPES = [(1, 1), (1, 37), (3, 5), (37, 53)]


def _pixel_set(shim, d, w, depth_type, use_mask, use_depth, use_ego):
    o = R.options(mask="bce" if use_mask else None, depth=(depth_type, False, False) if use_depth else None, entropy=False, smoothness=False,
                  dyn=False, ego=use_ego)
    terms, g = shim_run(shim, d, o, v6=(1.0, 1.0, 1.0, 0.0, 0.0, 0.0), w6=(*w, 0.0, 0.0, 0.0))
    assert not terms[3:].any()
    return terms[:3], g


def _pixel_set_check(terms, g, want, on, tag):
    for i, k in enumerate(("rgb_loss", "sky_loss", "depth_loss")):
        w_ = float(want[k]) if on[i] else 0.0
        assert abs(float(terms[i]) - w_) <= 3e-6 * max(1.0, abs(w_)), (tag, k, float(terms[i]), w_)
    for i, (k, name) in enumerate((("rgb", "v_rgb"), ("opacity", "v_opacity"), ("depth", "v_depth"))):
        if not on[i]:
            assert not g[k].any(), (tag, k)
            continue
        ref = np.asarray(want[name], np.float64)
        assert np.abs(g[k].astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30) <= 3e-6, (tag, k)


@pytest.mark.parametrize("H,W", OLD_SET_SHAPES)
def test_host_math_at_the_pixel_loss_option_set_matches_the_loss_oracle(shim, H, W):
    from oracle import loss_oracle as LO
    g = torch.Generator().manual_seed(H * 100 + W)
    t = dict(rgb=torch.rand(H, W, 3, generator=g), pixels=torch.rand(H, W, 3, generator=g), opacity=torch.rand(H, W, 1, generator=g) * 0.98 + 0.01,
             depth=torch.rand(H, W, 1, generator=g) * 40 + 0.5, sky=(torch.rand(H, W, generator=g) > 0.7).float(),
             lidar=torch.rand(H, W, generator=g) * 60 * (torch.rand(H, W, generator=g) > 0.3).float(), ego=(torch.rand(H, W, generator=g) > 0.8).float())
    t["lidar"].reshape(-1)[0] = 12.0            # (at least one lidar hit: the depth term divides by their count)
    t["ego"].reshape(-1)[0] = 0.0
    t["dyn"] = torch.zeros(H, W, 1)
    d64 = {k: v.double() for k, v in t.items()}
    w = (0.8, 0.05, 0.01)
    for depth_type in ("l1", "l2"):
        for um, ud, ue in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
            want = LO.pixel_loss(d64["rgb"], d64["pixels"], d64["opacity"], d64["sky"], d64["depth"], d64["lidar"], d64["ego"] if ue else None, w=w,
                                 depth_l2=depth_type == "l2")
            terms, grads = _pixel_set(shim, t, w, depth_type, um, ud, ue)
            _pixel_set_check(terms, grads, {k: v.numpy() for k, v in want.items()}, (True, um, ud), (depth_type, um, ud, ue))


def test_host_math_at_the_pixel_loss_option_set_matches_the_reference_goldens(shim):
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pixel_loss_*f32.npz")))
    assert len(files) >= 3
    for f in files:
        z = np.load(f)
        ego = bool(z["egocar"].size)
        d = {k: torch.from_numpy(z[s]) for k, s in (("rgb", "rgb"), ("pixels", "pixels"), ("opacity", "opacity"), ("depth", "depth"), ("sky", "sky_masks"),
                                                    ("lidar", "lidar"))}
        d["ego"] = torch.from_numpy(z["egocar"]).float() if ego else torch.zeros_like(d["sky"])
        d["dyn"] = torch.zeros_like(d["opacity"])
        terms, grads = _pixel_set(shim, d, [float(v) for v in z["w"]], "l2" if int(z["depth_l2"]) else "l1", True, True, ego)
        _pixel_set_check(terms, grads, z, (True, True, True), os.path.basename(f))


@pytest.mark.parametrize("H,W", OLD_SET_SHAPES)
def test_host_math_at_the_reg_losses_option_set_matches_the_loss_oracle(shim, H, W):
    import itertools
    from oracle import loss_oracle as LO
    g = torch.Generator().manual_seed(H * 131 + W)
    pix = torch.rand(H, W, 3, generator=g)
    rgb = torch.rand(H, W, 3, generator=g) * 1.1
    op = torch.rand(H, W, 1, generator=g)
    if H * W > 1:
        op[0, 0, 0], op[-1, -1, 0] = 0.0, 1.0             # outside the clamp interval: zero gradient
    dep = torch.rand(H, W, 1, generator=g) * 30 + 0.2
    dyn = torch.rand(H, W, 1, generator=g)
    dyn.reshape(-1)[0] = 0.9                              # (at least one pixel above the threshold)
    ego = (torch.rand(H, W, generator=g) > 0.8).float()
    ego.reshape(-1)[0] = 0.0
    wt = (0.7, 1.3, 0.4)
    d = dict(rgb=rgb, pixels=pix, opacity=op, depth=dep, dyn=dyn, ego=ego, sky=torch.zeros(H, W), lidar=torch.zeros(H, W))
    for use_op, use_dyn, use_dep, use_ego in itertools.product((False, True), repeat=4):
        if not (use_op or use_dyn or use_dep) or (use_dep and (H == 1 or W == 1)):
            continue
        tag = (use_op, use_dyn, use_dep, use_ego)
        o64 = {k: v.double().requires_grad_(True) for k, v in dict(op=op, dep=dep, rgb=rgb).items()}
        t_ref = LO.reg_losses(pix.double(), o64["op"] if use_op else None, o64["dep"] if use_dep else None, o64["rgb"],
                              dyn.double() if use_dyn else None, ego.double() if use_ego else None)
        (t_ref * torch.tensor(wt, dtype=torch.float64)).sum().backward()
        o = R.options(mask=None, depth=None, entropy=use_op, smoothness=use_dep, dyn=use_dyn, ego=use_ego)
        terms, grads = shim_run(shim, d, o, v6=(0.0, 0.0, 0.0, *wt), w6=(0.0, 0.0, 0.0, 1.0, 1.0, 1.0))
        assert not terms[:3].any(), tag
        assert torch.allclose(torch.from_numpy(terms[3:]).double(), t_ref.detach(), rtol=2e-5, atol=1e-7), (tag, terms, t_ref)
        for k, name in (("op", "opacity"), ("dep", "depth"), ("rgb", "rgb")):
            want, got = o64[k].grad, torch.from_numpy(grads[name]).double()
            if want is None or float(want.abs().max()) == 0.0:
                assert float(got.abs().max()) == 0.0, (tag, k)
                continue
            assert float((got - want).norm() / want.norm()) < 2e-5, (tag, k)
        if use_op and H * W > 1:
            assert grads["opacity"][0, 0, 0] == 0.0 and grads["opacity"][-1, -1, 0] == 0.0


# ---- argument validation, options, the seam -----------------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu():
    lib, p = L.lib(), 1 << 20      # never dereferenced: every case fails its argument check first
    w = (ctypes.c_float * 6)(*R.W6)

    def head(H=4, W=4, rgb=p, pixels=p, opacity=p, depth=p, sky=p, lidar=p, ego=None, dyn=None, kind=1, limit=0.1, typ=0, red=0, ent=1, smooth=1,
             max_depth=80.0, weights=w):
        return (H, W, rgb, pixels, opacity, depth, sky, lidar, ego, dyn, kind, limit, typ, 0, 0, max_depth, red, ent, smooth, 0.2, weights)

    def fwd(terms=p, sums=p, temp=p, nb=1 << 20, **kw):
        return lib.bds_image_loss_fwd(*head(**kw), terms, sums, temp, nb, None)

    def bwd(sums=p, v_terms=p, **kw):
        return lib.bds_image_loss_bwd(*head(**kw), sums, v_terms, p, p, p, None)

    for f in (fwd, bwd):
        assert f(H=0) == L.BDS_EINVAL and f(W=0) == L.BDS_EINVAL and f(H=1 << 16, W=1 << 16) == L.BDS_EINVAL
        assert f(rgb=None) == L.BDS_EINVAL and f(pixels=None) == L.BDS_EINVAL and f(weights=None) == L.BDS_EINVAL
        assert f(sky=None) == L.BDS_EINVAL and f(kind=0) == L.BDS_EINVAL and f(opacity=None) == L.BDS_EINVAL       # the sky pair
        assert f(depth=None) == L.BDS_EINVAL and f(depth=None, smooth=0) == L.BDS_EINVAL                           # the lidar pair
        assert f(opacity=None, sky=None, kind=0) == L.BDS_EINVAL and f(depth=None, lidar=None) == L.BDS_EINVAL      # the flags' images
        assert f(kind=3) == L.BDS_EINVAL and f(kind=-1) == L.BDS_EINVAL and f(typ=3) == L.BDS_EINVAL and f(red=3) == L.BDS_EINVAL
        assert f(kind=2, limit=0.0) == L.BDS_EINVAL and f(kind=2, limit=1.0) == L.BDS_EINVAL and f(max_depth=0.0) == L.BDS_EINVAL
    assert fwd(terms=None) == L.BDS_EINVAL and fwd(sums=None) == L.BDS_EINVAL and fwd(temp=None) == L.BDS_EINVAL
    assert fwd(nb=lib.bds_image_loss_temp_bytes(4, 4) - 1) == L.BDS_EINVAL
    assert bwd(sums=None) == L.BDS_EINVAL and bwd(v_terms=None) == L.BDS_EINVAL
    assert lib.bds_image_loss_temp_bytes(4, 4) == 36 and lib.bds_image_loss_temp_bytes(1080, 1920) == 36 * 2048 and lib.bds_image_loss_temp_bytes(0, 4) == 0
    assert 2048 * 256 == R.FWD_GRID < R.SWEEP_SHAPE[0] * R.SWEEP_SHAPE[1]


def test_abi_version_and_signatures():
    assert L.lib().bds_abi_version() == 7
    decl = {k: v for k, v in declared_signatures().items() if k.startswith("bds_image_loss")}
    assert sorted(decl) == ["bds_image_loss_bwd", "bds_image_loss_fwd", "bds_image_loss_temp_bytes"]
    for name, (ret, args) in decl.items():
        res, argtypes = L._SIGS[name]
        assert res is ret and len(argtypes) == len(args), name
        for got, want in zip(argtypes, args):
            assert (got is ctypes.c_void_p or issubclass(got, ctypes._Pointer)) if want is ctypes.c_void_p else got is want, (name, got, want)


def test_unknown_options_raise_with_the_reference_wording_and_cpu_tensors_are_refused():
    d = R.make(4, 4)
    pos, kw = R.call_args(d, R.options())
    with pytest.raises(NotImplementedError, match="Unknown loss type: huber"):
        losses.image_terms(*pos, **dict(kw, depth_loss_type="huber"))
    with pytest.raises(NotImplementedError, match="Unknown loss type: focal"):
        losses.image_terms(*pos, **dict(kw, mask_loss="focal"))
    for r in ("none", "median"):
        with pytest.raises(NotImplementedError, match="Unknown reduction method: " + r):
            losses.image_terms(*pos, **dict(kw, depth_reduction=r))
    with pytest.raises(ValueError):
        losses.image_terms(*pos, **dict(kw, weights=(1.0, 2.0)))
    with pytest.raises(ValueError):
        losses.image_terms(pos[0], pos[1], None, pos[3], **kw)
    with pytest.raises(L.BdsError):
        losses.image_terms(*pos, **kw)


def _trainer(block, cls=R.StandInTrainer, **kw):
    return cls(R.Ns(R.LOSS_BLOCKS[block]), **kw)


KEYS = {
    "omnire_ms_bilateral_extended": ["rgb_loss", "ssim_loss", "sky_loss_opacity", "depth_loss", "affine_loss"],
    "paper_legacy/streetgs": ["rgb_loss", "ssim_loss", "sky_loss_opacity", "depth_loss", "opacity_entropy_loss", "inverse_depth_smoothness_loss",
                              "vehicle_region_rgb_loss"],
}
CLASS_KEYS = ["Background_sharp_shape_reg", "RigidNodes_reg_a", "RigidNodes_reg_b"]


def test_install_and_uninstall_restore_the_class_and_cpu_tensors_keep_its_method():
    class Trainer(R.StandInTrainer):
        pass

    class Other(R.StandInTrainer):
        pass
    assert "compute_losses" not in Trainer.__dict__ and not hasattr(Trainer, "_bds_reference_compute_losses")
    losses.install(Trainer)
    assert Trainer.compute_losses is losses.image_compute_losses and Trainer._bds_reference_compute_losses is R.StandInTrainer.compute_losses
    assert Other.compute_losses is R.StandInTrainer.compute_losses
    d = R.make(24, 40, 5)
    for block in KEYS:
        step = 20001 if "streetgs" in block else 0
        got = _trainer(block, Trainer, step=step).compute_losses(*R.trainer_inputs(d))      # CPU tensors: the class's own method
        ref = _trainer(block, step=step).compute_losses(*R.trainer_inputs(d))
        assert list(got) == list(ref) == KEYS[block] + CLASS_KEYS
        assert all(torch.equal(got[k], ref[k]) for k in ref)
    losses.install(Trainer)                      # twice: still one original
    losses.uninstall(Trainer)
    assert "compute_losses" not in Trainer.__dict__ and not hasattr(Trainer, "_bds_reference_compute_losses")
    assert Trainer.compute_losses is R.StandInTrainer.compute_losses


@pytest.mark.parametrize("block", list(KEYS))
@pytest.mark.parametrize("ego", [True, False])
def test_installed_method_composes_the_dict_like_the_class(monkeypatch, block, ego):
    """The composition on the CPU, with the fused node and SSIM stood in for by the framework expressions: the reference's keys in the
    reference's order and values, the modules' methods called as the class calls them, the depth weight's decay, the side effect."""
    class Trainer(R.StandInTrainer):
        pass
    seen = {}

    def terms(*a, **kw):
        seen.update(kw)
        return R.framework_terms(*a, **kw)
    monkeypatch.setattr(losses, "image_terms", terms)
    monkeypatch.setattr(losses, "ssim_loss", lambda a, b: 1 - R.gaussian_ssim(b.permute(2, 0, 1)[None], a.permute(2, 0, 1)[None]))
    monkeypatch.setattr(losses, "_on_device", lambda outputs: True)
    d = R.make(24, 40, 6)
    cfg = R.Ns(R.LOSS_BLOCKS[block])
    cfg["depth"] = R.Ns(cfg["depth"], lidar_w_decay=2.0)
    step = 20001 if "streetgs" in block else 4000

    def run(cls):
        tr = cls(cfg, step=step)
        outputs, infos, cams = R.trainer_inputs(d, ego=ego)
        out = tr.compute_losses(outputs, infos, cams)
        sum(out.values()).backward()
        return tr, out, {k: outputs[k].grad for k in R.GRADS}
    ref_tr, ref, ref_g = run(R.StandInTrainer)
    losses.install(Trainer)
    try:
        tr, got, got_g = run(Trainer)
    finally:
        losses.uninstall(Trainer)
    assert list(got) == list(ref) == KEYS[block] + CLASS_KEYS
    for k in ref:
        assert float(got[k]) == pytest.approx(float(ref[k]), rel=1e-5), k
    for k in R.GRADS:
        np.testing.assert_allclose(got_g[k].numpy(), ref_g[k].numpy(), rtol=1e-4, atol=1e-9, err_msg=k)
    assert seen["weights"][2] == pytest.approx(cfg.depth.w * np.exp(-step / 8000 * 2.0), rel=1e-7)          # lidar_w_decay, on the host
    assert seen["depth_inverse"] == cfg.depth.inverse_depth and seen["mask_loss"] == "bce" and seen["max_depth"] == 80
    assert (seen["egocar_masks"] is not None) == ego
    for name in ("Background", "RigidNodes"):
        assert tr.models[name].calls == ref_tr.models[name].calls == ["compute_reg_loss"]
    if "Affine" in tr.models:
        assert tr.models["Affine"].calls == ref_tr.models["Affine"].calls


def test_installed_method_sets_render_dynamic_mask_and_keeps_the_zero_key(monkeypatch):
    class Trainer(R.StandInTrainer):
        pass
    monkeypatch.setattr(losses, "image_terms", R.framework_terms)
    monkeypatch.setattr(losses, "ssim_loss", lambda a, b: 1 - R.gaussian_ssim(b.permute(2, 0, 1)[None], a.permute(2, 0, 1)[None]))
    monkeypatch.setattr(losses, "_on_device", lambda outputs: True)
    d = R.make(24, 40, 6)
    losses.install(Trainer)
    try:
        for step, flag, key in ((19999, False, False), (20000, True, False), (20001, False, True)):
            tr = _trainer("paper_legacy/streetgs", Trainer, step=step)
            out = tr.compute_losses(*R.trainer_inputs(d))
            assert tr.render_dynamic_mask is flag and ("vehicle_region_rgb_loss" in out) is key, step
        tr = _trainer("paper_legacy/streetgs", Trainer, step=20001)
        out = tr.compute_losses(*R.trainer_inputs(dict(d, dyn=torch.zeros_like(d["dyn"]))))
        assert float(out["vehicle_region_rgb_loss"]) == 0.0            # the documented deviation: the key with value 0
        assert "vehicle_region_rgb_loss" not in tr._bds_reference_compute_losses(*R.trainer_inputs(dict(d, dyn=torch.zeros_like(d["dyn"]))))
        with pytest.raises(KeyError):                                  # no original_rgb under the multi-scale bilateral transform
            _trainer("omnire_ms_bilateral_extended", Trainer).compute_losses(*R.trainer_inputs(d, original=False))
        tr = _trainer("omnire_ms_bilateral_extended", Trainer)
        tr.depth_loss_fn.depth_error_percentile = 0.9
        with pytest.raises(NotImplementedError):
            tr.compute_losses(*R.trainer_inputs(d))
    finally:
        losses.uninstall(Trainer)
