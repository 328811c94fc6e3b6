"""The fused image loss on the MI355X (the image-loss section of csrc/loss.hip through bilateral_driving_amd/losses.py ``image_terms``)
against the float64 restatement (tests/image_loss_ref64.py), the reference-generated golden (scripts/gen_golden_image_loss.py) and the
same kernels called as two nodes (``pixel_loss`` + ``reg_losses``), on poisoned, recycled memory with guard bands (tests/poison.py), with every input and the
incoming gradient at 4-byte phases (tests/placement.py), twice for the bit-equality the op claims; and the installed
``compute_losses`` on a stand-in with BasicTrainer's attribute layout.

Bounds (tests/image_loss_ref64.py): per compared tensor (each term, each gradient), the largest difference over the tensor's largest
reference magnitude is held to 2 x the float32 framework expression's own such error against float64 on the same inputs (run on the
CPU: its order of summation is fixed there) + FLOOR.  FLOOR = 6.0e-7 is the host shim's largest error over the same cases, measured on
the CPU by tests/test_image_loss_cpu.py (the entropy and sky terms).  A reference that is exactly zero (a term that is off, the
gradient under the egocar mask) is held exactly, a NaN one (an empty mean) by NaN.  The forward strides a grid of at most 2048
workgroups of 256 threads (R.FWD_GRID = 524 288 pixels a sweep): the 725 x 725 case is more than one sweep.

Measured on the MI355X: over the cases the worst error is 2.2e-7 (a depth gradient) against bounds of 8e-7 and more; the old option set
is 1.3e-7 from float64 (``pixel_loss`` + ``reg_losses``, the same kernels as two nodes: 1.3e-7; 5.7e-9 between the two, the rgb gradient's
two products against one).  Under the installed ``compute_losses`` the
rgb gradient also carries SSIM's node: 3.7e-7 .. 1.35e-6 against the framework's own 2.6e-7 .. 5.2e-7 (bounds 1.1e-6 .. 1.64e-6)."""
import os

import numpy as np
import pytest
import torch

from tests import image_loss_ref64 as R
from tests import placement, poison

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "image_loss.npz")
CASES = R.gpu_cases()


@pytest.fixture(scope="module")
def S():
    from bilateral_driving_amd import losses
    return losses


def fused(S, d, o, off=0):
    """image_terms on the GPU with every input ``off`` elements behind an aligned base and the incoming gradient re-placed likewise ->
    (terms, grads) in R.run's layout."""
    return R.run(d, o, fn=S.image_terms, dtype=torch.float32, device="cuda", place=lambda t: placement.placed(t, off),
                 regrad=lambda t: placement.regrad(t, off))


def poisoned_twice(run, name):
    """``run()`` plainly and inside poisoned allocations: nothing unwritten, no guard touched, the two results bit-equal."""
    plain = run()
    torch.cuda.synchronize()
    with poison.poisoned_allocations(True, name=name) as pz:
        got = run()
        torch.cuda.synchronize()
        assert len(pz.records) >= 3
    for (k, a), (_, b) in zip([("terms", got[0])] + list(got[1].items()), [("terms", plain[0])] + list(plain[1].items())):
        assert not bool(poison.holds_poison(torch.as_tensor(a)).any()), k
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), k
    return got


@pytest.mark.parametrize("case", list(CASES))
def test_terms_and_gradients_match_float64(S, case):
    H, W, seed, o = CASES[case]
    d = R.make(H, W, seed)
    ref = R.ref(d, o)
    b = R.bounds(R.errors(R.run(d, o, dtype=torch.float32), ref))
    off = 1 + list(CASES).index(case) % 3
    got = poisoned_twice(lambda: fused(S, d, o, off), "image_terms " + case)
    e = R.errors(got, ref)
    print(f"\nimage_terms {case} (phase {4 * off}): worst error {max(e.values()):.3e} ({max(e, key=e.get)}), its bound {b[max(e, key=e.get)]:.3e}")
    assert R.within(e, b), {k: (e[k], b[k]) for k in b if e[k] > b[k]}
    on = (True, o["mask"] is not None, o["depth"] is not None, o["entropy"], o["smoothness"], o["dyn"])
    assert all(got[0][k] == 0 for k in range(6) if not on[k])
    if o["ego"]:
        under = d["ego"].bool().numpy()
        assert not got[1]["rgb"][under].any()                                   # valid = 0: no photometric gradient


def test_every_phase_and_aligned_change_no_bit(S):
    H, W, seed, o = CASES["smooth_l1-norm-inv-safe_bce"]
    d = R.make(H, W, seed)
    runs = [fused(S, d, o, off) for off in (0, 1, 2, 3)]
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and all(np.array_equal(r[1][k], runs[0][1][k]) for k in R.GRADS)


def test_against_the_reference_golden(S):
    z = np.load(GOLD)
    d = {k: torch.from_numpy(z[k]) for k in ("rgb", "pixels", "opacity", "depth", "sky", "lidar", "ego")}
    d["dyn"] = torch.zeros_like(d["opacity"])
    off = dict(mask=None, depth=None, entropy=False, smoothness=False, dyn=False)
    entries = [(R.options(**off), 0, "rgb", z["rgb_value"], z["rgb_grad"])]
    entries += [(R.options(**dict(off, mask=kind)), 1, "opacity", z[f"mask_{kind}_value"], z[f"mask_{kind}_grad"]) for kind in ("bce", "safe_bce")]
    for k, c in enumerate(z["depth_cases"]):
        t, n, i, r = str(c).split(",")
        entries.append((R.options(**dict(off, depth=(t, bool(int(n)), bool(int(i))), reduction=r)), 2, "depth", z[f"depth_{k}_value"], z[f"depth_{k}_grad"]))
    assert len(entries) == 17
    for o, k, g, value, grad in entries:      # the rule with the golden (the reference's own float32 run) as the float32 side
        (t64, g64), (terms, grads) = R.ref(d, o), fused(S, d, o, 1)
        assert R.err(terms[k], t64[k]) <= 2 * R.err(value, t64[k]) + R.FLOOR, (o, terms[k], value, t64[k])
        assert R.err(grads[g], g64[g]) <= 2 * R.err(grad, g64[g]) + R.FLOOR, (o, g)


def _tiny(n, **kw):
    d = dict(rgb=torch.full((1, n, 3), 0.5), pixels=torch.full((1, n, 3), 0.25), opacity=torch.full((1, n, 1), 0.5), depth=torch.full((1, n, 1), 10.0),
             sky=torch.zeros(1, n), lidar=torch.full((1, n), 12.0), ego=torch.zeros(1, n), dyn=torch.zeros(1, n, 1))
    for k, v in kw.items():
        d[k] = torch.tensor(v, dtype=torch.float32).reshape(d[k].shape)
    return d


ONLY = dict(mask=None, depth=None, entropy=False, smoothness=False, dyn=False, ego=False)


def test_exact_cases_on_the_device(S):
    """The SafeBCE and depth cases of tests/test_image_loss_cpu.py (the derivations are there)."""
    d = _tiny(8, opacity=[0.0, 1.0, 1.000001, -1e-7, 0.95, 0.999, 0.05, 0.5], sky=[1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    o = R.options(**dict(ONLY, mask="safe_bce"))
    terms, g = fused(S, d, o, 1)
    t32, g32 = R.run(d, o, dtype=torch.float32)
    got, k = g["opacity"].reshape(-1), R.V6[1] * R.W6[1] / 8
    assert got[0] == 0 and got[1] == 0
    np.testing.assert_allclose(got, g32["opacity"].reshape(-1), rtol=2e-6)
    np.testing.assert_allclose(got[2:7], [k / 0.1, -k / 0.1, k / 0.1, k / 0.1, -k / 0.1], rtol=2e-6)
    np.testing.assert_allclose(terms[1], t32[1], rtol=1e-6)
    empty = _tiny(4, lidar=[0.0, 0.005, 80.0, 95.0])
    for r, want in (("mean_on_hit", np.nan), ("sum", 0.0), ("mean_on_hw", 0.0)):
        terms, g = poisoned_twice(lambda: fused(S, empty, R.options(**dict(ONLY, depth=("l1", False, False), reduction=r)), 1), "image_terms empty " + r)
        assert np.array_equal(terms[2], np.float32(want), equal_nan=True) and not g["depth"].any() and not np.isnan(g["depth"]).any(), (r, terms)
    d = _tiny(3, depth=[85.0, 40.0, 5e-5], lidar=[60.0, 60.0, 60.0])
    terms, g = fused(S, d, R.options(**dict(ONLY, depth=("l1", True, False))), 2)
    assert g["depth"].reshape(-1)[0] == 0 and g["depth"].reshape(-1)[2] == 0 and g["depth"].reshape(-1)[1] != 0
    np.testing.assert_allclose(terms[2], R.W6[2] * 0.25, rtol=1e-6)
    d = _tiny(4, depth=[12.5, 11.5, 14.0, 9.0], lidar=[12.0] * 4)
    terms, g = fused(S, d, R.options(**dict(ONLY, depth=("smooth_l1", False, False), reduction="sum")), 3)
    np.testing.assert_allclose(terms[2], R.W6[2] * 4.25, rtol=1e-6)
    np.testing.assert_allclose(g["depth"].reshape(-1), np.array([0.5, -0.5, 1, -1]) * R.V6[2] * R.W6[2], rtol=1e-6)
    d = R.make(1, 9, 3)
    terms, g = fused(S, d, R.options(**dict(ONLY, smoothness=True)), 1)
    assert np.isnan(terms[4]) and R.err(g["depth"], R.ref(d, R.options(**dict(ONLY, smoothness=True)))[1]["depth"]) <= R.FLOOR


def test_the_old_option_set_equals_pixel_loss_plus_reg_losses(S):
    """One node against the same kernels called as two nodes (``pixel_loss`` and ``reg_losses`` are option sets of ``image_terms``).  Not
    bit-equal: the one node's rgb gradient is one product with the sum of the rgb and the dynamic-region factors, the two nodes' is two
    products that autograd adds.  Both within the bound of float64, so within twice the bound of each other."""
    H, W, seed = 37, 53, 90
    d = R.make(H, W, seed)
    o = R.options(mask="bce", depth=("l1", False, False))
    ref = R.ref(d, o)
    b = R.bounds(R.errors(R.run(d, o, dtype=torch.float32), ref))
    got = fused(S, d, o)

    def old(*a, **kw):
        pix = S.pixel_loss(a[0], a[2], a[3], a[1], kw["sky_masks"], kw["lidar_depth"], kw["egocar_masks"], *R.W6[:3], "l1", 80.0)
        reg = S.reg_losses(a[1], a[2], a[3], a[0], kw["dyn_opacity"], kw["egocar_masks"], 0.2)
        return torch.cat([pix, reg * torch.tensor(R.W6[3:], device="cuda")])
    prev = R.run(d, o, fn=old, dtype=torch.float32, device="cuda")
    e, e_prev, between = R.errors(got, ref), R.errors(prev, ref), R.errors(got, prev)
    print(f"\nimage_terms vs float64 {max(e.values()):.3e}, pixel_loss + reg_losses vs float64 {max(e_prev.values()):.3e}, between {max(between.values()):.3e}")
    assert R.within(e, b)
    assert R.within(e_prev, b), {k: (e_prev[k], b[k]) for k in b if e_prev[k] > b[k]}
    assert all(between[k] <= 2 * b[k] for k in b), {k: (between[k], 2 * b[k]) for k in b if between[k] > 2 * b[k]}


# ---- the install hook --------------------------------------------------------------------------------------------------------------
def _loss_and_grads(tr, inputs):
    outputs, infos, cams = inputs
    out = tr.compute_losses(outputs, infos, cams)
    sum(out.values()).backward()
    torch.cuda.synchronize()
    return {k: float(v.detach()) for k, v in out.items()}, {k: outputs[k].grad.cpu().numpy() for k in R.GRADS}


@pytest.mark.parametrize("block,step,ego", [("omnire_ms_bilateral_extended", 4000, True), ("paper_legacy/streetgs", 20001, True),
                                            ("paper_legacy/streetgs", 20000, False)])
def test_installed_compute_losses_matches_the_class_and_float64(S, block, step, ego):
    class Trainer(R.StandInTrainer):
        pass
    d = R.make(37, 53, 91)
    cfg = R.Ns(R.LOSS_BLOCKS[block])
    cfg["depth"] = R.Ns(cfg["depth"], lidar_w_decay=2.0)
    ref_vals, ref_g = _loss_and_grads(R.StandInTrainer(cfg, "cuda", step), R.trainer_inputs(d, "cuda", ego=ego))
    tr = Trainer(cfg, "cuda", step)
    S.install(Trainer)
    try:
        vals, g = _loss_and_grads(tr, R.trainer_inputs(d, "cuda", ego=ego))
        again = _loss_and_grads(Trainer(cfg, "cuda", step), R.trainer_inputs(d, "cuda", ego=ego))
    finally:
        S.uninstall(Trainer)
    dyn_on = "dynamic_region" in cfg and step > cfg.dynamic_region.start_from
    assert tr.render_dynamic_mask is ("dynamic_region" in cfg and step == cfg.dynamic_region.start_from)
    assert list(vals) == list(ref_vals), (list(vals), list(ref_vals))       # (pixels qualify here: the zero-key deviation does not show)
    # float64: the six terms with the trainer's weights, SSIM by the framework expression in float64
    w = [cfg.rgb.w, cfg.mask.w, cfg.depth.w * float(np.exp(-step / 8000 * 2.0)), cfg.get("opacity_entropy", R.Ns(w=0)).w,
         cfg.get("inverse_depth_smoothness", R.Ns(w=0)).w, 1.0]
    o = R.options(mask="bce", depth=(cfg.depth.loss_type, cfg.depth.normalize, cfg.depth.inverse_depth), entropy="opacity_entropy" in cfg,
                  smoothness="inverse_depth_smoothness" in cfg, dyn=dyn_on, ego=ego)
    t64, g64 = R.ref(d, o, W6=w, V6=(1.0,) * 6)
    valid = (1.0 - d["ego"].double()) if ego else torch.ones_like(d["ego"].double())
    rgb64 = d["rgb"].double().requires_grad_(True)
    ssim64 = cfg.ssim.w * (1 - R.gaussian_ssim((d["pixels"].double() * valid[..., None]).permute(2, 0, 1)[None], (rgb64 * valid[..., None]).permute(2, 0, 1)[None]))
    ssim64.backward()
    g64 = dict(g64, rgb=g64["rgb"] + rgb64.grad.numpy())
    want = {key: t64[k] for k, key in enumerate(S.IMAGE_TERMS) if key in vals}
    want["ssim_loss"] = float(ssim64)
    for k in ref_vals:
        if k in want:                    # |fused - float64| <= 2 |framework - float64| + FLOOR |float64|
            print(f"\nimage loss hook {k}: framework vs float64 {abs(ref_vals[k] - want[k]):.3e}, fused {abs(vals[k] - want[k]):.3e} of {abs(want[k]):.3e}")
            assert abs(vals[k] - want[k]) <= 2 * abs(ref_vals[k] - want[k]) + R.FLOOR * abs(want[k]), (k, vals[k], ref_vals[k], want[k])
        else:                            # the trainer's own modules: the same launches
            assert vals[k] == ref_vals[k], k
        if k != "ssim_loss":             # (SSIM is its own node still, and its forward ends in float atomics: its value is not bit-equal)
            assert vals[k] == again[0][k], k
    for k in R.GRADS:
        e32, e = R.err(ref_g[k], g64[k]), R.err(g[k], g64[k])
        print(f"\nimage loss hook gradient {k}: framework vs float64 {e32:.3e}, fused {e:.3e}")
        assert e <= 2 * e32 + R.FLOOR, (k, e, e32)
        assert np.array_equal(g[k].view(np.int32), again[1][k].view(np.int32)), k


def test_installed_compute_losses_keeps_the_zero_dynamic_key(S):
    class Trainer(R.StandInTrainer):
        pass
    d = R.make(37, 53, 92)
    d["dyn"] = torch.zeros_like(d["dyn"])
    cfg = R.Ns(R.LOSS_BLOCKS["paper_legacy/streetgs"])
    ref_vals, _ = _loss_and_grads(R.StandInTrainer(cfg, "cuda", 20001), R.trainer_inputs(d, "cuda"))
    S.install(Trainer)
    try:
        vals, _ = _loss_and_grads(Trainer(cfg, "cuda", 20001), R.trainer_inputs(d, "cuda"))
    finally:
        S.uninstall(Trainer)
    assert "vehicle_region_rgb_loss" not in ref_vals and vals["vehicle_region_rgb_loss"] == 0.0
    assert [k for k in vals if k != "vehicle_region_rgb_loss"] == list(ref_vals)
