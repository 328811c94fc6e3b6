"""Pose chain and skinning of the SMPL nodes on the MI355X (csrc/smpl.hip through bilateral_driving_amd/smpl.py): the fused op against the
reference-generated golden vectors (scripts/gen_golden_smpl_skin.py) and against the float64 restatement (tests/smpl_skin_ref64.py)
over sizes, instance counts and fields; border safety on field views inside a NaN-filled buffer; poisoned allocations with guard
bands; determinism of the pose and translation gradients; the interpolated and the ball form; and the install hook on a stand-in with
SMPLNodes' attribute layout, through rasterization().

Tolerances are the measured bound of tests/smpl_skin_ref64.py (4 x the float32 framework's own error against float64 on the same
inputs, each tensor's largest error over max(1, its largest reference magnitude); printed by every test).  Measured on the MI355X: the
float32 framework's error 2.6e-7 .. 1.4e-6 over the cases (largest at I = 1, V = 6890: the pose gradients are sums over every point),
so the bounds are 1.0e-6 .. 5.5e-6; the fused op's error 1.8e-7 .. 1.5e-6, against the golden 7.3e-7 and 6.6e-7."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import smpl_skin_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smpl_skin.npz")
POSE = ("instances_quats", "smpl_quats", "instances_trans")


@pytest.fixture(scope="module")
def S():
    from bilateral_driving_amd import smpl
    return smpl


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLD)


def run_fused(S, d, f, ball=False, interpolate=False, grad=True, field_views=None):
    """skin_transform on the GPU -> (outs, grads) in run_framework's layout.  ``field_views``: (voxel_base, voxel_corr) device tensors
    to use in place of d's."""
    dev = "cuda"
    ts = {k: d[k].detach().to(dev).clone().requires_grad_(grad) for k in R.INPUTS if d.get(k) is not None}
    kw = R.template_kwargs(d, device=dev)
    if field_views is not None:
        kw["voxel_base"], ts["voxel_corr"] = field_views
    wm, wq = S.skin_transform(ts["means"], None if ball else ts["quats"], ts["instances_quats"], ts["smpl_quats"], ts["instances_trans"],
                              d["instances_fv"].to(dev), f, voxel_corr=ts.get("voxel_corr"), interpolate=interpolate, ball=ball, **kw)
    outs = {"wm": wm.detach().cpu().numpy()}
    loss = (wm * d["w_m"].to(dev)).sum()
    if not ball:
        outs["wq"] = wq.detach().cpu().numpy()
        loss = loss + (wq * d["w_q"].to(dev)).sum()
    else:
        assert wq is None
    grads = {}
    if grad:
        loss.backward()
        grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy() for k, t in ts.items()}
    return outs, grads, loss


@pytest.mark.parametrize("which", [0, 1])
def test_fused_matches_reference_golden(S, golden, which):
    d, z = golden
    f, s = int(z["train_frames"][which]), int(z["stride"])
    bound, e32 = R.measured_bound(d, f)
    outs, grads, _ = run_fused(S, d, f)
    errs = {"wm": R.scaled_err(outs["wm"][::s], z[f"f{f}_wm"]), "wq": R.scaled_err(outs["wq"][::s], z[f"f{f}_wq"])}
    for k in R.INPUTS:      # (the field gradient: the same bound relative to its largest entry; its summation order is unspecified)
        errs[k] = R.scaled_err(grads[k][::s] if k in ("means", "quats") else grads[k], z[f"f{f}_grad_{k}"])
    print(f"\nsmpl golden frame {f}: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused vs golden {max(errs.values()):.3e}")
    assert max(errs.values()) <= bound, (errs, bound)


CASES = [   # I, V, field, parents, absent
    (1, 1, (2, 2, 2), R.SMPL_PARENTS, ()),
    (3, 63, (3, 5, 7), R.SMPL_PARENTS, (1,)),
    (1, 64, (4, 16, 16), R.PERMUTED_PARENTS, ()),
    (3, 65, (2, 2, 2), R.PERMUTED_PARENTS, ()),
    (17, 65, (3, 5, 7), R.SMPL_PARENTS, (0, 16)),
    (17, 1, (2, 2, 2), R.SMPL_PARENTS, (3,)),
    (1, 6890, (4, 16, 16), R.SMPL_PARENTS, ()),
    (3, 6890, (3, 5, 7), R.SMPL_PARENTS, (2,)),
]


@pytest.mark.parametrize("I,V,dhw,parents,absent", CASES, ids=[f"I{c[0]}-V{c[1]}-{'x'.join(map(str, c[2]))}" for c in CASES])
def test_fused_matches_float64(S, I, V, dhw, parents, absent):
    d = R.make_inputs(I, V, dhw, seed=7 * I + V, parents=parents, absent=absent)
    ref = R.run_framework(d, 1)
    bound, e32 = R.measured_bound(d, 1, ref)
    outs, grads, _ = run_fused(S, d, 1)
    worst = R.worst(outs, grads, ref)
    print(f"\nsmpl I={I} V={V} {dhw}: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused {worst:.3e}")
    assert worst <= bound, (worst, bound)
    for i in absent:
        rows = slice(i * V, (i + 1) * V)
        assert (outs["wm"][rows] == d["instances_trans"][1, i].numpy()).all() and (outs["wq"][rows] == np.array([1, 0, 0, 0], np.float32)).all()
        assert np.abs(grads["means"][rows]).max() == 0 and np.abs(grads["quats"][rows]).max() == 0 and np.abs(grads["voxel_corr"][i]).max() == 0
        assert np.abs(grads["smpl_quats"][1, i]).max() == 0 and np.abs(grads["instances_quats"][1, i]).max() == 0
    for k in POSE:          # the tables' gradients live in row cur_frame only
        assert np.abs(grads[k][0]).max() == 0 and np.abs(grads[k][2]).max() == 0


def test_every_instance_absent(S):
    I, V = 3, 65
    d = R.make_inputs(I, V, (3, 5, 7), seed=4, absent=(0, 1, 2))
    outs, grads, _ = run_fused(S, d, 1)
    assert (outs["wm"] == d["instances_trans"][1].repeat_interleave(V, 0).numpy()).all()
    assert (outs["wq"] == np.array([1, 0, 0, 0], np.float32)).all()
    for k in ("means", "quats", "instances_quats", "smpl_quats", "voxel_corr"):
        assert np.abs(grads[k]).max() == 0, k
    ref = d["w_m"].double().reshape(I, V, 3).sum(1).numpy()
    assert R.scaled_err(grads["instances_trans"][1], ref) <= 1e-6 and np.abs(grads["instances_trans"][[0, 2]]).max() == 0


def test_fixed_weight_form(S):
    d = R.make_inputs(3, 65, (2, 2, 2), seed=108, absent=(1,), field=False, settle=False)
    gap, real = R.blend_margins(d, 1)
    assert float(gap.min()) >= R.GAP and float(real.min()) >= R.GAP
    ref = R.run_framework(d, 1)
    bound, e32 = R.measured_bound(d, 1, ref)
    outs, grads, _ = run_fused(S, d, 1)
    worst = R.worst(outs, grads, ref)
    print(f"\nsmpl fixed weights: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused {worst:.3e}")
    assert worst <= bound, (worst, bound)


def test_border_safety_inside_a_nan_buffer(S):
    """The field tensors are views into the middle of a larger NaN-filled buffer and the points lie at and beyond every face: a
    neighbour fetched out of range, even with weight zero, would surface as NaN."""
    I, V, dhw = 2, 130, (3, 5, 7)
    d = R.make_inputs(I, V, dhw, seed=31)
    u = torch.tensor([[a, b, c] for a in (-1.5, -1.0, 1.0, 1.5) for b in (-1.5, -1.0, 1.0, 1.5) for c in (-1.5, -1.0, 1.0, 1.5)])
    u[:, 2] /= d["ratio"]
    d["means"].reshape(I, V, 3)[:, 4:4 + len(u)] = d["offset"] + d["scale"] * u
    for _ in range(20):      # the placed points keep their face coordinates; a row whose branch is too close to call moves in x or y only
        gap, real = R.blend_margins(d, 1)
        bad = (gap < R.GAP) | (real < R.GAP)
        if not bad.any():
            break
        d["means"].reshape(I, V, 3)[bad] += torch.tensor([0.37, -0.29, 0.0]) * d["scale"].expand(I, V, 3)[bad]
    assert not bad.any()
    n = R.normalize_coords(d["means"].reshape(I, V, 3).double(), d["offset"].double(), d["scale"].double(), d["ratio"], d["ratio_dim"])
    assert int((n[..., :2] == 1).any(-1).sum()) >= 8 and int((n[..., :2] == -1).any(-1).sum()) >= 8 and int((n.abs() > 1).any(-1).sum()) >= 50
    vol = I * 24 * dhw[0] * dhw[1] * dhw[2]
    views = []
    for k in ("voxel_base", "voxel_corr"):
        buf = torch.full((3 * vol,), float("nan"), device="cuda")
        buf[vol:2 * vol] = d[k].reshape(-1).cuda()
        views.append(buf[vol:2 * vol].view(d[k].shape))
    views[1].requires_grad_(True)
    ref = R.run_framework(d, 1)
    bound, e32 = R.measured_bound(d, 1, ref)
    outs, grads, _ = run_fused(S, d, 1, field_views=tuple(views))
    for k, v in list(outs.items()) + list(grads.items()):
        assert np.isfinite(v).all(), k
    worst = R.worst(outs, grads, ref)
    print(f"\nsmpl border: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused {worst:.3e}")
    assert worst <= bound, (worst, bound)


def test_poisoned_allocations_and_determinism(S):
    from tests import poison
    I, V = 3, 300
    d = R.make_inputs(I, V, (3, 5, 7), seed=77, absent=(1,))
    ref = R.run_framework(d, 1)
    bound, _ = R.measured_bound(d, 1, ref)
    plain_o, plain_g, _ = run_fused(S, d, 1)
    torch.cuda.synchronize()
    with poison.poisoned_allocations(True, name="smpl skin") as pz:      # (guards are compared on exit)
        got_o, got_g, _ = run_fused(S, d, 1)
        torch.cuda.synchronize()
        assert len(pz.records) >= 6
    for k, v in list(got_o.items()) + list(got_g.items()):
        t = torch.as_tensor(v)
        assert not bool(poison.holds_poison(t).any()), (k, int(poison.holds_poison(t).sum()))
    for k in ("wm", "wq"):
        assert np.array_equal(got_o[k].view(np.int32), plain_o[k].view(np.int32)), k
    for k in ("means", "quats") + POSE:      # bit-equal run to run; the field gradient (atomics) within the bound
        assert np.array_equal(got_g[k].view(np.int32), plain_g[k].view(np.int32)), k
    assert R.scaled_err(got_g["voxel_corr"], ref[1]["voxel_corr"]) <= bound and R.scaled_err(plain_g["voxel_corr"], ref[1]["voxel_corr"]) <= bound
    assert R.worst(got_o, got_g, ref) <= bound


def test_interpolated_form_forward_and_its_backward_raises(S, golden):
    d, z = golden
    f, s = int(z["interp_frame"]), int(z["stride"])
    ref, _ = R.run_framework(d, f, interpolate=True, grad=False)
    o32, _ = R.run_framework(d, f, torch.float32, interpolate=True, grad=False)
    bound = max(4 * max(R.scaled_err(o32[k], ref[k]) for k in ref), 1e-6)
    outs, _, loss = run_fused(S, d, f, interpolate=True, grad=False)
    errs = [R.scaled_err(outs[k], ref[k]) for k in ref] + [R.scaled_err(outs["wm"][::s], z[f"f{f}_wm"]), R.scaled_err(outs["wq"][::s], z[f"f{f}_wq"])]
    print(f"\nsmpl interpolated: bound {bound:.3e}, fused {max(errs):.3e}")
    assert max(errs) <= bound
    small = R.make_inputs(2, 9, (2, 2, 2), seed=5, F=5, frames=(2,))
    ts = {k: small[k].cuda().requires_grad_(True) for k in R.INPUTS}
    wm, wq = S.skin_transform(ts["means"], ts["quats"], ts["instances_quats"], ts["smpl_quats"], ts["instances_trans"], small["instances_fv"].cuda(),
                              2, voxel_corr=ts["voxel_corr"], interpolate=True, **R.template_kwargs(small, device="cuda"))
    with pytest.raises(RuntimeError, match="no gradient in the interpolated"):
        (wm.sum() + wq.sum()).backward()


def test_ball_form(S, golden):
    d, z = golden
    f, s = int(z["train_frames"][0]), int(z["stride"])
    ref = R.run_framework(d, f, ball=True)
    bound, e32 = R.measured_bound(d, f, ref, ball=True)
    outs, grads, _ = run_fused(S, d, f, ball=True)
    worst = max(R.worst(outs, grads, ref), R.scaled_err(outs["wm"][::s], z[f"f{f}_wm_ball"]))
    print(f"\nsmpl ball: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused {worst:.3e}")
    assert worst <= bound, (worst, bound)
    assert np.abs(grads["quats"]).max() == 0        # (the raw quaternions pass through get_gaussians untouched)


# ---- the install hook --------------------------------------------------------------------------------------------------------------
VIEW = torch.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 30.0], [0, 0, 0, 1]])
KS = torch.tensor([[60.0, 0, 48], [0, 60.0, 32], [0, 0, 1]])


def _cam():
    return SimpleNamespace(camtoworlds=torch.linalg.inv(VIEW).cuda()[None])


def _render_loss(gs):
    from bilateral_driving_amd import rendering
    img, alpha, _ = rendering.rasterization(gs["_means"], gs["_quats"], gs["_scales"], gs["_opacities"].squeeze(-1), gs["_rgbs"],
                                            VIEW.cuda()[None], KS.cuda()[None], 96, 64)
    wimg = torch.linspace(0, 1, img.numel(), device=img.device).reshape(img.shape)
    return (img * wimg).sum() + alpha.sum()


def _hook_inputs():
    d = R.make_inputs(3, 500, (3, 5, 7), seed=12, absent=(1,))
    d["instances_trans"] = d["instances_trans"] * 0.4
    return d


@pytest.mark.parametrize("ball", [False, True], ids=["ellipsoids", "balls"])
def test_install_hook_matches_framework_through_rasterization(S, ball):
    class Nodes(R.StandInNodes):
        pass
    d = _hook_inputs()

    def run(hooked):
        m = Nodes(d, "cuda", sh_degree=1, ball=ball)
        if hooked:
            S.install(Nodes)
        try:
            gs = m.get_gaussians(_cam())
            cache = dict(m._gs_cache)
            _render_loss(gs).backward()
        finally:
            if hooked:
                S.uninstall(Nodes)
        return gs, cache, {k: p.grad.clone() for k, p in m.parameters().items() if p.grad is not None}, m

    ref_gs, ref_cache, ref_g, _ = run(False)
    got_gs, got_cache, got_g, m = run(True)
    assert Nodes.get_gaussians is R.StandInNodes.get_gaussians
    assert m.filter_mask.all() and m.filter_mask.shape == (1500,)
    assert list(got_gs) == list(ref_gs) == ["_means", "_opacities", "_rgbs", "_scales", "_quats"] and list(got_cache) == list(ref_cache) == ["_scales"]
    for k in ref_gs:
        torch.testing.assert_close(got_gs[k], ref_gs[k], rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(got_cache["_scales"], ref_cache["_scales"], rtol=1e-5, atol=2e-5)
    assert sorted(got_g) == sorted(ref_g) and {"voxel_w_correction", "smpl_qauts", "instances_quats", "instances_trans"} <= set(ref_g)
    for k in ref_g:
        if ball and k == "_quats":      # an isotropic Gaussian does not depend on its rotation: both gradients are rounding residue
            assert float(ref_g[k].norm()) < 1e-5 * float(ref_g["_means"].norm()) and float(got_g[k].norm()) < 1e-5 * float(ref_g["_means"].norm())
            continue
        # both sides carry float32 rounding through the rasterizer's backward: relative to the gradient's norm, as the node classes' test
        assert float(ref_g[k].norm()) > 0, k
        assert float((got_g[k] - ref_g[k]).norm() / ref_g[k].norm()) < 2e-3, k


@pytest.mark.parametrize("what,msg", [
    ("nan_mean", "NaN detected in gaussian _means at step 7"),
    ("zero_point_quat", "NaN detected in gaussian _quats at step 7"),
    ("inf_trans", "Inf detected in gaussian _means at step 7"),
    ("nan_logit", "NaN detected in gaussian _opacities at step 7"),
    ("inf_scale", "Inf detected in gaussian _scales at step 7"),
])
def test_nonfinite_inputs_raise_the_reference_message(S, what, msg):
    class Nodes(R.StandInNodes):
        pass
    m = Nodes(_hook_inputs(), "cuda", sh_degree=1)
    m.step = 7
    with torch.no_grad():
        if what == "nan_mean":
            m._means[17, 1] = float("nan")
        elif what == "zero_point_quat":
            m._quats[5] = 0.0
        elif what == "inf_trans":
            m.instances_trans[m.cur_frame, 0] = float("inf")
        elif what == "nan_logit":
            m._opacities[9] = float("nan")
        else:
            m._scales[3, 0] = 200.0
    for hooked in (False, True):
        if hooked:
            S.install(Nodes)
        try:
            with pytest.raises(ValueError) as e:
                m.get_gaussians(_cam())
            assert str(e.value) == msg
        finally:
            if hooked:
                S.uninstall(Nodes)


def test_hook_returns_none_when_nobody_is_present(S):
    class Nodes(R.StandInNodes):
        pass
    m = Nodes(R.make_inputs(2, 9, (2, 2, 2), seed=2, absent=(0, 1)), "cuda")
    S.install(Nodes)
    try:
        assert m.get_gaussians(_cam()) is None and m.filter_mask.all()
    finally:
        S.uninstall(Nodes)
