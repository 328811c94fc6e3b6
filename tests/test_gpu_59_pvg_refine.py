"""Density control of the periodic-vibration Gaussians on the device (bilateral_driving_amd.pvg_densify -> csrc/refine.hip pvg_* kernels
through the C ABI): the drop-in against the golden vectors of the reference's own refinement_after / after_train, the port against the
restatement (tests/pvg_refine_ref64.py) at sizes around a workgroup and across the count scan's 1024-segment boundary, the statistics,
and velocity_reg against float64 autograd.  Every call runs on poisoned, guard-banded allocations (tests/poison.py)."""
import functools
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import pvg_refine_ref64 as R
from tests.poison import holds_poison, poisoned_allocations

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "pvg_refine_step*.npz")))
IDS = [os.path.basename(f)[len("pvg_refine_"):-4] for f in FILES]
COPIED = ("_features_dc", "_features_rest", "_quats", "_velocity")      # rows that only move: bit-equal


def build_model(P, M, V, stats, ctrl, step, opt_cls, dev="cuda"):
    model = types.SimpleNamespace(ctrl_cfg=R.Cfg(ctrl), scene_scale=R.SCENE_SCALE, scene_origin=torch.tensor(R.ORIGIN, device=dev),
                                  num_train_images=R.NUM_TRAIN_IMAGES, step=step, class_prefix="Background#", T=ctrl["cycle_length"])
    groups = []
    for a, n in zip(R.ATTRS, R.GROUPS):
        prm = torch.nn.Parameter(P[a].clone().to(dev))
        setattr(model, a, prm)
        groups.append({"params": [prm], "lr": 1e-3, "eps": 1e-15, "weight_decay": 0, "name": model.class_prefix + n})
    opt = opt_cls(groups, lr=0.0, eps=1e-15)
    for a in R.ATTRS:
        opt.state[getattr(model, a)] = {"step": torch.tensor(1.0), "exp_avg": M[a].clone().to(dev), "exp_avg_sq": V[a].clone().to(dev)}
    for k in R.STATS:
        setattr(model, k, None if stats is None else stats[k].clone().to(dev))
    return model, opt


def printed(out):
    """{'current': n, 'Split': n, 'Dup': n, 'Cull': n, 'left': n} of the drop-in's prints (the reference's lines)."""
    got = {k: int(v) for k, v in re.findall(r"(Split|Dup|Cull): (\d+)", out)}
    got["current"] = int(re.search(r"Class Background# current points: (\d+) @ step", out).group(1))
    got["left"] = int(re.search(r"Class Background# left points: (\d+)", out).group(1))
    return got


def check_wiring(model, opt):
    for a, n in zip(R.ATTRS, R.GROUPS):
        prm = getattr(model, a)
        assert isinstance(prm, torch.nn.Parameter) and prm.is_cuda and not bool(holds_poison(prm).any()), a
        grp = [g for g in opt.param_groups if g["name"] == model.class_prefix + n][0]
        assert grp["params"][0] is prm and len(grp["params"]) == 1
        st = opt.state[prm]
        assert st["exp_avg"].shape == prm.shape and st["exp_avg_sq"].shape == prm.shape
        assert not bool(holds_poison(st["exp_avg"]).any()) and not bool(holds_poison(st["exp_avg_sq"]).any())
    assert len(opt.state) == len(R.ATTRS)                       # the old parameters' entries are gone
    assert all(getattr(model, k) is None for k in R.STATS)


@pytest.mark.parametrize("path", FILES, ids=IDS)
@pytest.mark.parametrize("fused", [False, True], ids=["torch_adam", "fused_adam"])
def test_drop_in_equals_reference_golden(path, fused, capsys):
    from bilateral_driving_amd.optim import FusedAdam
    from bilateral_driving_amd.pvg_densify import refinement_after
    z = np.load(path)
    ctrl = {k[5:]: z[k].item() for k in z.files if k.startswith("ctrl_")}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    P, M, V = ({a: t(z[pre + a]) for a in R.ATTRS} for pre in ("in", "in_m", "in_v"))
    stats = {k: t(z["in_" + k]) for k in R.STATS}
    step, samples = int(z["step"]), t(z["samples"])
    assert tuple(z["scene_origin"]) == R.ORIGIN
    model, opt = build_model(P, M, V, stats, ctrl, step, FusedAdam if fused else torch.optim.Adam)
    with poisoned_allocations(True, name=f"pvg refinement {os.path.basename(path)}"):
        refinement_after(model, step, opt, samples=samples)
        torch.cuda.synchronize()
    check_wiring(model, opt)
    for a in R.ATTRS:
        got, ref = getattr(model, a).detach().cpu().numpy(), z["out" + a]
        assert got.shape == ref.shape, a
        if a in COPIED:
            np.testing.assert_array_equal(got, ref, err_msg=a)
        else:                                                    # exp / log / rotation: last bits (tests/test_gpu_11_refine.py)
            err = np.abs(got - ref) / (3e-6 + 3e-6 * np.abs(ref))
            print(f"{a}: worst error / (3e-6 + 3e-6 |ref|) = {err.max(initial=0.0):.3f}")
            np.testing.assert_allclose(got, ref, rtol=3e-6, atol=3e-6, err_msg=a)
        st = opt.state[getattr(model, a)]
        np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), z["out_m" + a], err_msg="exp_avg" + a)
        np.testing.assert_array_equal(st["exp_avg_sq"].cpu().numpy(), z["out_v" + a], err_msg="exp_avg_sq" + a)
    # the printed counts are the reference's (restated in float64: no decision lies within 1e-4 of its threshold)
    _, _, _, c = R.refine(R.geometry_only(P), None, None, stats, step, ctrl, samples, torch.float64)
    got = printed(capsys.readouterr().out)
    want = {"current": int(z["N"]), "left": z["out_means"].shape[0]}
    if step > ctrl["warmup_steps"] and "parent" in c:
        want.update(Split=c["split"], Dup=c["dup"])
    if "culls" in c:
        want["Cull"] = c["cull"]
    assert got == want
    # the optimiser keeps working on all nine groups
    for a in R.ATTRS:
        getattr(model, a).grad = torch.full_like(getattr(model, a), 1e-3)
    opt.step()
    assert all(float(opt.state[getattr(model, a)]["step"]) == 2 for a in R.ATTRS)


# ---- the port against the restatement ------------------------------------------------------------------------------------------------
STEP = 3300


@functools.lru_cache(maxsize=None)
def case(N, no_time_split, kind="balanced"):
    """Inputs (SH degree 3) and the restated result, computed once: float64 and float32 on the geometry, and the row map (which input
    row every output row copies, and whether it is a child) for the arrays that only move."""
    ctrl = dict(R.CTRL, no_time_split=no_time_split, sh_degree=3)
    noise = R.seeded_noise(1000 + N)
    P, stats = R.synthetic(N, seed=N + 17 * no_time_split, K=16, special=min(N // 9, 2000))
    if kind == "nothing_split":
        stats["xys_grad_norm"].zero_(); stats["t_grad_accum"].zero_()
    if kind == "all_culled":
        P["_opacities"].fill_(-20.0)
    R.settle(P, stats, STEP, ctrl, noise)
    M, V = R.moments(P, N)
    G = R.geometry_only(P)
    o64, _, _, i64 = R.refine(G, None, None, stats, STEP, ctrl, noise, torch.float64)
    o32, _, _, i32 = R.refine(G, None, None, stats, STEP, ctrl, noise, torch.float32)
    assert all(i64[k] == i32[k] for k in ("split", "dup", "cull"))
    parent = i64.get("parent", torch.arange(N))
    keep = ~i64["culls"]
    rows, child = parent[keep], (torch.arange(parent.numel()) >= N)[keep]
    samples = i64.get("samples", torch.zeros(0, 4))
    pop = R.populations(P, stats, STEP, ctrl, noise)
    return ctrl, P, M, V, stats, samples, o64, o32, i64, rows, child, pop


CASES = [(1, True, "balanced"), (255, True, "balanced"), (257, False, "balanced"), (1000, True, "balanced"), (1000, False, "balanced"),
         (262_145, True, "balanced"), (262_145, False, "balanced"), (1000, True, "nothing_split"), (257, False, "all_culled")]


@pytest.mark.parametrize("N,no_time_split,kind", CASES, ids=[f"N{n}-{'nts' if t else 'ts'}-{k}" for n, t, k in CASES])
def test_port_equals_restatement(N, no_time_split, kind, capsys):
    from bilateral_driving_amd.pvg_densify import refinement_after
    ctrl, P, M, V, stats, samples, o64, o32, i64, rows, child, pop = case(N, no_time_split, kind)
    model, opt = build_model(P, M, V, stats, ctrl, STEP, torch.optim.Adam)
    with poisoned_allocations(True, name=f"pvg refinement N={N} {kind}"):
        refinement_after(model, STEP, opt, samples=samples)
        torch.cuda.synchronize()
    check_wiring(model, opt)
    n_out = rows.numel()
    got = printed(capsys.readouterr().out)
    assert got == {"current": N, "Split": i64["split"], "Dup": i64["dup"], "Cull": i64["cull"], "left": n_out}
    if kind == "nothing_split":
        assert i64["split"] == 0 and i64["dup"] == 0 and 0 < n_out < N
    if kind == "all_culled":
        assert n_out == 0 and i64["split"] > 0
    if kind == "balanced" and N >= 1000:
        assert all(pop[k] > 0 for k in R.POPULATIONS) and pop["mixed_fate_parents"] > 0, pop
    dev_rows, dev_child = rows.cuda(), child.cuda()
    for a in R.ATTRS:
        prm = getattr(model, a).detach()
        st = opt.state[getattr(model, a)]
        assert prm.shape == (n_out,) + tuple(P[a].shape[1:]), a
        # Adam moments: the parent's for an original, zeros for a child -- bit-equal
        shape = (-1,) + (1,) * (P[a].dim() - 1)
        for key, src in (("exp_avg", M[a]), ("exp_avg_sq", V[a])):
            want = src.cuda()[dev_rows] * (~dev_child).reshape(shape)
            assert torch.equal(st[key], want), (key, a)
        if a in COPIED:
            assert torch.equal(prm, P[a].cuda()[dev_rows]), a
            continue
        ref = o64[a].numpy()
        if a == "_opacities":
            assert torch.equal(prm, P[a].cuda()[dev_rows]), a     # no reset at this step: copied too
        elif a == "_means":
            # a child's mean is a sum of terms (scale x noise up to ~2000, rotated) that partly cancel: last-bit differences of exp
            # are relative to the terms, not to the result.  Bound: twice the float32 restatement's own distance from float64, + 1e-6
            e32 = R.scaled_err(o32[a].numpy(), ref)
            err = R.scaled_err(prm.cpu().numpy(), ref)
            print(f"_means: float32 restatement vs float64 {e32:.3e}, port {err:.3e}")
            assert err <= 2.0 * e32 + 1e-6, (err, e32)
        else:
            np.testing.assert_allclose(prm.cpu().numpy(), ref, rtol=3e-6, atol=3e-6, err_msg=a)


# ---- the core's compaction, with either class's rows ---------------------------------------------------------------------------------
TRAILING = {"_means": (3,), "_features_dc": (3,), "_features_rest": (8, 3), "_opacities": (1,), "_scales": (3,), "_quats": (4,), "_velocity": (3,),
            "_taus": (1,), "_betas": (1,)}


def byte_mask(kind, N):
    m = torch.zeros(N, dtype=torch.uint8)
    if kind == "all":
        m.fill_(1)
    elif kind == "last":
        m[-1] = 1
    elif kind == "half":
        m = (torch.rand(N, generator=torch.Generator().manual_seed(7 * N)) < 0.5).to(torch.uint8)
    return m


@pytest.mark.parametrize("kind", ["none", "all", "last", "half"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("rows", ["periodic", "vanilla_with_point_ids"])
def test_compact_rows_equals_boolean_mask_indexing(rows, N, kind):
    """``densify.compact_rows`` (one cull-only plan of 256-wide workgroups, one read-back, one move): every array of the layout, both
    Adam moments after a real step and ``point_ids`` are bit-equal to indexing with ``~mask``."""
    from bilateral_driving_amd.densify import PERIODIC_ROWS, VANILLA_ROWS, compact_rows
    lay = PERIODIC_ROWS if rows == "periodic" else VANILLA_ROWS
    g = torch.Generator().manual_seed(N)
    model = types.SimpleNamespace(class_prefix="Background#")
    groups = []
    for a, n in zip(lay.attrs, lay.groups):
        prm = torch.nn.Parameter(torch.randn((N,) + TRAILING[a], generator=g).cuda())
        setattr(model, a, prm)
        groups.append({"params": [prm], "lr": 1e-3, "name": model.class_prefix + n})
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for a in lay.attrs:
        getattr(model, a).grad = torch.randn((N,) + TRAILING[a], generator=g).cuda()
    opt.step()
    if lay.int64_columns:
        model.point_ids = (torch.arange(N, dtype=torch.int64)[:, None] * 1_000_003 - (1 << 40)).cuda()      # both 32-bit words in use
    before = {a: getattr(model, a) for a in lay.attrs}
    old = {a: p.detach().clone() for a, p in before.items()}
    old_m = {a: opt.state[p]["exp_avg"].clone() for a, p in before.items()}
    old_v = {a: opt.state[p]["exp_avg_sq"].clone() for a, p in before.items()}
    assert all(bool(old_m[a].any()) and bool(old_v[a].any()) for a in lay.attrs)
    old_ids = model.point_ids.clone() if lay.int64_columns else None
    mask = byte_mask(kind, N).cuda()
    keep = ~mask.bool()
    want = int(keep.sum())
    with poisoned_allocations(True, name=f"compact_rows {rows} N={N} {kind}"):
        n_left = compact_rows(model, opt, lay, mask)
        torch.cuda.synchronize()
    assert n_left == want == getattr(model, lay.attrs[0]).shape[0]
    for a, n in zip(lay.attrs, lay.groups):
        prm = getattr(model, a)
        assert (prm is before[a]) == (want == N), a                          # nothing culled: no parameter is replaced
        assert isinstance(prm, torch.nn.Parameter) and prm.shape == (want,) + TRAILING[a] and torch.equal(prm.detach(), old[a][keep]), a
        grp = [gr for gr in opt.param_groups if gr["name"] == model.class_prefix + n][0]
        assert len(grp["params"]) == 1 and grp["params"][0] is prm
        st = opt.state[prm]
        assert st["exp_avg"].shape == prm.shape and st["exp_avg_sq"].shape == prm.shape and float(st["step"]) == 1.0
        assert torch.equal(st["exp_avg"], old_m[a][keep]) and torch.equal(st["exp_avg_sq"], old_v[a][keep]), a
    assert len(opt.state) == len(lay.attrs)
    if lay.int64_columns:
        assert model.point_ids.dtype == torch.int64 and model.point_ids.shape == (want, 1) and torch.equal(model.point_ids, old_ids[keep])
    if want:
        for a in lay.attrs:
            getattr(model, a).grad = torch.zeros_like(getattr(model, a))
        opt.step()
        assert all(float(opt.state[getattr(model, a)]["step"]) == 2.0 for a in lay.attrs)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
def run_after_train(calls, last_size):
    from bilateral_driving_amd.pvg_densify import after_train
    N = calls[0]["filter_mask"].numel()
    model = types.SimpleNamespace(_means=torch.zeros(N, 3, device="cuda"), _taus=torch.nn.Parameter(torch.zeros(N, 1, device="cuda")),
                                  **{k: None for k in R.STATS})
    outs = []
    for c in calls:
        model.filter_mask = c["filter_mask"].cuda()
        model._taus.grad = c["taus_grad"].cuda()
        with poisoned_allocations(True, name="pvg after_train"):
            after_train(model, c["radii"].cuda(), c["xys_grad"].cuda(), last_size)
            torch.cuda.synchronize()
        outs.append({k: getattr(model, k).clone() for k in R.STATS})
    return outs


def check_stats(outs, want):
    for i, (o, w) in enumerate(zip(outs, want)):
        for k in R.STATS:
            assert o[k].dtype == torch.float32 and not bool(holds_poison(o[k]).any())
            ref = torch.as_tensor(w[k]).cuda()
            if k == "xys_grad_norm":        # the norm's sqrt and the running sum: tests/test_gpu_10_optim.py
                assert torch.allclose(o[k], ref, rtol=2e-7, atol=0), (i, k, float((o[k] - ref).abs().max()))
            else:
                assert torch.equal(o[k], ref), (i, k)


@pytest.mark.parametrize("N", [1, 257, 5000])
def test_statistics_equal_the_restatement(N):
    calls = R.stats_calls(N, seed=N)
    check_stats(run_after_train(calls, 960), R.run_stats(calls, 960))


def test_statistics_equal_reference_golden():
    z = np.load(os.path.join(GOLD, "pvg_refine_stats.npz"))
    calls = [{k: torch.from_numpy(z[f"c{i}_{k}"]) for k in ("filter_mask", "radii", "xys_grad", "taus_grad")} for i in range(3)]
    check_stats(run_after_train(calls, int(z["last_size"])), [{k: z[f"c{i}_out_{k}"] for k in R.STATS} for i in range(3)])


def test_statistics_scale_raw_gradients_and_take_float_radii():
    """The DensifyStats-style call: raw gradients with sx = width / 2, sy = height / 2, and radii given as floats."""
    from bilateral_driving_amd.pvg_densify import densify_stats
    c = R.stats_calls(777, seed=3)[0]
    W, H = 960, 640
    raw = c["xys_grad"] / torch.tensor([W / 2.0, H / 2.0])
    scaled = raw.clone()
    scaled[..., 0] *= W / 2.0
    scaled[..., 1] *= H / 2.0
    want = R.run_stats([dict(c, xys_grad=scaled)], W)[0]
    got = densify_stats(None, c["filter_mask"].cuda(), c["radii"].float().cuda(), raw.cuda(), c["taus_grad"].cuda(), W, sx=W / 2.0, sy=H / 2.0)
    check_stats([dict(zip(R.STATS, got))], [want])


# ---- velocity_reg --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 5000])
def test_velocity_reg_equals_float64_autograd(N):
    from bilateral_driving_amd.pvg_densify import velocity_reg
    vel, betas, mask, radii = R.velocity_rows(N, seed=N)
    m64, gv64, gb64 = R.velocity_reg_autograd(vel, betas, mask, radii, torch.float64)
    m32, gv32, gb32 = R.velocity_reg_autograd(vel, betas, mask, radii, torch.float32)
    e32 = max(R.scaled_err(m32.numpy(), m64.numpy()), R.scaled_err(gv32.numpy(), gv64.numpy()), R.scaled_err(gb32.numpy(), gb64.numpy()))
    bound = 2.0 * e32 + 1e-6       # twice the float32 restatement's own distance from float64, + 1e-6

    def run():
        v, b = vel.cuda().requires_grad_(True), betas.cuda().requires_grad_(True)
        with poisoned_allocations(True, name="pvg velocity_reg"):
            total, out = velocity_reg(v, b, mask.cuda(), radii.cuda(), R.T)
            s, count = out.tolist()
            loss = total / count
            loss.backward()
            torch.cuda.synchronize()
        return loss.detach(), v.grad, b.grad, s, count
    loss, gv, gb, s, count = run()
    seen = torch.zeros(N, dtype=torch.bool)
    seen[mask] = radii > 0
    assert count == int(seen.sum()) > 0
    assert abs(float(loss) - s / count) <= 2.0 ** -22 * abs(s / count)      # the float32 sum over the count: two roundings
    worst = max(R.scaled_err(loss.cpu().numpy(), m64.numpy()), R.scaled_err(gv.cpu().numpy(), gv64.numpy()), R.scaled_err(gb.cpu().numpy(), gb64.numpy()))
    print(f"velocity_reg N={N}: float32 autograd vs float64 {e32:.3e}, bound {bound:.3e}, port {worst:.3e}")
    assert worst <= bound, (worst, bound)
    assert gb.shape == betas.shape and bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gb).all()) and np.isfinite(float(loss))
    zero = (vel == 0).all(-1)
    outside = (~seen | zero).cuda()
    assert bool((gv[outside] == 0).all()) and bool((gb[outside] == 0).all())        # exact zeros outside the set and for a zero velocity
    if N >= 63:
        assert int((zero & seen).sum()) > 0 and int((~zero & seen).sum()) > 0 and bool((gv[(seen & ~zero).cuda()] != 0).any())
    again = run()
    assert torch.equal(again[0], loss) and torch.equal(again[1], gv) and torch.equal(again[2], gb) and again[3] == s     # bit-identical


def test_compute_reg_loss_adds_the_term_and_omits_it_when_nothing_is_visible():
    from bilateral_driving_amd import pvg_densify as PD

    class Base:
        def compute_reg_loss(self):
            return {"flatten": torch.tensor(1.0, device="cuda")}

    class Fake(Base):
        def compute_reg_loss(self):
            raise AssertionError("the class's own method must not run for GPU tensors")

    N = 300
    vel, betas, mask, radii = R.velocity_rows(N, seed=9)
    obj = Fake()
    obj._means = torch.zeros(N, 3, device="cuda")
    obj._velocity, obj._betas = vel.cuda().requires_grad_(True), betas.cuda().requires_grad_(True)
    obj.filter_mask, obj.T = mask.cuda(), R.T
    obj.reg_cfg = R.Cfg(velocity_reg=R.Cfg(w=0.01))
    PD.install(Fake)
    try:
        obj.cur_radii = radii.cuda()
        d = obj.compute_reg_loss()
        assert set(d) == {"flatten", "velocity_reg"}
        m64, gv64, _ = R.velocity_reg_autograd(vel, betas, mask, radii)
        m32, gv32, _ = R.velocity_reg_autograd(vel, betas, mask, radii, torch.float32)
        bound = 2.0 * max(R.scaled_err(m32.numpy(), m64.numpy()), R.scaled_err(gv32.numpy(), gv64.numpy())) + 1e-6      # as above
        assert R.scaled_err(float(d["velocity_reg"].detach()) / 0.01, float(m64)) <= bound
        d["velocity_reg"].backward()
        assert R.scaled_err(obj._velocity.grad.cpu().numpy() / 0.01, gv64.numpy()) <= bound
        obj.cur_radii = torch.zeros_like(radii).cuda()          # no row visible: the key is absent, as in the reference
        assert set(obj.compute_reg_loss()) == {"flatten"}
        obj.reg_cfg = R.Cfg()                                     # the term switched off
        assert set(obj.compute_reg_loss()) == {"flatten"}
    finally:
        PD.uninstall(Fake)
    assert "compute_reg_loss" in Fake.__dict__ and "_bds_reference_compute_reg_loss" not in Fake.__dict__
