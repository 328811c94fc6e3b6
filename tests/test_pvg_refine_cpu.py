"""Density control of the periodic-vibration Gaussians (bilateral_driving_amd/pvg_densify.py, csrc/refine.hip pvg_* kernels) on the
CPU: what the golden vectors of the reference's own refinement_after / after_train (scripts/gen_golden_pvg_refine.py) cover, the
restatement (tests/pvg_refine_ref64.py) against them, the device math on the host (tests/hostmath_pvg_refine_shim.hip) against the
float64 restatement, the new kernels' resources, argument validation of the C entries, and the install seam.

Measured on the 3000 shim rows (printed by the test; errors scaled by max(1, |reference|)): the float32 restatement differs from
float64 by at most 2.1e-5 on the split geometry (a child's mean is a sum of terms up to ~2000 that partly cancel), so the shim is
allowed twice that plus 1e-6 = 4.3e-5 and measures 2.1e-5, with either value of no_time_split; on the velocity term and its gradient
float32 autograd differs from float64 by 2.5e-7, the shim is allowed 1.5e-6 and measures 2.1e-7.  Every decision is identical."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import pvg_densify as PD
from tests import pvg_refine_ref64 as R
from tests.util import build_shim, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILES = sorted(glob.glob(os.path.join(GOLD, "pvg_refine_step*.npz")))
IDS = [os.path.basename(f)[len("pvg_refine_"):-4] for f in FILES]
COPIED = ("_features_dc", "_features_rest", "_quats", "_velocity")      # rows that only move: bit-equal; the others go through exp / log / rotation


def load(path):
    z = np.load(path)
    ctrl = {k[5:]: z[k].item() for k in z.files if k.startswith("ctrl_")}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    P = {a: t(z["in" + a]) for a in R.ATTRS}
    M = {a: t(z["in_m" + a]) for a in R.ATTRS}
    V = {a: t(z["in_v" + a]) for a in R.ATTRS}
    stats = {k: t(z["in_" + k]) for k in R.STATS}
    return z, ctrl, P, M, V, stats


def test_goldens_cover_the_contract():
    assert len(FILES) == 8
    limit = max(os.path.getsize(f) for f in glob.glob(os.path.join(GOLD, "refine_*.npz")))
    seen = set()
    for path, case in zip(FILES, IDS):
        z, ctrl, P, M, V, stats = load(path)
        step, N = int(z["step"]), int(z["N"])
        assert os.path.getsize(path) <= limit
        assert 600 <= N <= 800 and P["_features_rest"].shape == (N, 8, 3) and ctrl["cycle_length"] == 0.2 == R.T
        assert tuple(z["scene_origin"]) == R.ORIGIN and np.abs(z["scene_origin"]).min() > 0 and float(z["scene_scale"]) == R.SCENE_SCALE
        for k, v in R.CTRL.items():
            if k not in ("no_time_split", "densify_until_num_points"):
                assert ctrl[k] == v, k
        samples = torch.from_numpy(z["samples"])
        sch = PD.schedule(step, R.Cfg(ctrl), int(z["num_train_images"]), N)
        assert float(R.margins(P, stats, step, ctrl, samples).min()) >= R.BAND       # no row's fate hangs on the last bit
        pop = R.populations(P, stats, step, ctrl, samples)
        if sch["do_densify"]:
            for k in R.POPULATIONS:
                assert pop[k] > 0 or (k == "split_screen_only" and not sch["by_screen"]), (case, k)
            if sch["cull_by_scale"]:
                assert pop["mixed_fate_parents"] > 0, case      # two children of one parent with different cull decisions
            assert samples.shape == (2 * int(sum(pop[k] for k in ("split_xyz_only", "split_t_only", "split_both", "split_screen_only"))), 4)
            assert (P["_velocity"] == 0).all(-1).any()
        else:
            assert samples.shape[0] == 0
        seen.add((sch["do_densify"], sch["do_cull"], sch["by_screen"], sch["cull_by_scale"], sch["do_reset"], bool(ctrl["no_time_split"])))
        if case == "step3300_full":
            assert ctrl["densify_until_num_points"] < N and not sch["do_densify"] and 0 < z["out_means"].shape[0] < N
    # densify + full cull, densify + opacity cull, densify past the screen tests, cull only (by count and by step), reset; both time-split values
    assert len(seen) == 8
    z = np.load(os.path.join(GOLD, "pvg_refine_stats.npz"))
    for i in range(3):
        r = z[f"c{i}_radii"]
        assert 0 < int((r == 0).sum()) < r.size < int(z["N"]) and int(z[f"c{i}_filter_mask"].sum()) == r.size


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_float32_restatement_matches_reference_golden(path):
    z, ctrl, P, M, V, stats = load(path)
    step = int(z["step"])
    samples = torch.from_numpy(z["samples"])
    oP, oM, oV, counts = R.refine(P, M, V, stats, step, ctrl, samples, torch.float32)
    for a in R.ATTRS:
        got, ref = oP[a].numpy(), z["out" + a]
        assert got.shape == ref.shape, a
        if a in COPIED:
            np.testing.assert_array_equal(got, ref, err_msg=a)
        else:
            np.testing.assert_allclose(got, ref, rtol=3e-6, atol=3e-6, err_msg=a)      # tests/test_gpu_11_refine.py
        np.testing.assert_array_equal(oM[a].numpy(), z["out_m" + a], err_msg="exp_avg" + a)
        np.testing.assert_array_equal(oV[a].numpy(), z["out_v" + a], err_msg="exp_avg_sq" + a)
    # the float64 restatement takes the same decisions
    dP, _, _, c64 = R.refine(R.geometry_only(P), None, None, stats, step, ctrl, samples, torch.float64)
    assert dP["_means"].shape == z["out_means"].shape and all(c64[k] == counts[k] for k in ("split", "dup", "cull"))


def test_restated_statistics_match_reference_golden():
    z = np.load(os.path.join(GOLD, "pvg_refine_stats.npz"))
    calls = [{k: torch.from_numpy(z[f"c{i}_{k}"]) for k in ("filter_mask", "radii", "xys_grad", "taus_grad")} for i in range(3)]
    outs = R.run_stats(calls, int(z["last_size"]))
    for i, o in enumerate(outs):
        for k in R.STATS:
            np.testing.assert_array_equal(o[k].numpy(), z[f"c{i}_out_{k}"], err_msg=f"{i} {k}")
    assert (z["c2_out_vis_counts"] > 1).any() and (z["c0_out_vis_counts"] == 1).all()


def test_cpu_tensors_raise():
    P, stats = R.synthetic(20, 1)
    o = torch.tensor(R.ORIGIN)
    c = R.stats_calls(20, 2)[0]
    with pytest.raises(L.BdsError):
        PD.densify_stats(None, c["filter_mask"], c["radii"], c["xys_grad"], c["taus_grad"], 960)
    with pytest.raises(L.BdsError):
        PD.refine_plan(*[stats[k] for k in R.STATS], P["_scales"], P["_betas"], P["_means"], o, 30.0, grad_thresh=2e-4, t_grad_thresh=2e-3,
                       size_thresh=0.3, t_size_thresh=0.01, split_by_screen=True, split_screen_size=0.05)
    with pytest.raises(L.BdsError):
        PD.cull_mask(P["_opacities"], P["_scales"], P["_means"], None, o, 30.0, cull_alpha_thresh=0.005, cull_by_scale=True, cull_scale_thresh=15.0,
                     cull_by_screen=False, cull_screen_size=0.15)
    with pytest.raises(L.BdsError):
        PD.velocity_reg(P["_velocity"], P["_betas"], c["filter_mask"], c["radii"], R.T)


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("pvg_refine")
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    h.hm_pvg_refine_decide.argtypes = [ci, cf, cf, cf, cf, ci, cf, cf] + [vp] * 10
    h.hm_pvg_refine_split.argtypes = [ci, ci, ci, cd] + [vp] * 13
    h.hm_pvg_cull.argtypes = [ci, cf, ci, cf, ci, cf, cf] + [vp] * 6
    h.hm_pvg_grad_norm.argtypes = [ci, cf, cf, vp, vp]
    h.hm_pvg_velocity.argtypes = [ci, cd, cf] + [vp] * 5
    return h


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.contiguous().data_ptr()


@pytest.mark.parametrize("no_time_split", [True, False], ids=["nts", "ts"])
def test_host_math_matches_float64_restatement(shim, no_time_split):
    n, step, samps = 3000, 3300, 2
    ctrl = dict(R.CTRL, no_time_split=no_time_split)
    cfg = R.Cfg(ctrl)
    noise = R.seeded_noise(77)
    P, stats = R.synthetic(n, seed=31)
    R.settle(P, stats, step, ctrl, noise)
    G = {k: v.contiguous() for k, v in R.geometry_only(P).items()}
    _, _, _, i64 = R.refine(G, None, None, stats, step, ctrl, noise, torch.float64)
    _, _, _, i32 = R.refine(G, None, None, stats, step, ctrl, noise, torch.float32)
    origin = np.array(R.ORIGIN, np.float32)
    flags, kinds = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    shim.hm_pvg_refine_decide(n, cfg.densify_grad_thresh, cfg.densify_t_grad_thresh, cfg.densify_size_thresh * R.SCENE_SCALE,
                              cfg.densify_t_size_thresh, 1, cfg.split_screen_size, R.SCENE_SCALE, _p(origin), *[_p(stats[k]) for k in R.STATS],
                              _p(G["_scales"]), _p(G["_betas"]), _p(G["_means"]), _p(flags), _p(kinds))
    d = i64["decisions"]
    split, dup = d["splits"].numpy(), d["dups"].numpy()
    np.testing.assert_array_equal(flags & 1, split)                       # decisions: identical
    np.testing.assert_array_equal(flags >> 1, dup)
    np.testing.assert_array_equal(kinds & 1, d["small_xyz"].numpy())
    np.testing.assert_array_equal(kinds >> 1, d["small_t"].numpy())
    assert (split & dup).sum() > 100 and split.sum() > 500 and dup.sum() > 300
    # every split parent's children, in the reference's layout
    idx = np.nonzero(split)[0]
    S = idx.size
    smp = np.zeros((n, samps, 4), np.float32)
    samples = i64["samples"].numpy()
    for s in range(samps):
        smp[idx, s] = samples[s * S:(s + 1) * S]
    shrunk, c_scale = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    c_beta, c_means, c_taus = np.zeros((n, 1), np.float32), np.zeros((n, samps, 3), np.float32), np.zeros((n, samps, 1), np.float32)
    shim.hm_pvg_refine_split(n, samps, int(no_time_split), R.T, _p(kinds), _p(smp), *[_p(G[k]) for k in ("_means", "_quats", "_scales", "_velocity", "_taus", "_betas")],
                             _p(shrunk), _p(c_scale), _p(c_beta), _p(c_means), _p(c_taus))
    parent_scale = np.where(split[:, None], shrunk, G["_scales"].numpy())
    di = np.nonzero(dup)[0]
    pre = {"_means": np.concatenate([G["_means"].numpy()] + [c_means[idx, s] for s in range(samps)] + [G["_means"].numpy()[di]]),
           "_scales": np.concatenate([parent_scale] + [c_scale[idx]] * samps + [parent_scale[di]]),
           "_taus": np.concatenate([G["_taus"].numpy()] + [c_taus[idx, s] for s in range(samps)] + [G["_taus"].numpy()[di]]),
           "_betas": np.concatenate([G["_betas"].numpy()] + [c_beta[idx]] * samps + [G["_betas"].numpy()[di]])}
    e32 = max(R.scaled_err(i32["pre_cull"][k].numpy(), i64["pre_cull"][k].numpy()) for k in pre)
    worst = max(R.scaled_err(pre[k], i64["pre_cull"][k].numpy()) for k in pre)
    bound = 2.0 * e32 + 1e-6
    print(f"\npvg refine shim ({'nts' if no_time_split else 'ts'}): float32 restatement vs float64 {e32:.3e}, bound {bound:.3e}, shim {worst:.3e}")
    assert worst <= bound, (worst, bound)
    # the cull of the new rows, children by their own means
    m = pre["_means"].shape[0]
    logits = np.ascontiguousarray(i64["pre_cull"]["_opacities"].numpy().astype(np.float32))
    m2d = np.ascontiguousarray(i64["pre_cull_max_2Dsize"].numpy().astype(np.float32))
    mask = np.zeros(m, np.uint8)
    shim.hm_pvg_cull(m, cfg.cull_alpha_thresh, 1, cfg.cull_scale_thresh * R.SCENE_SCALE, 1, cfg.cull_screen_size, R.SCENE_SCALE, _p(origin),
                     _p(logits), _p(np.ascontiguousarray(pre["_scales"])), _p(np.ascontiguousarray(pre["_means"])), _p(m2d), _p(mask))
    np.testing.assert_array_equal(mask, i64["culls"].numpy())
    fate = i64["culls"][n:n + samps * S].reshape(samps, S)
    assert int((fate.any(0) & ~fate.all(0)).sum()) > 0 and 0 < mask.sum() < m


def test_host_velocity_term_matches_float64_autograd(shim):
    n = 4000
    vel, betas, _, _ = R.velocity_rows(n, 5)
    every, radii = torch.ones(n, dtype=torch.bool), torch.ones(n, dtype=torch.int32)
    sum64 = lambda dt: tuple(x * n if i else x for i, x in enumerate(R.velocity_reg_autograd(vel, betas, every, radii, dt)))      # mean -> sum
    (_, gv64, gb64), (_, gv32, gb32) = sum64(torch.float64), sum64(torch.float32)
    n64 = (vel.double() * torch.exp(-0.5 * (torch.exp(betas.double()) / R.T))).norm(dim=-1)
    n32 = (vel * torch.exp(-0.5 * (torch.exp(betas) / R.T))).norm(dim=-1)
    norm, gv, gb = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 1), np.float32)
    shim.hm_pvg_velocity(n, R.T, 1.0, _p(vel), _p(betas), _p(norm), _p(gv), _p(gb))
    e32 = max(R.scaled_err(n32.numpy(), n64.numpy()), R.scaled_err(gv32.numpy(), gv64.numpy()), R.scaled_err(gb32.numpy(), gb64.numpy()))
    worst = max(R.scaled_err(norm, n64.numpy()), R.scaled_err(gv, gv64.numpy()), R.scaled_err(gb, gb64.numpy()))
    bound = 2.0 * e32 + 1e-6
    print(f"\npvg velocity shim: float32 autograd vs float64 {e32:.3e}, bound {bound:.3e}, shim {worst:.3e}")
    assert worst <= bound, (worst, bound)
    zero = (vel == 0).all(-1).numpy()
    assert zero.sum() > 1000 and np.isfinite(gv).all() and np.isfinite(gb).all()
    assert (gv[zero] == 0).all() and (gb[zero] == 0).all() and (norm[zero] == 0).all()      # a zero velocity: exact zeros, no NaN
    g = torch.randn(50, 2)
    out = np.zeros(50, np.float32)
    shim.hm_pvg_grad_norm(50, 1.0, 1.0, _p(g), _p(out))
    np.testing.assert_allclose(out, g.norm(dim=-1).numpy(), rtol=2e-7, atol=0)


# ---- resources and argument validation ---------------------------------------------------------------------------------------------
KERNELS = ("pvg_refine_flags_kernel", "pvg_refine_geometry_kernel", "pvg_cull_mask_kernel", "pvg_mask_count_kernel", "pvg_mask_scan_kernel",
           "pvg_stats_kernel", "pvg_velocity_reg_fwd_kernel", "pvg_velocity_reg_final_kernel", "pvg_velocity_reg_bwd_kernel")


def test_new_kernels_use_no_scratch():
    res = kernel_resources("refine.hip")
    for prefix in KERNELS:
        ks = [k for k in res if k.startswith(prefix)]
        assert len(ks) == 1, (prefix, list(res))
        r = res[ks[0]]
        print(f"\n{prefix}: {r}")
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= 8, (prefix, r)


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    fake = 1 << 20      # never dereferenced: every case fails its argument check first
    E = L.BDS_EINVAL
    tb = lambda n: lib.bds_pvg_mask_temp_bytes(n)

    def stats(N=100, M=50, p=fake, temp=fake, nb=1 << 20, last=960):
        return lib.bds_pvg_densify_stats(N, M, p, fake, 1.0, 1.0, fake, 0, fake, last, 1, fake, fake, fake, p, temp, nb, None)

    def plan(N=100, p=fake, temp=fake, nb=1 << 20, ranks=fake, scale=30.0):
        return lib.bds_pvg_refine_plan(N, *([p] * 8), scale, 2e-4, 2e-3, 0.3, 0.01, 1, 0.05, fake, fake, ranks, fake, temp, nb, None)

    def geom(N=100, samps=2, T=0.2, p=fake, out=fake):
        return lib.bds_pvg_refine_geometry(N, samps, 1, T, *([fake] * 5), *([p] * 6), *([out] * 4), None)

    def cull(N=100, n_old=60, p=fake, m2d=fake, mask=fake, scale=30.0):
        return lib.bds_pvg_cull_mask(N, n_old, p, p, p, m2d, fake, scale, 0.005, 1, 15.0, 1, 0.15, mask, None)

    def vfwd(N=100, M=50, T=0.2, p=fake, out=fake, temp=fake, nb=1 << 20):
        return lib.bds_pvg_velocity_reg_fwd(N, M, T, p, fake, 0, p, fake, fake, out, temp, nb, None)

    def vbwd(N=100, T=0.2, p=fake, g=fake):
        return lib.bds_pvg_velocity_reg_bwd(N, T, fake, fake, p, p, g, g, None)

    for f in (stats, plan, geom, cull, vfwd, vbwd):
        assert f(N=-1) == E and f(p=None) == E, f.__name__
    assert stats(M=101) == E and stats(M=-1) == E and stats(last=0) == E and stats(temp=None) == E and stats(nb=tb(100) - 1) == E
    assert vfwd(M=101) == E and vfwd(T=0.0) == E and vfwd(out=None) == E and vfwd(temp=None) == E and vfwd(nb=tb(100) - 1) == E
    assert plan(temp=None) == E and plan(nb=lib.bds_refine_plan_temp_bytes(100) - 1) == E and plan(ranks=fake + 4) == E and plan(scale=0.0) == E
    assert geom(samps=0) == E and geom(samps=-1) == E and geom(T=0.0) == E and geom(out=None) == E
    assert cull(n_old=101) == E and cull(m2d=None) == E and cull(mask=None) == E and cull(scale=-1.0) == E
    assert vbwd(T=-0.2) == E and vbwd(g=None) == E
    # nothing to do: no pointer is needed, nothing is launched
    assert stats(N=0, M=0, p=None, temp=None, nb=0) == L.BDS_OK and geom(N=0, p=None, out=None) == L.BDS_OK
    assert cull(N=0, n_old=0, p=None, mask=None) == L.BDS_OK and vbwd(N=0, p=None, g=None) == L.BDS_OK
    assert tb(0) == 0 and tb(1) >= 3 * 2 * 4 and tb(3 * 10 ** 6) >= 3 * 4 * (3 * 10 ** 6 // 256 + 1)


# ---- the seam ----------------------------------------------------------------------------------------------------------------------
def test_install_and_uninstall_restore_the_class():
    from bilateral_driving_amd import pvg

    class Base:
        def compute_reg_loss(self):
            return {"base": 1.0}

    class Fake(Base):
        _means = torch.zeros(3, 3)      # CPU tensors keep the class's own methods

        def after_train(self, radii, xys_grad, last_size):
            return ("own after_train", last_size)

        def refinement_after(self, step, optimizer):
            return ("own refinement_after", step)

        def compute_reg_loss(self):
            return dict(super().compute_reg_loss(), own=2.0)

        def get_gaussians(self, cam):
            return "own get_gaussians"

    before = dict(Fake.__dict__)
    PD.install(Fake)
    assert Fake.after_train is PD.after_train and Fake.refinement_after is PD.refinement_after
    assert Fake.compute_reg_loss is not before["compute_reg_loss"]
    assert Fake._bds_reference_after_train is before["after_train"] and Fake._bds_reference_compute_reg_loss is before["compute_reg_loss"]
    obj = Fake()
    assert obj.after_train(None, None, 7) == ("own after_train", 7) and obj.refinement_after(9, None) == ("own refinement_after", 9)
    assert obj.compute_reg_loss() == {"base": 1.0, "own": 2.0}
    pvg.install(Fake)                       # composes with the time transform's seam, in either order of removal
    assert Fake.get_gaussians is pvg.pvg_get_gaussians and Fake.after_train is PD.after_train
    PD.uninstall(Fake)
    assert Fake.get_gaussians is pvg.pvg_get_gaussians and Fake.after_train is before["after_train"]
    pvg.uninstall(Fake)
    assert dict(Fake.__dict__) == before
    PD.install(Fake); PD.install(Fake)      # a second install changes nothing more
    PD.uninstall()
    assert dict(Fake.__dict__) == before
