"""Time transform of the periodic-vibration Gaussians on the MI355X (csrc/pvg.hip through bilateral_driving_amd/pvg.py): the fused op
against the reference-generated golden vectors (scripts/gen_golden_pvg.py) and against framework_transform in float64 on the CPU
(colours through oracle/gs_oracle.py's SH) over sizes, colour modes and extreme masks, within the measured bound of
tests/pvg_ref64.py; determinism; NaN / Inf in kept and dropped rows; and the install hook on a stand-in with the reference class's
attribute layout, through rasterization().  300000 rows are 1172 blocks: more than the 1024 block counts one scan pass covers."""
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from oracle import gs_oracle
from tests.pvg_ref64 import OUTS, RAW, SETTINGS, T, WEIGHTS, measured_bound, random_rows, run_framework, scaled_err, settle_clamp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pvg_time.npz")


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import pvg
    return pvg


def fused(P, d, setting, deg, grad=True):
    """Fused forward (+ backward of the weighted sum) of the CPU rows d -> ({out: array}, mask array, {raw: dense grad array})."""
    cur, dt, smooth = setting
    ts = {k: d[k].detach().cuda().float().requires_grad_(grad) for k in RAW}
    info = {}
    *outs, mask = P.time_transform(*[ts[k] for k in RAW], d["cam_pos"].cuda(), cur, dt, smooth, T, deg, info=info)
    assert mask.dtype == torch.bool and mask.shape == (d["means"].shape[0],) and info["M"] == int(mask.sum())
    g = {}
    if grad:
        loss = sum((o * d[w].cuda()[mask]).sum() for o, w in zip(outs, WEIGHTS))
        loss.backward()
        g = {k: t.grad.cpu().numpy() for k, t in ts.items()}
    return {k: o.detach().cpu().numpy() for k, o in zip(OUTS, outs)}, mask.cpu().numpy(), g


def compare(got, ref, bound, grads=RAW):
    (o, m, g), (ro, rm, rg) = got, ref
    np.testing.assert_array_equal(m, rm)
    for k in OUTS:
        assert o[k].shape == ro[k].shape, k
        assert scaled_err(o[k], ro[k]) <= bound, (k, scaled_err(o[k], ro[k]), bound)
    for k in grads:
        assert g[k].shape == rg[k].shape, k
        assert scaled_err(g[k], rg[k]) <= bound, (k, scaled_err(g[k], rg[k]), bound)
        assert np.abs(g[k][~m]).max(initial=0.0) == 0.0, k          # dropped rows: exactly zero


# ---- the reference's golden vectors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(3))
def test_fused_matches_reference_golden(P, i):
    z = np.load(GOLD)
    n = z["means"].shape[0]
    d = {k: torch.as_tensor(z[k]) for k in RAW[:7] + ("w_m", "w_o", "w_s", "w_q")}
    g_ = torch.Generator().manual_seed(i)
    d.update(features_dc=torch.rand(n, 3, generator=g_) - 0.5, features_rest=torch.zeros(n, 0, 3), cam_pos=torch.zeros(3),
             w_c=torch.randn(n, 3, generator=g_))
    setting = (float(z[f"s{i}_cur_time"]), float(z[f"s{i}_delta_t"]), bool(z[f"s{i}_in_smooth"]))
    bound, e32 = measured_bound(d, setting, 0)
    o, m, g = fused(P, d, setting, 0)
    np.testing.assert_array_equal(m, z[f"s{i}_mask"])                 # bit-equal
    worst = 0.0
    for k in ("means", "opacities", "scales", "quats"):
        worst = max(worst, scaled_err(o[k], z[f"s{i}_{k}"]))
    for k in RAW[:7]:
        worst = max(worst, scaled_err(g[k], z[f"s{i}_grad_{k}"]))
    print(f"\npvg golden s{i}: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, fused vs reference {worst:.3e}")
    assert worst <= bound, (worst, bound)
    # all nine gradients and the (sigmoid) colours against float64
    compare((o, m, g), run_framework(d, setting, 0), bound)


# ---- float64 over sizes and colour modes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 256, 257, 5000, 300000])
def test_fused_matches_float64_over_sizes(P, N):
    d = random_rows(N, 100 + N % 89)
    setting = SETTINGS[1 + N % 2]
    settle_clamp(d, setting, 3)
    ref = run_framework(d, setting, 3, sh=gs_oracle.spherical_harmonics)
    bound, _ = measured_bound(d, setting, 3, ref) if N else (1e-6, 0.0)
    got = fused(P, d, setting, 3)
    compare(got, ref, bound)
    ids = torch.nonzero(torch.as_tensor(got[1])).reshape(-1)
    if N:
        # compaction in the original order: row r of the outputs is the r-th kept row of the input (compare() holds all five tensors
        # to ref[mask]; here directly: the scales are an elementwise function of log_scales)
        assert scaled_err(got[0]["scales"], np.exp(d["log_scales"].double().numpy())[ids.numpy()]) <= bound
    for k in RAW:
        assert got[2][k].shape == tuple(d[k].shape)


@pytest.mark.parametrize("K,deg", [(16, 0), (16, 1), (16, 2), (16, 3), (1, 0), (4, 1), (9, 2)])
def test_colour_modes_match_the_oracle_sh(P, K, deg):
    d = random_rows(5000, 7 + K + deg, K=K)
    d["features_dc"] *= 2.0                                           # both clamp sides are reached
    setting = SETTINGS[0]
    settle_clamp(d, setting, deg)
    ref = run_framework(d, setting, deg, sh=gs_oracle.spherical_harmonics)
    bound, _ = measured_bound(d, setting, deg, ref)
    got = fused(P, d, setting, deg)
    compare(got, ref, bound)
    if K > 1:
        c = ref[0]["rgbs"]
        assert (c == 0.0).any() and (c == 1.0).any() and ((c > 0) & (c < 1)).any()
        nb = (deg + 1) ** 2
        assert np.abs(got[2]["features_rest"][:, nb - 1:]).max(initial=0.0) == 0.0     # bands beyond the degree in use
        assert np.abs(got[2]["features_rest"][:, :nb - 1]).max(initial=1.0) > 0.0


@pytest.mark.parametrize("what", ["all", "none"])
def test_extreme_masks(P, what):
    N = 1000
    d = random_rows(N, 5, spread=(5.0, 6.0) if what == "all" else (1e-4, 2e-4))
    if what == "none":
        d["taus"] += 10.0            # far from every cur_time: the marginal underflows to 0
    setting = SETTINGS[1]
    settle_clamp(d, setting, 3)
    ref = run_framework(d, setting, 3, sh=gs_oracle.spherical_harmonics)
    assert ref[1].sum() == (N if what == "all" else 0)
    bound, _ = measured_bound(d, setting, 3, ref)
    got = fused(P, d, setting, 3)
    compare(got, ref, bound)
    for k, w in zip(OUTS, (3, 1, 3, 3, 4)):
        assert got[0][k].shape == ((N if what == "all" else 0), w)
    for k in RAW:
        assert got[2][k].shape == tuple(d[k].shape)
        if what == "none":
            assert np.abs(got[2][k]).max() == 0.0


def test_two_runs_are_bit_identical(P):
    d = random_rows(300000, 9)
    a, b = fused(P, d, SETTINGS[2], 3), fused(P, d, SETTINGS[2], 3)
    for k in OUTS:
        assert np.array_equal(a[0][k], b[0][k]), k
    for k in RAW:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.abs(a[2]["taus"]).sum() > 0


# ---- a stand-in with the reference class's attribute layout -----------------------------------------------------------------------
class StandInPVG(nn.Module):
    """PeriodicVibrationGaussians' attribute layout (models/gaussians/pvg.py); get_gaussians is the rule of :374-425 on
    framework_transform, written from the contract."""

    def __init__(self, N, seed, sh_degree=3, scene=True):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        d = random_rows(N, seed, K=(sh_degree + 1) ** 2, settings=[(f / 39 * 0.78, 0, 0) for f in range(40)], spread=(0.1, 0.5))
        if scene:
            from tests.util import make_scene
            sc = make_scene(N, 96, 64, seed=seed)
            self.scene = sc
            d.update(means=sc["means"], quats=sc["quats"], log_scales=torch.log(sc["scales"]), logits=torch.logit(sc["opacities"]).reshape(N, 1))
            d["velocity"] = 0.05 * torch.randn(N, 3, generator=g)
        for a, k in dict(_means="means", _velocity="velocity", _taus="taus", _betas="betas", _opacities="logits", _scales="log_scales",
                         _quats="quats", _features_dc="features_dc", _features_rest="features_rest").items():
            setattr(self, a, nn.Parameter(d[k].float().cuda()))
        self.sh_degree, self.step, self.cur_frame, self.T = sh_degree, 7, 13, 0.2
        self.ctrl_cfg = SimpleNamespace(sh_degree_interval=2, enable_temporal_smoothing=True, smooth_probability=0.5, distribution_span=1.5)
        self.normalized_timestamps = torch.linspace(0, 1, 40).cuda()
        self.normalized_time_interval = 1.0 / 39
        self.train_time_scale = 0.02 / self.normalized_time_interval

    def get_gaussians(self, cam):
        from bilateral_driving_amd import gs_ops, pvg
        pvg._set_time(self)
        n = min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree)
        *dense, mask = pvg.framework_transform(self._means, self._velocity, self._taus, self._betas, self._opacities, self._scales,
                                               self._quats, self._features_dc, self._features_rest, cam.camtoworlds.data[..., :3, 3],
                                               float(self.cur_time), float(self.delta_t), self.in_smooth, self.T, n,
                                               sh=gs_ops.spherical_harmonics)
        self.filter_mask = mask
        gs = {k: v[mask] for k, v in zip(("_means", "_opacities", "_rgbs", "_scales", "_quats"), dense)}
        for k, v in gs.items():
            if torch.isnan(v).any():
                raise ValueError(f"NaN detected in gaussian {k} at step {self.step}")
            if torch.isinf(v).any():
                raise ValueError(f"Inf detected in gaussian {k} at step {self.step}")
        return gs


def _cam(m):
    return SimpleNamespace(camtoworlds=torch.linalg.inv(m.scene["viewmats"][0].cuda())[None])


def test_time_draw_follows_the_reference_rule(P):
    """cur_time, delta_t and in_smooth: random.random() < smooth_probability decides, Uniform(-bound, bound) is drawn only then, eval
    never smooths, and the same seeds give the same times."""
    from torch.distributions import uniform
    m = StandInPVG(500, 1)
    P.install(StandInPVG)
    try:
        seen = set()
        for seed in range(8):
            random.seed(seed)
            torch.manual_seed(seed)
            m.train()
            m.get_gaussians(_cam(m))
            random.seed(seed)
            torch.manual_seed(seed)
            scaled = m.normalized_timestamps[m.cur_frame] * m.train_time_scale
            if random.random() < 0.5:
                bound = m.normalized_time_interval * 1.5 * m.train_time_scale
                cur = scaled + uniform.Uniform(-bound, bound).sample((1,)).item()
                assert m.in_smooth is True and float(m.cur_time) == float(cur) and float(m.delta_t) == float(scaled - cur)
                assert abs(float(m.delta_t)) <= bound and float(m.delta_t) != 0.0
            else:
                assert m.in_smooth is False and float(m.cur_time) == float(scaled) and m.delta_t == 0.0
            seen.add(m.in_smooth)
            assert m.filter_mask.dtype == torch.bool and m.filter_mask.shape == (500,)
            m.eval()
            m.get_gaussians(_cam(m))
            assert m.in_smooth is False and m.delta_t == 0.0 and float(m.cur_time) == float(scaled)
        assert seen == {True, False}
    finally:
        P.uninstall(StandInPVG)


def test_install_hook_matches_framework_through_rasterization(P):
    from bilateral_driving_amd import rendering as R

    def run(hooked, seed):
        m = StandInPVG(3000, 11)
        random.seed(seed)
        torch.manual_seed(seed)
        if hooked:
            P.install(StandInPVG)
        try:
            gs = m.get_gaussians(_cam(m))
            img, alpha, _ = R.rasterization(gs["_means"], gs["_quats"], gs["_scales"], gs["_opacities"].squeeze(-1), gs["_rgbs"],
                                            m.scene["viewmats"].cuda(), m.scene["Ks"].cuda(), 96, 64, absgrad=True)
            wimg = torch.linspace(0, 1, img.numel(), device=img.device).reshape(img.shape)
            ((img * wimg).sum() + alpha.sum()).backward()
        finally:
            if hooked:
                P.uninstall(StandInPVG)
        return gs, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, m

    for seed in (0, 1, 2):       # (both branches of the smoothing draw are among these seeds)
        ref_gs, ref_g, rm = run(False, seed)
        got_gs, got_g, m = run(True, seed)
        assert list(got_gs) == list(ref_gs) == ["_means", "_opacities", "_rgbs", "_scales", "_quats"]
        assert m.in_smooth == rm.in_smooth and float(m.cur_time) == float(rm.cur_time) and float(m.delta_t) == float(rm.delta_t)
        assert torch.equal(m.filter_mask, rm.filter_mask) and 0 < int(m.filter_mask.sum()) < 3000
        for k in ref_gs:
            torch.testing.assert_close(got_gs[k], ref_gs[k], rtol=1e-5, atol=2e-5)
        assert sorted(got_g) == sorted(ref_g)
        for k in ("_taus", "_betas", "_velocity"):
            g = got_g[k]
            assert g.shape == getattr(m, k).shape and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0, k
        for k in ref_g:
            a, b = ref_g[k].double(), got_g[k].double()
            assert float((a - b).norm() / a.norm().clamp_min(1e-30)) < 2e-3, k


def test_install_and_uninstall_restore_the_original(P):
    class A(StandInPVG):
        pass
    orig = A.get_gaussians
    P.install(A)
    assert A.get_gaussians is P.pvg_get_gaussians and A._bds_reference_get_gaussians is orig
    P.install(A)                      # twice: the original is kept
    assert A._bds_reference_get_gaussians is orig
    P.uninstall(A)
    assert A.get_gaussians is orig


@pytest.mark.parametrize("what,msg", [
    ("nan_velocity_kept", "NaN detected in gaussian _means at step 7"),
    ("nan_velocity_dropped", None),
    ("big_log_scale_kept", "Inf detected in gaussian _scales at step 7"),
    ("zero_quat_kept", "NaN detected in gaussian _quats at step 7"),
    ("nan_tau", None),
    ("nan_sh_rest_kept", "NaN detected in gaussian _rgbs at step 7"),
    ("nan_sh_dc_kept", "NaN detected in gaussian _rgbs at step 7"),
    ("nan_sh_rest_dropped", None),
])
def test_nonfinite_values_follow_the_reference(P, what, msg):
    m = StandInPVG(2000, 3)
    m.eval()
    cam = _cam(m)
    m.get_gaussians(cam)
    kept = int(torch.nonzero(m.filter_mask)[5])
    dropped = int(torch.nonzero(~m.filter_mask)[5])
    with torch.no_grad():
        if what == "nan_velocity_kept":
            m._velocity[kept, 1] = float("nan")
        elif what == "nan_velocity_dropped":
            m._velocity[dropped, 1] = float("nan")
        elif what == "big_log_scale_kept":
            m._scales[kept, 2] = 100.0
        elif what == "zero_quat_kept":
            m._quats[kept] = 0.0
        elif what == "nan_sh_rest_kept":          # torch.clamp keeps a NaN colour: the clamp of the kernel must not turn it into 0
            m._features_rest[kept, 4, 1] = float("nan")
        elif what == "nan_sh_dc_kept":
            m._features_dc[kept, 2] = float("nan")
        elif what == "nan_sh_rest_dropped":
            m._features_rest[dropped, 4, 1] = float("nan")
        else:
            m._taus[kept] = float("nan")
    for hooked in (False, True):
        if hooked:
            P.install(StandInPVG)
        try:
            if msg is None:
                gs = m.get_gaussians(cam)
                assert all(bool(torch.isfinite(v).all()) for v in gs.values())
                assert not bool(m.filter_mask[dropped]) and (what != "nan_tau" or not bool(m.filter_mask[kept]))
            else:
                with pytest.raises(ValueError) as e:
                    m.get_gaussians(cam)
                assert str(e.value) == msg
        finally:
            if hooked:
                P.uninstall(StandInPVG)
