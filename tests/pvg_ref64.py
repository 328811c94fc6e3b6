"""Shared by tests/test_pvg_cpu.py and tests/test_gpu_37_pvg.py (test infrastructure): random parameter rows for the periodic-vibration
Gaussians' time transform, ``bilateral_driving_amd.pvg.framework_transform`` evaluated with autograd in a chosen precision, and the
error bound both files use.

The bound is MEASURED, not fixed: the worst per-element error of framework_transform in float32 on the CPU against itself in float64
over the same rows (outputs and gradients; each error divided by max(1, |reference|)), times 4 -- the factor covers a different but
equally accurate exp / sin and FMA contraction -- with a floor of 1e-6."""
import numpy as np
import torch

from bilateral_driving_amd.pvg import framework_transform, sh_colors

RAW = ("means", "velocity", "taus", "betas", "logits", "log_scales", "quats", "features_dc", "features_rest")
OUTS = ("means", "opacities", "rgbs", "scales", "quats")
WEIGHTS = ("w_m", "w_o", "w_c", "w_s", "w_q")
T, SCALE = 0.2, 0.78                       # the shipped schedule: cycle_length, train_time_scale (time_interval 0.02, 40 timestamps)
SETTINGS = ((0.31, 0.0, False), (0.417, -0.017, True), (0.637, 0.023, True))      # cur_time, delta_t, in_smooth
BAND = 1e-4


def marg64(taus, betas, cur):
    return torch.exp(-0.5 * (taus.double() - cur) ** 2 / torch.exp(betas.double()) ** 2)


def random_rows(n, seed, K=16, settings=SETTINGS, spread=(0.03, 0.4)):
    """Float32 parameters on the CPU: about half the rows kept at each setting; no row within BAND of the threshold at any of them."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    d = dict(means=(r(n, 3) - 0.5) * 40, velocity=torch.randn(n, 3, generator=g) * 2, taus=r(n, 1) * SCALE,
             betas=torch.log(spread[0] * (spread[1] / spread[0]) ** r(n, 1)), logits=torch.randn(n, 1, generator=g) * 2,
             log_scales=r(n, 3) * 4 - 4, quats=torch.randn(n, 4, generator=g), features_dc=(r(n, 3) - 0.5) * 3,
             features_rest=torch.randn(n, K - 1, 3, generator=g) * 0.5, cam_pos=torch.tensor([1.5, -2.0, 0.7]))
    for _ in range(100):
        near = torch.zeros(n, dtype=torch.bool)
        for cur, _dt, _sm in settings:
            near |= ((marg64(d["taus"], d["betas"], cur) / 0.05 - 1).abs() < BAND).reshape(-1)
        if not near.any():
            break
        d["taus"][near] = r(int(near.sum()), 1) * SCALE
    assert not near.any()
    d.update(w_m=torch.randn(n, 3, generator=g), w_o=torch.randn(n, 1, generator=g), w_c=torch.randn(n, 3, generator=g),
             w_s=torch.randn(n, 3, generator=g), w_q=torch.randn(n, 4, generator=g))
    return d


def settle_clamp(d, setting, deg):
    """Move (in place, band 0 by 0.01) the rows whose colour lies within BAND of a clamp edge in float64: like the keep threshold, the
    clamp's pass / block decision then does not hang on the last bits, and no row is excluded from the gradient comparison."""
    if d["features_rest"].shape[1] == 0 or d["means"].shape[0] == 0:
        return d
    cur, dt, smooth = setting
    for _ in range(50):
        ts = [d[k].double() for k in RAW]
        m = framework_transform(*ts, d["cam_pos"].double(), cur, dt, smooth, T, deg)[0]
        dirs = m - d["cam_pos"].double()
        x = sh_colors(deg, dirs / dirs.norm(dim=-1, keepdim=True), torch.cat((ts[7][:, None, :], ts[8]), 1)) + 0.5
        near = ((x.abs() < BAND) | ((x - 1).abs() < BAND)).any(-1)
        if not near.any():
            return d
        d["features_dc"][near] += 0.01
    raise AssertionError("colours did not settle")


def run_framework(d, setting, deg, dtype=torch.float64, sh=None, grad=True):
    """framework_transform + the five mask gathers on the CPU in ``dtype`` -> ({out: [M,.] array}, mask array, {raw: dense grad})."""
    cur, dt, smooth = setting
    ts = {k: d[k].detach().cpu().to(dtype).clone().requires_grad_(grad) for k in RAW}
    *dense, mask = framework_transform(*[ts[k] for k in RAW], d["cam_pos"].cpu().to(dtype), cur, dt, smooth, T, deg, sh=sh)
    outs = {k: v[mask] for k, v in zip(OUTS, dense)}
    grads = {}
    if grad:
        loss = sum((outs[k] * d[w].cpu().to(dtype)[mask]).sum() for k, w in zip(OUTS, WEIGHTS))
        loss.backward()
        grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in ts.items()}
    return {k: v.detach().numpy() for k, v in outs.items()}, mask.numpy(), grads


def scaled_err(got, ref) -> float:
    """Worst per-element |got - ref| / max(1, |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max(initial=0.0))


def measured_bound(d, setting, deg, ref=None):
    """(bound, float32-vs-float64 figure) for rows d at one setting; ``ref``: a float64 run_framework result to reuse."""
    o64, m64, g64 = ref if ref is not None else run_framework(d, setting, deg)
    o32, m32, g32 = run_framework(d, setting, deg, torch.float32)
    assert (m32 == m64).all()
    e32 = max([scaled_err(o32[k], o64[k]) for k in OUTS] + [scaled_err(g32[k], g64[k]) for k in RAW])
    return max(4.0 * e32, 1e-6), e32
