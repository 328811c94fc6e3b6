"""Time transform of the periodic-vibration Gaussians (bilateral_driving_amd/pvg.py, csrc/pvg.hip) on the CPU: the float64 restatement
against the golden vectors produced by the reference's own PeriodicVibrationGaussians properties (scripts/gen_golden_pvg.py), the
device math on the host (tests/hostmath_pvg_shim.hip) against float64 autograd within the measured bound of tests/pvg_ref64.py, the
new kernels' resources, and argument validation of the C entries.

Measured on the 4000 shim rows (printed by the test): float32 framework ops against float64 differ by at most 5.6e-6 without and
4.4e-6 with smoothing (scaled by max(1, |reference|); the sine's argument of up to 25 rad carries its float32 rounding into the tau
gradient), so the shim is allowed 2.2e-5 and 1.7e-5; it measures 5.7e-6 and 4.4e-6."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import pvg
from tests.pvg_ref64 import BAND, OUTS, RAW, SETTINGS, T, marg64, measured_bound, random_rows, run_framework, scaled_err, settle_clamp
from tests.util import build_shim, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pvg_time.npz")
GOLD_RAW = RAW[:7]


def test_golden_covers_the_contract():
    z = np.load(GOLD)
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "node_pose_train.npz"))
    assert float(z["T"]) == 0.2
    smooth = [bool(z[f"s{i}_in_smooth"]) for i in range(3)]
    dts = [float(z[f"s{i}_delta_t"]) for i in range(3)]
    assert not smooth[0] and dts[0] == 0.0 and smooth[1] and dts[1] < 0 and smooth[2] and dts[2] > 0
    for i in range(3):
        frac = z[f"s{i}_mask"].mean()
        assert 0.4 <= frac <= 0.7
        m = marg64(torch.as_tensor(z["taus"]), torch.as_tensor(z["betas"]), float(z[f"s{i}_cur_time"]))
        assert float((m / 0.05 - 1).abs().min()) >= BAND        # no row's decision hangs on the last bits of exp


@pytest.mark.parametrize("i", range(3))
def test_float64_restatement_matches_reference_golden(i):
    z = np.load(GOLD)
    n = z["means"].shape[0]
    d = {k: torch.as_tensor(z[k]) for k in GOLD_RAW + ("w_m", "w_o", "w_s", "w_q")}
    d.update(features_dc=torch.zeros(n, 3), features_rest=torch.zeros(n, 0, 3), cam_pos=torch.zeros(3), w_c=torch.zeros(n, 3))
    setting = (float(z[f"s{i}_cur_time"]), float(z[f"s{i}_delta_t"]), bool(z[f"s{i}_in_smooth"]))
    outs, mask, grads = run_framework(d, setting, 0)
    np.testing.assert_array_equal(mask, z[f"s{i}_mask"])
    for k in ("means", "opacities", "scales", "quats"):
        np.testing.assert_allclose(outs[k], z[f"s{i}_{k}"], rtol=1e-6, atol=1e-6)
    for k in GOLD_RAW:
        ref = z[f"s{i}_grad_{k}"]
        # per element, 1e-6 of the element or of the tensor's largest entry: the golden is the reference's own float32 run, whose
        # small entries carry the rounding of the large terms they are differences of
        np.testing.assert_allclose(grads[k], ref, rtol=1e-6, atol=1e-6 * np.abs(ref).max(), err_msg=k)
        assert np.abs(grads[k][~mask]).max() == 0.0 and np.abs(ref[~mask]).max() == 0.0


def test_cpu_tensors_raise():
    d = random_rows(10, 0)
    with pytest.raises(L.BdsError):
        pvg.time_transform(*[d[k] for k in RAW], d["cam_pos"], 0.3, 0.0, False, T, 3)


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("pvg")
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    h.hm_pvg_fwd.argtypes = [ci, ci, ci, cf, cf, ci, cd] + [vp] * 15
    h.hm_pvg_bwd.argtypes = [ci, cf, cf, ci, cd] + [vp] * 16
    return h


@pytest.fixture(scope="module")
def rows():
    return random_rows(4000, 21)


def _p(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.contiguous().data_ptr()


@pytest.mark.parametrize("setting", SETTINGS[:2], ids=["plain", "smoothed"])
def test_host_math_matches_float64_autograd(shim, rows, setting):
    d, n = rows, 4000
    cur, dt, smooth = setting
    ref = run_framework(settle_clamp(d, setting, 3), setting, 3)
    bound, e32 = measured_bound(d, setting, 3, ref)
    o64, mask, g64 = ref
    coeffs = torch.cat((d["features_dc"][:, None, :], d["features_rest"]), 1).contiguous()
    o = dict(means=np.zeros((n, 3), np.float32), opacities=np.zeros((n, 1), np.float32), rgbs=np.zeros((n, 3), np.float32),
             scales=np.zeros((n, 3), np.float32), quats=np.zeros((n, 4), np.float32))
    keep = np.zeros(n, np.uint8)
    shim.hm_pvg_fwd(n, 16, 3, cur, dt, int(smooth), T, *[_p(d[k]) for k in RAW[:7]], _p(coeffs), _p(d["cam_pos"]),
                    *[_p(o[k]) for k in OUTS], _p(keep))
    np.testing.assert_array_equal(keep.astype(bool), mask)
    worst = max(scaled_err(o[k][mask], o64[k]) for k in OUTS)
    # the VJP of the four small tensors (the colour's is the SH backward: bases times the clamped gradient, checked on the GPU)
    g = dict(velocity=np.zeros((n, 3), np.float32), taus=np.zeros((n, 1), np.float32), betas=np.zeros((n, 1), np.float32),
             logits=np.zeros((n, 1), np.float32), log_scales=np.zeros((n, 3), np.float32), quats=np.zeros((n, 4), np.float32))
    shim.hm_pvg_bwd(n, cur, dt, int(smooth), T, *[_p(d[k]) for k in ("velocity", "taus", "betas", "logits", "log_scales", "quats")],
                    *[_p(d[k]) for k in ("w_m", "w_o", "w_s", "w_q")], *[_p(g[k]) for k in g])
    for k in g:
        worst = max(worst, scaled_err(g[k][mask], g64[k][mask]))
    print(f"\npvg shim: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, shim {worst:.3e}")
    assert worst <= bound, (worst, bound)
    assert np.abs(g64["taus"][mask]).min() > 0 and np.abs(g64["betas"][mask]).max() > 0


# ---- resources and argument validation ---------------------------------------------------------------------------------------------
def test_pvg_kernel_resources():
    res = kernel_resources("pvg.hip")
    # (count, scan: one instance each; write, backward: one per colour mode 0..3 and the sigmoid form)
    for prefix, (n, occ) in {"pvg_count_kernel": (1, 8), "pvg_scan_kernel": (1, 8), "pvg_write_kernel": (5, 8), "pvg_bwd_kernel": (5, 7)}.items():
        ks = [k for k in res if k.startswith(prefix)]
        assert len(ks) == n, (prefix, list(res))
        for k in ks:
            assert res[k]["ScratchSize"] == 0, (k, res[k])
            assert res[k]["Occupancy"] >= occ, (k, res[k])


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    fake = 1 << 20      # never dereferenced: every case fails its argument check first

    def fwd(N=100, K=16, deg=3, T=0.2, p=fake, rest=fake, temp=fake, nb=1 << 20):
        return lib.bds_pvg_fwd(N, K, deg, 0.3, 0.0, 0, T, *([p] * 8), rest, *([fake] * 8), temp, nb, None)

    def bwd(N=100, M=50, K=16, deg=3, T=0.2, p=fake, temp=fake, nb=1 << 20, g=fake):
        return lib.bds_pvg_bwd(N, M, K, deg, 0.3, 0.0, 0, T, *([p] * 8), temp, nb, *([fake] * 7), *([g] * 9), None)

    for f in (fwd, bwd):
        assert f(N=-1) == L.BDS_EINVAL and f(p=None) == L.BDS_EINVAL
        for K in (0, 2, 3, 8, 15, 25):
            assert f(K=K, deg=0) == L.BDS_EINVAL, K
        assert f(K=9, deg=3) == L.BDS_EINVAL and f(K=1, deg=1) == L.BDS_EINVAL and f(deg=-1) == L.BDS_EINVAL and f(deg=4) == L.BDS_EINVAL
        assert f(T=0.0) == L.BDS_EINVAL and f(T=-0.2) == L.BDS_EINVAL
        assert f(temp=None) == L.BDS_EINVAL and f(temp=fake + 4) == L.BDS_EINVAL
        assert f(nb=lib.bds_pvg_temp_bytes(100) - 1) == L.BDS_EINVAL
        m0 = {"M": 0} if f is bwd else {}
        assert f(N=0, **m0) == L.BDS_OK and f(N=0, p=None, temp=None, nb=0, **m0) == L.BDS_OK
    assert fwd(rest=None) == L.BDS_EINVAL and bwd(g=None) == L.BDS_EINVAL and bwd(M=101) == L.BDS_EINVAL
    assert lib.bds_pvg_temp_bytes(0) == 0 and lib.bds_pvg_temp_bytes(1) >= 16 + 4
    assert lib.bds_pvg_temp_bytes(3 * 10 ** 6) >= 16 + 4 * (3 * 10 ** 6 // 256 + 1)
