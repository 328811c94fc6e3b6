"""Pose chain and skinning of the SMPL nodes (bilateral_driving_amd/smpl.py, csrc/smpl.hip) on the CPU: the float64 restatement
against the golden vectors produced by the reference's own SMPLNodes / SMPLTemplate / VoxelDeformer methods
(scripts/gen_golden_smpl_skin.py), the device math on the host (tests/hostmath_smpl_shim.hip) against float64 autograd within the
measured bound of tests/smpl_skin_ref64.py, argument validation of the C entries, the CPU behaviour of the Python layer and the
install seam.

Measured on the shim cases (printed by the test; each tensor's largest error over max(1, its largest reference magnitude)): float32
framework ops against float64 differ by 1.5e-7 .. 1.0e-6 depending on the case, so the shim is allowed 1.0e-6 (the floor) .. 4.0e-6; it
measures 9.4e-8 .. 1.0e-6 (at most 1.4 times the framework's own float32 error in any case)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import smpl
from tests import smpl_skin_ref64 as R
from tests.util import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smpl_skin.npz")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLD)


def test_golden_covers_the_contract(golden):
    d, z = golden
    assert os.path.getsize(GOLD) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "node_pose_train.npz"))
    I, V = d["instances_fv"].shape[1], d["means"].shape[0] // d["instances_fv"].shape[1]
    assert (I, V, tuple(d["voxel_base"].shape[2:]), d["instances_fv"].shape[0]) == (2, 6890, (4, 8, 8), 5)
    f_both, f_absent = (int(f) for f in z["train_frames"])
    f_int = int(z["interp_frame"])
    assert d["instances_fv"][f_both].all() and d["instances_fv"][f_absent].tolist() == [True, False] and 1 < f_int < 4
    for f in (f_both, f_absent, f_int):        # no row's branch or sign hangs on float32 rounding: the generator's condition, again
        gap, real = R.blend_margins(d, f, interpolate=f == f_int)
        assert float(gap.min()) >= 1e-6 and float(real.min()) >= 1e-6, (f, float(gap.min()), float(real.min()))
    n = R.normalize_coords(d["means"].reshape(I, V, 3).double(), d["offset"].double(), d["scale"].double(), d["ratio"], d["ratio_dim"])
    assert float((n.abs() > 1).any(-1).float().mean()) >= 0.01        # the border clamp is exercised
    assert int((n == 1).any(-1).sum()) >= 4                           # points exactly on an upper face


def _close(got, ref, name):
    # 1e-6 of the element or of the tensor's largest entry: the golden is the reference's own float32 run, whose small entries carry
    # the rounding of the large terms they are sums of
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6 * max(float(np.abs(ref).max()), 1e-30), err_msg=name)


@pytest.mark.parametrize("which", [0, 1])
def test_float64_restatement_matches_reference_golden_training(golden, which):
    d, z = golden
    f, s = int(z["train_frames"][which]), int(z["stride"])
    outs, grads = R.run_framework(d, f)
    _close(outs["wm"][::s], z[f"f{f}_wm"], "wm")
    _close(outs["wq"][::s], z[f"f{f}_wq"], "wq")
    for k in R.INPUTS:
        _close(grads[k][::s] if k in ("means", "quats") else grads[k], z[f"f{f}_grad_{k}"], k)
    if which == 1:      # instance 1 is absent: its translation gradient is the sum of its rows' weights, everything else of it zero
        V = 6890
        assert np.abs(grads["means"][V:]).max() == 0 and np.abs(grads["quats"][V:]).max() == 0 and np.abs(grads["voxel_corr"][1]).max() == 0
        assert np.abs(grads["smpl_quats"][f, 1]).max() == 0 and np.abs(grads["instances_quats"][f, 1]).max() == 0
        np.testing.assert_allclose(grads["instances_trans"][f, 1], d["w_m"][V:].double().sum(0).numpy(), rtol=1e-12)
        assert (outs["wq"][V:] == np.array([1.0, 0, 0, 0])).all() and (outs["wm"][V:] == d["instances_trans"][f, 1].double().numpy()).all()


def test_float64_restatement_matches_reference_golden_interpolated_and_ball(golden):
    d, z = golden
    f, s = int(z["interp_frame"]), int(z["stride"])
    outs, _ = R.run_framework(d, f, interpolate=True, grad=False)
    _close(outs["wm"][::s], z[f"f{f}_wm"], "wm")
    _close(outs["wq"][::s], z[f"f{f}_wq"], "wq")
    f = int(z["train_frames"][0])
    outs, _ = R.run_framework(d, f, ball=True, grad=False)
    _close(outs["wm"][::s], z[f"f{f}_wm_ball"], "wm_ball")


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("smpl")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.hm_smpl_fwd.argtypes = [ci, ci] + [vp] * 12 + [ci, ci, ci, vp, vp, cf, ci, vp, vp, vp]
    h.hm_smpl_bwd.argtypes = [ci, ci] + [vp] * 11 + [ci, ci, ci, vp, vp, cf, ci] + [vp] * 9
    return h


def _p(a):
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def run_shim(h, d, f, ball=False):
    """The shim's forward and backward on the inputs d at frame f -> (outs, grads) in run_framework's layout."""
    I = d["instances_fv"].shape[1]
    N = d["means"].shape[0]
    V = N // I
    c = lambda t: None if t is None else t.float().contiguous()
    root, body, trans = c(d["instances_quats"][f]), c(d["smpl_quats"][f]), c(d["instances_trans"][f])
    present = d["instances_fv"][f].to(torch.uint8).contiguous()
    par = (ctypes.c_int32 * 24)(*([0] + list(d["parents"][1:])))
    field = d.get("voxel_base") is not None
    base, corr, W, off, sc = (c(d.get(k)) for k in ("voxel_base", "voxel_corr", "W", "offset", "scale"))
    dhw = tuple(base.shape[2:]) if field else (0, 0, 0)
    means, quats = c(d["means"]), c(d["quats"])
    wm, wq, A = np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32), np.zeros((I, 24, 3, 4), np.float32)
    tail = (*dhw, _p(off), _p(sc), float(d.get("ratio") or 1.0), int(d.get("ratio_dim") or 0) % 3)
    assert h.hm_smpl_fwd(I, V, _p(means), _p(quats), _p(root), _p(body), _p(trans), _p(present), _p(c(d["J_canonical"])), _p(c(d["A0_inv"])),
                         ctypes.cast(par, ctypes.c_void_p), _p(base), _p(corr), _p(W), *tail, _p(wm), None if ball else _p(wq), _p(A)) == 0
    F = d["instances_fv"].shape[0]
    g = dict(means=np.zeros((N, 3), np.float32), quats=np.zeros((N, 4), np.float32), instances_quats=np.zeros((F, I, 1, 4), np.float32),
             smpl_quats=np.zeros((F, I, 23, 4), np.float32), instances_trans=np.zeros((F, I, 3), np.float32))
    if field:
        g["voxel_corr"] = np.full(tuple(base.shape), np.nan, np.float32)
    w_m, w_q = c(d["w_m"]), c(d["w_q"])
    assert h.hm_smpl_bwd(I, V, _p(means), _p(quats), _p(root), _p(body), _p(present), _p(c(d["J_canonical"])), _p(c(d["A0_inv"])),
                         ctypes.cast(par, ctypes.c_void_p), _p(base), _p(corr), _p(W), *tail, _p(A), _p(w_m), None if ball else _p(w_q),
                         _p(g["means"]), None if ball else _p(g["quats"]), _p(g["instances_quats"][f]), _p(g["smpl_quats"][f]),
                         _p(g["instances_trans"][f]), _p(g.get("voxel_corr"))) == 0
    outs = {"wm": wm} if ball else {"wm": wm, "wq": wq}
    if ball:
        del g["quats"]
    return outs, g


CASES = {   # I, V, field, parents, absent, ball
    "one-point": (1, 1, (2, 2, 2), R.SMPL_PARENTS, (), False),
    "three-by-63": (3, 63, (3, 5, 7), R.SMPL_PARENTS, (), False),
    "three-by-65-permuted-absent": (3, 65, (4, 16, 16), R.PERMUTED_PARENTS, (1,), False),
    "one-by-65": (1, 65, (3, 5, 7), R.PERMUTED_PARENTS, (), False),
    "three-by-one": (3, 1, (4, 16, 16), R.SMPL_PARENTS, (2,), False),
    "one-by-63-small-field": (1, 63, (2, 2, 2), R.SMPL_PARENTS, (), False),
    "ball": (3, 65, (3, 5, 7), R.SMPL_PARENTS, (0,), True),
    "fixed-weights": (3, 63, None, R.SMPL_PARENTS, (1,), False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_host_math_matches_float64_autograd(shim, case):
    I, V, dhw, parents, absent, ball = CASES[case]
    d = R.make_inputs(I, V, dhw or (2, 2, 2), seed=100 + len(case), parents=parents, absent=absent, field=dhw is not None, settle=dhw is not None)
    if dhw is None:      # (a fixed table is not settled by moving points: check the margins instead)
        gap, real = R.blend_margins(d, 1)
        assert float(gap.min()) >= R.GAP and float(real.min()) >= R.GAP
    ref = R.run_framework(d, 1, ball=ball)
    bound, e32 = R.measured_bound(d, 1, ref, ball=ball)
    outs, grads = run_shim(shim, d, 1, ball=ball)
    worst = R.worst(outs, grads, ref)
    print(f"\nsmpl shim {case}: float32 framework vs float64 {e32:.3e}, bound {bound:.3e}, shim {worst:.3e}")
    assert worst <= bound, (worst, bound)
    for i in absent:     # exactly: translation and unit quaternion out, only the translation's gradient back
        rows = slice(i * V, (i + 1) * V)
        assert (outs["wm"][rows] == d["instances_trans"][1, i].numpy()).all() and np.abs(grads["means"][rows]).max() == 0
        assert np.abs(grads["smpl_quats"][1, i]).max() == 0 and np.abs(grads["instances_quats"][1, i]).max() == 0
        if not ball:
            assert (outs["wq"][rows] == np.array([1, 0, 0, 0], np.float32)).all() and np.abs(grads["quats"][rows]).max() == 0
        if "voxel_corr" in grads:
            assert np.abs(grads["voxel_corr"][i]).max() == 0


def test_host_math_rejects_a_bad_parent_table(shim):
    d = R.make_inputs(1, 1, (2, 2, 2), seed=3)
    for bad in ((-1, 0, 2) + R.SMPL_PARENTS[3:], R.SMPL_PARENTS[:23] + (23,), R.SMPL_PARENTS[:5] + (-1,) + R.SMPL_PARENTS[6:]):
        with pytest.raises(AssertionError):
            run_shim(shim, dict(d, parents=bad), 1)


# ---- argument validation, CPU behaviour, the seam ----------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    fake = 1 << 20      # never dereferenced: every case fails its argument check first
    good = (ctypes.c_int32 * 24)(*([0] + list(R.SMPL_PARENTS[1:])))

    def fwd(I=2, V=100, p=fake, quats=fake, par=good, base=fake, corr=fake, W=None, dhw=(4, 8, 8), off=fake, rdim=2, wm=fake, wq=fake, A=fake):
        return lib.bds_smpl_skin_fwd(I, V, p, quats, p, p, p, p, p, p, par, base, corr, W, *dhw, off, off, 2.0, rdim, wm, wq, A, None)

    def bwd(I=2, V=100, p=fake, quats=fake, par=good, base=fake, corr=fake, W=None, dhw=(4, 8, 8), off=fake, rdim=2, A=fake, vwq=fake, vq=fake,
            g=fake, vcorr=fake, temp=fake, nb=1 << 24):
        return lib.bds_smpl_skin_bwd(I, V, p, quats, p, p, p, p, p, par, base, corr, W, *dhw, off, off, 2.0, rdim, A, p, vwq, g, vq, g, g, g, vcorr,
                                     temp, nb, None)

    for f in (fwd, bwd):
        assert f(I=0) == L.BDS_EINVAL and f(V=0) == L.BDS_EINVAL and f(p=None) == L.BDS_EINVAL and f(par=None) == L.BDS_EINVAL
        for table in ([0, 1] + list(R.SMPL_PARENTS[2:]), list(R.SMPL_PARENTS[:23]) + [23], [0, -1] + list(R.SMPL_PARENTS[2:]),
                      [0] + list(R.SMPL_PARENTS[1:12]) + [12] + list(R.SMPL_PARENTS[13:])):
            assert f(par=(ctypes.c_int32 * 24)(*table)) == L.BDS_EINVAL, table
        assert f(rdim=3) == L.BDS_EINVAL and f(rdim=-1) == L.BDS_EINVAL
        assert f(dhw=(0, 8, 8)) == L.BDS_EINVAL and f(off=None) == L.BDS_EINVAL
        assert f(base=None, corr=None, W=None) == L.BDS_EINVAL and f(base=None, corr=fake, W=fake) == L.BDS_EINVAL
    assert fwd(wm=None) == L.BDS_EINVAL and fwd(A=None) == L.BDS_EINVAL and fwd(quats=None) == L.BDS_EINVAL
    assert bwd(A=None) == L.BDS_EINVAL and bwd(g=None) == L.BDS_EINVAL and bwd(vwq=None) == L.BDS_EINVAL and bwd(vq=None) == L.BDS_EINVAL
    assert bwd(temp=None) == L.BDS_EINVAL and bwd(temp=fake + 4) == L.BDS_EINVAL
    assert bwd(nb=lib.bds_smpl_skin_bwd_temp_bytes(2, 100) - 1) == L.BDS_EINVAL
    assert bwd(base=None, corr=None, W=fake, vcorr=fake) == L.BDS_EINVAL
    assert lib.bds_smpl_skin_bwd_temp_bytes(0, 5) == 0 and lib.bds_smpl_skin_bwd_temp_bytes(5, 0) == 0
    assert lib.bds_smpl_skin_bwd_temp_bytes(1, 1) >= 4 * (24 * 12 + 3)
    assert lib.bds_smpl_skin_bwd_temp_bytes(8, 6890) >= 8 * 27 * 4 * (24 * 12 + 3)


def test_cpu_tensors_raise_and_bad_tables_are_refused():
    d = R.make_inputs(2, 5, (2, 2, 2), seed=1)
    args = (d["means"], d["quats"], d["instances_quats"], d["smpl_quats"], d["instances_trans"], d["instances_fv"], 1)
    with pytest.raises(L.BdsError):
        smpl.skin_transform(*args, voxel_corr=d["voxel_corr"], **R.template_kwargs(d))
    with pytest.raises(ValueError):
        smpl.check_parents((0, 1) + R.SMPL_PARENTS[2:])
    with pytest.raises(ValueError):
        smpl.check_parents(R.SMPL_PARENTS[:23])


class _Cam:
    camtoworlds = torch.eye(4)


def test_install_and_uninstall_restore_the_class_and_cpu_tensors_keep_its_method(golden):
    class Nodes(R.StandInNodes):
        pass

    class Other(R.StandInNodes):
        pass
    own = Nodes.__dict__.get("get_gaussians")
    assert own is None and not hasattr(Nodes, "_bds_reference_get_gaussians")
    smpl.install(Nodes)
    assert Nodes.get_gaussians is smpl.smpl_get_gaussians and Nodes._bds_reference_get_gaussians is R.StandInNodes.get_gaussians
    assert Other.get_gaussians is R.StandInNodes.get_gaussians
    d = R.make_inputs(2, 9, (2, 2, 2), seed=2)
    node = Nodes(d, "cpu", sh_degree=0)
    gs = node.get_gaussians(_Cam())          # CPU tensors: the class's own method
    ref = R.StandInNodes.get_gaussians(Nodes(d, "cpu", sh_degree=0), _Cam())
    assert list(gs) == ["_means", "_opacities", "_rgbs", "_scales", "_quats"] and all(torch.equal(gs[k], ref[k]) for k in gs)
    smpl.install(Nodes)                      # twice: still one original
    smpl.uninstall(Nodes)
    assert "get_gaussians" not in Nodes.__dict__ and not hasattr(Nodes, "_bds_reference_get_gaussians")
    assert Nodes.get_gaussians is R.StandInNodes.get_gaussians
