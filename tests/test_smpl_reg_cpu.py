"""The SMPL nodes' kNN and skinning-field regularisers (bilateral_driving_amd/smpl_reg.py, csrc/smpl_reg.hip) on the CPU: the float64
restatement (tests/smpl_reg_ref64.py) against torch autograd of the reference's own expressions and against the golden vectors the
reference's SMPLNodes.compute_reg_loss produced (scripts/gen_golden_smpl_reg.py); the device math on the host
(tests/hostmath_smpl_reg_shim.hip) against the restatement, which is where the GPU test's FLOOR is measured; the reverse lists; the
C entries' argument checks; and the install seam on a stand-in.

Measured here (printed by the tests; error = largest difference over the tensor's largest reference magnitude): the host shim against
float64 is 2.3e-7 .. 2.29e-6 over the kNN cases (the largest: the opacity gradient at K = 2) and 8.7e-8 .. 6.3e-7 over the field
cases; FLOOR = 2.3e-6 is the largest, rounded up to two digits.  The float32 framework expression's own error on the same cases: 2.2e-7 .. 2.27e-6 (kNN), 7.2e-8 .. 1.7e-7 (field); both are
exactly 0 on the constant and the all-self cases."""
import ctypes
import os

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import smpl_reg
from tests import smpl_reg_ref64 as R
from tests.util import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smpl_reg.npz")
PARAMS = ("_features_dc", "_features_rest", "_opacities", "_scales", "_quats")


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CASES))
def test_ref64_matches_float64_autograd_of_the_reference_lines(case):
    d = R.make_knn(seed=len(case), **R.CASES[case])
    e = R.errors(R.knn_ref(d), R.run_knn(d))
    assert max(e.values()) <= 1e-12, e


def test_ref64_with_every_instance_absent_is_zero():
    terms, grads = R.knn_ref(R.make_knn(2, 20, 3, absent=(0, 1)))
    assert not terms.any() and all(not g.any() for g in grads.values())


@pytest.mark.parametrize("case", list(R.FIELD_CASES))
def test_field_ref64_matches_float64_autograd_of_the_reference_lines(case):
    d = R.make_field(R.FIELD_CASES[case], seed=len(case))
    e = R.errors(R.field_ref(d), R.run_field(d))
    assert max(e.values()) <= 1e-12, e
    zero = R.make_field(R.FIELD_CASES[case], kind="zero")
    (terms, grad), (t64, g64) = R.field_ref(zero), R.run_field(zero)
    assert not terms.any() and not grad.any() and not t64.any() and not g64.any()      # torch: sign(0) = 0, the zero vector's norm has gradient 0


def _golden():
    z = np.load(GOLD)
    d = {k: torch.from_numpy(z[k]) for k in R.GROUPS}
    d.update(nn_ind=torch.from_numpy(z["nn_ind"].astype(np.int64)), w=None)
    return z, d, torch.from_numpy(z["field"]), torch.from_numpy(z["instances_fv"])


def _close(got, ref, name):
    # the golden is the reference's own float32 run: 2e-6 of the tensor's largest entry (sums of up to 2 x 96 x 9 float32 terms)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6 * max(float(np.abs(ref).max()), 1e-30), err_msg=name)


@pytest.mark.parametrize("frame", [0, 1])
def test_ref64_and_the_stand_in_match_the_reference_golden(frame):
    z, d, field, frames = _golden()
    assert frames.tolist() == [[True, True], [True, False]] and d["nn_ind"].shape == (2, 96, 3) and field.shape == (2, 24, 2, 4, 4)
    keys = [str(k) for k in z[f"f{frame}_keys"]]
    assert keys == ["voxel_deformer_reg"] + list(smpl_reg.KEYS)
    lam = np.array([R.LAMBDAS[k] for k in smpl_reg.LAMBDAS])
    d = dict(d, present=frames[frame], w=torch.from_numpy(lam))
    terms, grads = R.knn_ref(d)
    _close(terms * lam, z[f"f{frame}_values"][1:], "knn values")
    for attr, k in zip(PARAMS, R.GROUPS):
        _close(grads[k], z[f"f{frame}_grad{attr}"], attr)
        if frame == 1:
            assert not z[f"f{frame}_grad{attr}"][96:].any() and not grads[k][96:].any()      # the absent instance's rows
    f = dict(field=field, w=torch.tensor([R.VOX["lambda_std_w"], R.VOX["lambda_w_norm"]]))
    ft, fg = R.field_ref(f)
    _close(float((ft * f["w"].numpy()).sum()), z[f"f{frame}_values"][0], "field value")
    _close(fg, z[f"f{frame}_grad_field"], "field gradient")
    # the stand-in's own method is the reference's: the same keys, values and gradients
    node = R.StandInNodes(dict(d, w=None), field, "cpu", frames=frames, cur_frame=frame)
    node.reg_cfg = R.Ns(voxel_deformer_reg=node.reg_cfg.voxel_deformer_reg, knn_reg=node.reg_cfg.knn_reg)
    vals, g = R.loss_and_grads(node)
    assert list(vals) == keys
    _close(np.array(list(vals.values())), z[f"f{frame}_values"], "stand-in values")
    for attr in PARAMS:
        _close(g[attr], z[f"f{frame}_grad{attr}"], "stand-in " + attr)
    _close(g["voxel_w_correction"], z[f"f{frame}_grad_field"], "stand-in field")


# ---- the device math on the host ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("smpl_reg")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    h.hm_knn_reg_fwd.argtypes = [ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp]
    h.hm_knn_reg_bwd.argtypes = [ci, ci, ci] + [vp] * 5 + [ci, vp, vp, ci] + [vp] * 10
    h.hm_voxel_reg_fwd.argtypes = [ci] * 5 + [vp] * 3
    h.hm_voxel_reg_bwd.argtypes = [ci] * 5 + [vp] * 4
    for f in (h.hm_knn_reg_fwd, h.hm_knn_reg_bwd, h.hm_voxel_reg_fwd, h.hm_voxel_reg_bwd):
        f.restype = None
    return h


def _p(a):
    return None if a is None else a.ctypes.data


def shim_knn(h, d):
    I, V, K = d["nn_ind"].shape
    a = [None if d[k] is None else np.ascontiguousarray(d[k].numpy().reshape(I * V, -1), np.float32) for k in R.GROUPS]
    ctot = sum(0 if x is None else x.shape[1] for x in a)
    c_rest, s_dim = (0 if a[1] is None else a[1].shape[1]), (3 if a[3] is None else a[3].shape[1])
    nn = np.ascontiguousarray(d["nn_ind"].numpy(), np.int32)
    offsets, edges = (t.numpy() for t in smpl_reg.reverse_lists(d["nn_ind"]))
    present = np.ascontiguousarray(d["present"].numpy(), np.uint8)
    terms, norm = np.zeros(5, np.float32), np.zeros(5, np.float32)
    mean, rstd = np.zeros(I * V * ctot, np.float32), np.zeros(I * V * ctot, np.float32)
    h.hm_knn_reg_fwd(I, V, K, _p(nn), _p(present), _p(a[0]), _p(a[1]), c_rest, _p(a[2]), _p(a[3]), s_dim, _p(a[4]), _p(terms), _p(norm), _p(mean),
                     _p(rstd))
    g = [None if x is None else np.full_like(x, np.nan) for x in a]
    w = np.ascontiguousarray(d["w"].numpy(), np.float32)
    h.hm_knn_reg_bwd(I, V, K, _p(offsets), _p(edges), _p(present), _p(a[0]), _p(a[1]), c_rest, _p(a[2]), _p(a[3]), s_dim, _p(a[4]), _p(mean), _p(rstd),
                     _p(norm), _p(w), *[_p(x) for x in g])
    return terms, {k: x.reshape(d[k].shape) for k, x in zip(R.GROUPS, g) if x is not None}


def shim_field(h, d):
    x = np.ascontiguousarray(d["field"].numpy(), np.float32)
    I, J, D, H, W = x.shape
    terms, rnorm, grad = np.zeros(2, np.float32), np.zeros((I, D, H, W), np.float32), np.full_like(x, np.nan)
    h.hm_voxel_reg_fwd(I, J, D, H, W, _p(x), _p(terms), _p(rnorm))
    h.hm_voxel_reg_bwd(I, J, D, H, W, _p(x), _p(rnorm), _p(np.ascontiguousarray(d["w"].numpy(), np.float32)), _p(grad))
    return terms, grad


@pytest.mark.parametrize("case", list(R.CASES))
def test_host_math_matches_float64_within_the_floor(shim, case):
    d = R.make_knn(seed=len(case), **R.CASES[case])
    ref = R.knn_ref(d)
    e32 = R.errors(R.run_knn(d, dtype=torch.float32), ref)
    e = R.errors(shim_knn(shim, d), ref)
    print(f"\nsmpl_reg shim {case}: float32 framework vs float64 {max(e32.values()):.3e}, shim {max(e.values()):.3e} ({max(e, key=e.get)})")
    assert max(e.values()) <= R.FLOOR, e
    if case in ("self", "constant"):        # std exactly 0: terms and gradients exactly 0, nothing NaN
        terms, grads = shim_knn(shim, d)
        assert not terms.any() and all(not g.any() for g in grads.values())


def test_host_math_with_every_instance_absent(shim):
    terms, grads = shim_knn(shim, R.make_knn(2, 20, 3, absent=(0, 1)))
    assert not terms.any() and all(not g.any() for g in grads.values())


@pytest.mark.parametrize("case", list(R.FIELD_CASES))
def test_field_host_math_matches_float64_within_the_floor(shim, case):
    d = R.make_field(R.FIELD_CASES[case], seed=len(case))
    ref = R.field_ref(d)
    e32 = R.errors(R.run_field(d, dtype=torch.float32), ref)
    e = R.errors(shim_field(shim, d), ref)
    print(f"\nsmpl_reg field shim {case}: float32 framework vs float64 {max(e32.values()):.3e}, shim {max(e.values()):.3e}")
    assert max(e.values()) <= R.FLOOR, e
    terms, grad = shim_field(shim, R.make_field(R.FIELD_CASES[case], kind="zero"))
    assert not terms.any() and not grad.any()


def test_field_host_math_single_voxels_against_hand_derived_gradients(shim):
    """One non-zero voxel v > 0 in channel 0 of a [1,2,3,3,3] field: it is the higher end of its differences towards -1 and the lower
    end of those towards +1, so its own TV gradient is (number of its neighbours) signs of +1, each neighbour's is -1 (all over
    3 x that axis' count = 3 x 2 x 18), and the magnitude's is x / |x| = 1 over the 27 voxels, in channel 0 only."""
    for at, n_neighbours in (((0, 0, 0), 3), ((1, 1, 1), 6)):
        x = torch.zeros(1, 2, 3, 3, 3)
        x[(0, 0) + at] = 0.5
        terms, grad = shim_field(shim, dict(field=x, w=torch.tensor([1.0, 1.0])))
        unit = 1.0 / (3 * 2 * 18)
        np.testing.assert_allclose(grad[(0, 0) + at], n_neighbours * unit + 1.0 / 27, rtol=1e-6)
        np.testing.assert_allclose(terms, [0.5 * n_neighbours / (3 * 2 * 18), 0.5 / 27], rtol=1e-6)
        for ax in range(3):
            for step in (-1, 1):
                nb = list(at)
                nb[ax] += step
                if 0 <= nb[ax] < 3:
                    np.testing.assert_allclose(grad[(0, 0) + tuple(nb)], -unit, rtol=1e-6)
        assert np.count_nonzero(grad) == 1 + n_neighbours and not grad[0, 1].any()


# ---- the reverse lists ----------------------------------------------------------------------------------------------------------------
def test_reverse_lists_hold_every_edge_once_ascending_with_multi_edges():
    d = R.make_knn(3, 37, 5, seed=3, nn="hub")
    nn = d["nn_ind"]
    offsets, edges = smpl_reg.reverse_lists(nn)
    I, V, K = nn.shape
    assert offsets.dtype == edges.dtype == torch.int32 and offsets.shape == (I, V + 1) and edges.shape == (I, V * K)
    for i in range(I):
        assert sorted(edges[i].tolist()) == list(range(V * K))            # every (point, slot) once
        assert offsets[i, 0] == 0 and offsets[i, V] == V * K
        flat = nn[i].reshape(-1)
        for r in range(V):
            mine = edges[i, offsets[i, r]:offsets[i, r + 1]].tolist()
            assert mine == sorted(mine) and mine == (flat == r).nonzero().reshape(-1).tolist()
    assert int(offsets[0, 2] - offsets[0, 1]) == 0                        # row 1 is listed by nobody
    assert int(offsets[0, V // 2 + 1] - offsets[0, V // 2]) >= V          # the hub: every point's slot 0
    pair = [e for e in edges[0, offsets[0, nn[0, 0, 0]]:offsets[0, nn[0, 0, 0] + 1]].tolist() if e // K == 0]
    assert len(pair) >= 2                                                  # row 0 lists one index twice: both edges kept
    same, _ = smpl_reg.reverse_lists(nn.to(torch.int32))
    assert torch.equal(same, offsets)


def test_reverse_lists_refuse_indices_outside_the_instance():
    nn = R.make_knn(2, 10, 3)["nn_ind"]
    for bad in (-1, 10):
        broken = nn.clone()
        broken[1, 4, 2] = bad
        with pytest.raises(IndexError):
            smpl_reg.reverse_lists(broken)
    with pytest.raises(ValueError):
        smpl_reg.reverse_lists(nn.float())


def test_reverse_lists_are_cached_on_the_node_by_identity_and_version(monkeypatch):
    d = R.make_knn(2, 10, 3)
    node = R.StandInNodes(d, R.make_field((2, 24, 2, 2, 2))["field"], "cpu")
    calls = []
    real = smpl_reg.reverse_lists
    monkeypatch.setattr(smpl_reg, "reverse_lists", lambda nn: calls.append(1) or real(nn))
    a = smpl_reg.cached_reverse_lists(node, node.nn_ind)
    assert smpl_reg.cached_reverse_lists(node, node.nn_ind) is a and len(calls) == 1 and a[2].dtype == torch.int32
    node.nn_ind[0, 0, 0] = 3                   # written in place: the version moves
    b = smpl_reg.cached_reverse_lists(node, node.nn_ind)
    assert b is not a and len(calls) == 2
    node.nn_ind = node.nn_ind.clone()          # what update_knn does: another tensor
    assert smpl_reg.cached_reverse_lists(node, node.nn_ind) is not b and len(calls) == 3


# ---- argument validation, CPU behaviour, the seam -------------------------------------------------------------------------------------
def test_entries_reject_bad_arguments_without_a_gpu():
    lib, p = L.lib(), 1 << 20      # never dereferenced: every case fails its argument check first

    def fwd(I=2, V=10, K=3, nn=p, present=p, rest=p, c_rest=9, scales=p, s_dim=3, terms=p, mean=p, temp=p, nb=1 << 20):
        return lib.bds_smpl_knn_reg_fwd(I, V, K, nn, present, p, rest, c_rest, p, scales, s_dim, p, terms, p, mean, p, temp, nb, None)

    def bwd(I=2, V=10, K=3, off=p, rest=p, c_rest=9, s_dim=3, v_rest=p, v_dc=p, mean=p):
        return lib.bds_smpl_knn_reg_bwd(I, V, K, off, p, p, p, rest, c_rest, p, p, s_dim, p, mean, p, p, p, v_dc, v_rest, p, p, p, None)

    for f in (fwd, bwd):
        assert f(I=0) == L.BDS_EINVAL and f(V=0) == L.BDS_EINVAL and f(K=1) == L.BDS_EINVAL and f(K=33) == L.BDS_EINVAL
        assert f(c_rest=10) == L.BDS_EINVAL and f(s_dim=2) == L.BDS_EINVAL and f(mean=None) == L.BDS_EINVAL
    assert fwd(nn=None) == L.BDS_EINVAL and fwd(present=None) == L.BDS_EINVAL and fwd(terms=None) == L.BDS_EINVAL
    assert fwd(temp=None) == L.BDS_EINVAL and fwd(nb=lib.bds_smpl_knn_reg_temp_bytes(2, 10, 20) - 1) == L.BDS_EINVAL
    assert bwd(off=None) == L.BDS_EINVAL and bwd(v_rest=None) == L.BDS_EINVAL and bwd(rest=None) == L.BDS_EINVAL and bwd(v_dc=None) == L.BDS_EINVAL
    assert lib.bds_smpl_knn_reg_temp_bytes(8, 6890, 20) == 4 * 5 * ((8 * 6890 * 20 + 255) // 256) and lib.bds_smpl_knn_reg_temp_bytes(0, 5, 5) == 0

    def vfwd(dims=(1, 24, 2, 2, 2), x=p, terms=p, temp=p, nb=1 << 20):
        return lib.bds_voxel_reg_fwd(*dims, x, terms, p, temp, nb, None)

    def vbwd(dims=(1, 24, 2, 2, 2), x=p, terms=p, **_):
        return lib.bds_voxel_reg_bwd(*dims, x, p, terms, p, None)

    for f in (vfwd, vbwd):
        for dims in ((0, 24, 2, 2, 2), (1, 0, 2, 2, 2), (1, 65, 2, 2, 2), (1, 24, 1, 2, 2), (1, 24, 2, 1, 2), (1, 24, 2, 2, 1)):
            assert f(dims=dims) == L.BDS_EINVAL, dims
        assert f(x=None) == L.BDS_EINVAL and f(terms=None) == L.BDS_EINVAL
    assert vfwd(temp=None) == L.BDS_EINVAL and vfwd(nb=15) == L.BDS_EINVAL
    assert lib.bds_voxel_reg_temp_bytes(8, 16, 64, 64) == 16 * (8 * 16 * 64 * 64 // 256)


def test_cpu_tensors_raise_and_degenerate_shapes_are_refused():
    d = R.make_knn(2, 10, 3)
    kw = {k: d[k] for k in R.GROUPS}
    with pytest.raises(L.BdsError):
        smpl_reg.knn_reg(d["nn_ind"], d["present"], **kw)
    with pytest.raises(L.BdsError):
        smpl_reg.voxel_reg(torch.zeros(1, 24, 2, 2, 2))
    with pytest.raises(ValueError, match="K = 1"):
        smpl_reg.knn_reg(d["nn_ind"][:, :, :1], d["present"], **kw)
    for shape in ((1, 24, 1, 2, 2), (1, 24, 2, 1, 2), (1, 24, 2, 2, 1), (1, 65, 2, 2, 2)):
        with pytest.raises(ValueError):
            smpl_reg.voxel_reg(torch.zeros(shape))
    with pytest.raises(ValueError):
        smpl_reg.knn_reg(d["nn_ind"], d["present"], features_dc=d["features_dc"][:, :2])


def _node(frame=0, **kw):
    d = R.make_knn(2, 12, 3, seed=5)
    frames = torch.tensor([[True, True], [True, False], [False, False]])
    return R.StandInNodes(d, R.make_field((2, 24, 2, 2, 3), seed=6)["field"], "cpu", frames=frames, cur_frame=frame, **kw)


def test_install_and_uninstall_restore_the_class_and_cpu_tensors_keep_its_method():
    class Nodes(R.StandInNodes):
        pass

    class Other(R.StandInNodes):
        pass
    assert "compute_reg_loss" not in Nodes.__dict__ and not hasattr(Nodes, "_bds_reference_compute_reg_loss")
    smpl_reg.install(Nodes)
    assert Nodes.compute_reg_loss is smpl_reg.smpl_compute_reg_loss and Nodes._bds_reference_compute_reg_loss is R.StandInNodes.compute_reg_loss
    assert Other.compute_reg_loss is R.StandInNodes.compute_reg_loss
    d = R.make_knn(2, 12, 3, seed=5)
    field = R.make_field((2, 24, 2, 2, 3), seed=6)["field"]
    got, ref = R.loss_and_grads(Nodes(d, field, "cpu")), R.loss_and_grads(R.StandInNodes(d, field, "cpu"))      # CPU tensors: the class's own method
    assert list(got[0]) == list(ref[0]) and got[0] == ref[0] and all(np.array_equal(got[1][k], ref[1][k]) for k in ref[1])
    smpl_reg.install(Nodes)                      # twice: still one original
    smpl_reg.uninstall(Nodes)
    assert "compute_reg_loss" not in Nodes.__dict__ and not hasattr(Nodes, "_bds_reference_compute_reg_loss")
    assert Nodes.compute_reg_loss is R.StandInNodes.compute_reg_loss


@pytest.mark.parametrize("variant", ["all", "no-x-offset", "frozen-rest-and-q", "additional", "absent-frame", "only-others"])
def test_installed_method_composes_the_dict_like_the_class(monkeypatch, variant):
    """The composition on the CPU, with the two fused ops stood in for by the framework expressions: the reference's keys in the
    reference's order, the other terms untouched, each op called once, the config back in place."""
    class Nodes(R.StandInNodes):
        pass
    calls = []

    def knn(nn_ind, present, reverse=None, **kw):
        calls.append("knn")
        assert reverse is not None and reverse[2].dtype == torch.int32
        return smpl_reg.framework_knn_reg(nn_ind, present, **kw)

    def vox(field):
        calls.append("vox")
        return smpl_reg.framework_voxel_reg(field)
    monkeypatch.setattr(smpl_reg, "knn_reg", knn)
    monkeypatch.setattr(smpl_reg, "voxel_reg", vox)
    monkeypatch.setattr(smpl_reg, "_on_device", lambda node: True)
    kw = dict(freeze=("rest", "q")) if variant == "frozen-rest-and-q" else {}
    if variant == "additional":
        kw["extra"] = R.make_field((2, 5, 2, 2, 3), seed=8)["field"]

    def make(cls):
        node = _node(frame={"absent-frame": 2}.get(variant, 1), **kw)
        node.__class__ = cls
        if variant == "no-x-offset":
            node.reg_cfg = R.Ns({k: v for k, v in node.reg_cfg.items() if k != "x_offset"})
        if variant == "only-others":
            node.reg_cfg = R.Ns({k: v for k, v in node.reg_cfg.items() if k not in smpl_reg.HIDDEN})
        return node
    ref_node, node = make(R.StandInNodes), make(Nodes)
    cfg = node.reg_cfg
    smpl_reg.install(Nodes)
    try:
        got = R.loss_and_grads(node)
    finally:
        smpl_reg.uninstall(Nodes)
    ref = R.loss_and_grads(ref_node)
    assert node.reg_cfg is cfg
    assert list(got[0]) == list(ref[0]), (list(got[0]), list(ref[0]))
    expect = {"all": ["max_s_square", "smpl_temporal_smooth", "voxel_deformer_reg", *smpl_reg.KEYS, "x_offset"], "absent-frame": ["max_s_square"],
              "only-others": ["max_s_square", "smpl_temporal_smooth", "x_offset"]}.get(variant)
    if expect is not None:
        assert list(got[0]) == expect
    for k in ref[0]:
        assert got[0][k] == pytest.approx(ref[0][k], rel=1e-6), k
    for k in ref[1]:
        np.testing.assert_allclose(got[1][k], ref[1][k], rtol=1e-5, atol=1e-9, err_msg=k)
    want = {"absent-frame": [], "only-others": [], "additional": ["vox", "vox", "knn"]}.get(variant, ["vox", "knn"])
    assert calls == want, calls
