"""The SMPL nodes' kNN and skinning-field regularisers on the MI355X (csrc/smpl_reg.hip through bilateral_driving_amd/smpl_reg.py)
against the float64 restatement (tests/smpl_reg_ref64.py), the reference-generated golden (scripts/gen_golden_smpl_reg.py) and the
framework expressions, on poisoned, recycled memory with guard bands (tests/poison.py), with every input and the incoming gradient
at 4-byte phases (tests/placement.py), twice for the bit-equality the ops claim; and the install hook on a stand-in with SMPLNodes'
attribute layout.

Bounds (tests/smpl_reg_ref64.py): per compared tensor (each term, each gradient), the largest difference over the tensor's largest
reference magnitude is held to 2 x the float32 framework expression's own such error against float64 on the same inputs (run on the
CPU: its order of summation is fixed there) + FLOOR.  FLOOR = 2.3e-6 is the host shim's largest error over the same cases, measured on
the CPU by tests/test_smpl_reg_cpu.py (the opacity gradient at K = 2).  A reference that is exactly zero (constant attributes,
all-self neighbourhoods, the zero field, absent instances, unlisted rows) is held exactly."""
import os

import numpy as np
import pytest
import torch

from tests import placement, poison
from tests import smpl_reg_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "smpl_reg.npz")
PARAMS = ("_features_dc", "_features_rest", "_opacities", "_scales", "_quats")


@pytest.fixture(scope="module")
def S():
    from bilateral_driving_amd import smpl_reg
    return smpl_reg


def fused_knn(S, d, off=0):
    """knn_reg on the GPU with every input ``off`` elements behind an aligned base (bytes and int64: their own phases) and the incoming
    gradient re-placed likewise -> (terms, grads) in run_knn's layout."""
    byte_off, long_off = (0, 0) if off == 0 else (placement.OFFSETS[torch.bool][off % 2], placement.OFFSETS[torch.int64][0])
    ts = {k: placement.placed(d[k].cuda(), off).requires_grad_(True) for k in R.GROUPS if d[k] is not None}
    nn, present = placement.placed(d["nn_ind"].cuda(), long_off), placement.placed(d["present"].cuda(), byte_off)
    terms = S.knn_reg(nn, present, **ts)
    (placement.regrad(terms, off) * d["w"].cuda()).sum().backward()
    assert all(t.grad is not None for t in ts.values())
    return terms.detach().cpu().numpy(), {k: t.grad.cpu().numpy() for k, t in ts.items()}


def fused_field(S, d, off=0):
    x = placement.placed(d["field"].cuda(), off).requires_grad_(True)
    terms = S.voxel_reg(x)
    (placement.regrad(terms, off) * d["w"].cuda()).sum().backward()
    return terms.detach().cpu().numpy(), x.grad.cpu().numpy()


def poisoned_twice(run, name):
    """``run()`` plainly and inside poisoned allocations: nothing unwritten, no guard touched, the two results bit-equal."""
    plain = run()
    torch.cuda.synchronize()
    with poison.poisoned_allocations(True, name=name) as pz:
        got = run()
        torch.cuda.synchronize()
        assert len(pz.records) >= 3
    flat = lambda r: [("terms", r[0])] + (list(r[1].items()) if isinstance(r[1], dict) else [("field", r[1])])
    for (k, a), (_, b) in zip(flat(got), flat(plain)):
        assert not bool(poison.holds_poison(torch.as_tensor(a)).any()), k
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), k
    return got


@pytest.mark.parametrize("case", list(R.CASES))
def test_knn_terms_and_gradients_match_float64(S, case):
    d = R.make_knn(seed=len(case), **R.CASES[case])
    ref = R.knn_ref(d)
    b = R.bounds(R.errors(R.run_knn(d, dtype=torch.float32), ref))
    off = 1 + list(R.CASES).index(case) % 3
    got = poisoned_twice(lambda: fused_knn(S, d, off), "smpl knn_reg " + case)
    e = R.errors(got, ref)
    print(f"\nsmpl knn_reg {case} (phase {4 * off}): worst error {max(e.values()):.3e} ({max(e, key=e.get)}), its bound {b[max(e, key=e.get)]:.3e}")
    assert R.within(e, b), {k: (e[k], b[k]) for k in b if e[k] > b[k]}
    terms, grads = got
    I, V, K = d["nn_ind"].shape
    for k, g in grads.items():
        g = g.reshape(I, V, -1)
        for i in R.CASES[case].get("absent", ()):
            assert not g[i].any(), (k, i)                                  # an absent instance's rows: written zeros
        if R.CASES[case].get("nn") != "self":
            assert not g[:, 1].any(), k                                    # the row nobody lists: written zeros
    for g, name in enumerate(R.GROUPS):
        assert (terms[g] == 0) == (d[name] is None or case in ("self", "constant")), (name, terms[g])
    if case in ("self", "constant"):                                       # std exactly 0: gradient exactly 0, nothing NaN
        assert all(not g.any() for g in grads.values())


def test_knn_at_every_phase_and_aligned(S):
    d = R.make_knn(2, 70, 3, seed=11)
    ref = R.knn_ref(d)
    b = R.bounds(R.errors(R.run_knn(d, dtype=torch.float32), ref))
    runs = [fused_knn(S, d, off) for off in (0, 1, 2, 3)]
    for r in runs:
        assert R.within(R.errors(r, ref), b)
        assert np.array_equal(r[0], runs[0][0]) and all(np.array_equal(r[1][k], runs[0][1][k]) for k in r[1])      # the phase changes no bit


def test_knn_with_every_instance_absent_is_zero(S):
    d = R.make_knn(3, 70, 3, seed=2, absent=(0, 1, 2))
    terms, grads = poisoned_twice(lambda: fused_knn(S, d, 1), "smpl knn_reg all absent")
    assert not terms.any() and all(not g.any() for g in grads.values())


def test_knn_refuses_one_neighbour_bad_indices_and_cpu_tensors(S):
    from bilateral_driving_amd import _lib as L
    d = R.make_knn(2, 20, 3)
    kw = {k: d[k].cuda() for k in R.GROUPS}
    with pytest.raises(ValueError, match="K = 1"):
        S.knn_reg(d["nn_ind"][:, :, :1].cuda(), d["present"].cuda(), **kw)
    for bad in (-1, 20):
        nn = d["nn_ind"].clone()
        nn[1, 3, 1] = bad
        with pytest.raises(IndexError):
            S.knn_reg(nn.cuda(), d["present"].cuda(), **kw)
    with pytest.raises(L.BdsError):
        S.knn_reg(d["nn_ind"].cuda(), d["present"].cuda(), **dict(kw, quats=d["quats"]))


@pytest.mark.parametrize("case", list(R.FIELD_CASES))
def test_field_terms_and_gradient_match_float64(S, case):
    d = R.make_field(R.FIELD_CASES[case], seed=len(case))
    ref = R.field_ref(d)
    b = R.bounds(R.errors(R.run_field(d, dtype=torch.float32), ref))
    off = 1 + list(R.FIELD_CASES).index(case) % 3
    got = poisoned_twice(lambda: fused_field(S, d, off), "smpl voxel_reg " + case)
    e = R.errors(got, ref)
    print(f"\nsmpl voxel_reg {case} (phase {4 * off}): worst error {max(e.values()):.3e} ({max(e, key=e.get)}), its bound {b[max(e, key=e.get)]:.3e}")
    assert R.within(e, b), (e, b)
    assert np.array_equal(fused_field(S, d, 0)[1], got[1])
    terms, grad = poisoned_twice(lambda: fused_field(S, R.make_field(R.FIELD_CASES[case], kind="zero"), off), "smpl voxel_reg zero " + case)
    assert not terms.any() and not grad.any()                              # sign(0) = 0, the zero vector's norm has gradient 0


def test_field_single_voxels_against_hand_derived_gradients(S):
    """One voxel of 0.5 in channel 0 of a [1,2,3,3,3] field (the derivation: tests/test_smpl_reg_cpu.py)."""
    for at, n_neighbours in (((0, 0, 0), 3), ((1, 1, 1), 6)):
        x = torch.zeros(1, 2, 3, 3, 3)
        x[(0, 0) + at] = 0.5
        terms, grad = fused_field(S, dict(field=x, w=torch.tensor([1.0, 1.0])), 1)
        unit = 1.0 / (3 * 2 * 18)
        np.testing.assert_allclose(grad[(0, 0) + at], n_neighbours * unit + 1.0 / 27, rtol=1e-6)
        np.testing.assert_allclose(terms, [0.5 * n_neighbours * unit, 0.5 / 27], rtol=1e-6)
        for ax in range(3):
            for step in (-1, 1):
                nb = list(at)
                nb[ax] += step
                if 0 <= nb[ax] < 3:
                    np.testing.assert_allclose(grad[(0, 0) + tuple(nb)], -unit, rtol=1e-6)
        assert np.count_nonzero(grad) == 1 + n_neighbours and not grad[0, 1].any()


def test_field_refuses_degenerate_shapes(S):
    for shape in ((1, 24, 1, 4, 4), (1, 24, 4, 1, 4), (1, 24, 4, 4, 1), (1, 65, 2, 2, 2)):
        with pytest.raises(ValueError):
            S.voxel_reg(torch.zeros(shape, device="cuda"))


# ---- the install hook --------------------------------------------------------------------------------------------------------------
FREEZE = dict(dc="features_dc", rest="features_rest", o="opacities", s="scales", q="quats")
OTHERS = ("smpl_temporal_smooth", "x_offset")


def _golden():
    z = np.load(GOLD)
    d = {k: torch.from_numpy(z[k]) for k in R.GROUPS}
    d.update(nn_ind=torch.from_numpy(z["nn_ind"].astype(np.int64)), w=None)
    return z, d, torch.from_numpy(z["field"]), torch.from_numpy(z["instances_fv"])


def hook_case(S, d, field, frames, frame, extra=None, freeze=()):
    """compute_reg_loss of a stand-in (without the parent's scale term, so every gradient below is the two terms' alone) by the class's
    own method (framework ops on the GPU) and by the installed one, twice; the float64 values and gradients of the two terms.
    Asserts the keys, the untouched other terms, the bounds and the bit-equality -> (values, gradients, float64 values, float64
    gradients)."""
    class Nodes(R.StandInNodes):
        pass

    def make(cls):
        node = cls(d, field, "cuda", frames=frames, cur_frame=frame, extra=extra, freeze=freeze)
        node.reg_cfg = R.Ns({k: v for k, v in node.reg_cfg.items() if k != "max_s_square_reg"})
        return node
    lam = np.array([R.LAMBDAS[k] for k in S.LAMBDAS])
    live = dict(d, present=frames[frame], w=torch.from_numpy(lam), **{FREEZE[k]: None for k in freeze})
    k_ref = R.knn_ref(live)
    want_g = {attr: k_ref[1].get(name, np.zeros(tuple(d[name].shape))) for attr, name in zip(PARAMS, R.GROUPS)}
    want_v = {key: k_ref[0][k] * lam[k] for k, key in enumerate(S.KEYS) if live[R.GROUPS[k]] is not None}
    vox = 0.0
    for name, t, ws in (("voxel_w_correction", field, ("lambda_std_w", "lambda_w_norm")), ("additional_correction", extra, ("lambda_std_w_rest", "lambda_w_rest_norm"))):
        if t is not None:
            w = torch.tensor([R.VOX[ws[0]], R.VOX[ws[1]]])
            terms, want_g[name] = R.field_ref(dict(field=t, w=w))
            vox += float((terms * w.double().numpy()).sum())
    want_v["voxel_deformer_reg"] = vox
    ref_vals, ref_g = R.loss_and_grads(make(R.StandInNodes))
    node = make(Nodes)
    S.install(Nodes)
    try:
        vals, g = R.loss_and_grads(node)
        again = R.loss_and_grads(node)
    finally:
        S.uninstall(Nodes)
    assert list(vals) == list(ref_vals) == [OTHERS[0], "voxel_deformer_reg", *[k for k in S.KEYS if k in want_v], OTHERS[1]]
    for k in OTHERS:                     # the class's own code, the same launches
        assert vals[k] == ref_vals[k], k
    for k, want in want_v.items():       # |fused - float64| <= 2 |framework - float64| + FLOOR |float64|
        assert abs(vals[k] - want) <= 2 * abs(ref_vals[k] - want) + R.FLOOR * abs(want), (k, vals[k], ref_vals[k], want)
    for k, want in want_g.items():
        e32, e = R.err(ref_g[k], want), R.err(g[k], want)
        print(f"\nsmpl reg hook {k}: framework vs float64 {e32:.3e}, fused {e:.3e}")
        assert e <= 2 * e32 + R.FLOOR, (k, e, e32)
        assert R.err(g[k], ref_g[k]) <= 3 * e32 + R.FLOOR, k          # so the two agree within the bound plus the framework's own distance
        assert np.array_equal(g[k].view(np.int32), again[1][k].view(np.int32)), k      # bit-equal run to run
    assert all(vals[k] == again[0][k] for k in want_v)
    assert node.__dict__["_bds_knn_reverse"][0] is node.nn_ind and "_bds_fv_host" in node.__dict__      # built once, kept on the node
    return vals, g, want_v, want_g


@pytest.mark.parametrize("frame", [0, 1])
def test_installed_method_matches_the_reference_golden_and_the_framework(S, frame):
    z, d, field, frames = _golden()
    vals, g, want_v, want_g = hook_case(S, d, field, frames, frame)
    gold = dict(zip((str(k) for k in z[f"f{frame}_keys"]), z[f"f{frame}_values"]))
    assert sorted(gold) == sorted(want_v)
    for k, want in want_v.items():       # the same rule with the golden (the reference's own float32 run) as the float32 side
        assert abs(vals[k] - want) <= 2 * abs(float(gold[k]) - want) + R.FLOOR * abs(want), (k, vals[k], float(gold[k]), want)
    for attr in PARAMS + ("_field",):
        k = "voxel_w_correction" if attr == "_field" else attr
        assert R.err(g[k], want_g[k]) <= 2 * R.err(z[f"f{frame}_grad{attr}"], want_g[k]) + R.FLOOR, attr
        if frame == 1 and attr != "_field":
            assert not g[k][96:].any(), attr                               # the absent instance's rows


@pytest.mark.parametrize("variant", ["balls", "additional-correction", "frozen"])
def test_installed_method_variants_match_float64_and_the_class(S, variant):
    d = R.make_knn(2, 70, 3, seed=21, S=1 if variant == "balls" else 3)
    field = R.make_field((2, 24, 2, 3, 5), seed=22)["field"]
    extra = R.make_field((2, 5, 2, 3, 5), seed=23)["field"] if variant == "additional-correction" else None
    vals, g, _, _ = hook_case(S, d, field, torch.tensor([[True, True]]), 0, extra=extra, freeze=("dc", "s") if variant == "frozen" else ())
    if variant == "frozen":
        assert "knn_reg_dc" not in vals and "knn_reg_s" not in vals and not g["_features_dc"].any() and not g["_scales"].any()
    if variant == "balls":
        assert g["_scales"].shape == (140, 1) and g["_scales"].any()


def test_installed_method_returns_early_when_nobody_is_present(S):
    class Nodes(R.StandInNodes):
        pass
    d = R.make_knn(2, 20, 3, seed=4)
    node = Nodes(d, R.make_field((2, 24, 2, 2, 2))["field"], "cuda", frames=torch.tensor([[True, True], [False, False]]), cur_frame=1)
    S.install(Nodes)
    try:
        out = node.compute_reg_loss()
    finally:
        S.uninstall(Nodes)
    assert list(out) == ["max_s_square"] and "_bds_knn_reverse" not in node.__dict__
