"""Pose transform of the node classes on the MI355X (csrc/nodes.hip through bilateral_driving_amd/nodes.py): the fused op against the
reference-generated golden vectors (scripts/gen_golden_node_pose.py) and against the float64 restatement (tests/node_pose_ref64.py)
over sizes and instance counts; the interpolated (test-set) form; determinism of the instance gradients; bad ids, NaN and zero
quaternions; and the install hook on stand-ins with the reference's RigidNodes / DeformableNodes attribute layout, through
rasterization()."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from tests.node_pose_ref64 import INPUTS, grads64, rel, tensors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OUTS = ("wm", "wq", "op")


@pytest.fixture(scope="module")
def Nd():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import nodes
    return nodes


def load(name):
    return np.load(os.path.join(GOLD, f"node_pose_{name}.npz"))


def fused(Nd, t, f, interpolate=False, grad=True):
    """Fused forward (+ backward of the weighted sum) on tensors dict t (float32, on the GPU) -> outputs, {name: grad}."""
    ts = {k: t[k].detach().clone().requires_grad_(grad) for k in INPUTS}
    wm, wq, op = Nd.pose_transform(ts["means"], ts["quats"], ts["logits"], t["point_ids"], ts["instances_quats"], ts["instances_trans"],
                                   t["instances_fv"], f, interpolate)
    g = {}
    if grad:
        ((wm * t["w_m"]).sum() + (wq * t["w_q"]).sum() + (op * t["w_o"]).sum()).backward()
        g = {k: v.grad for k, v in ts.items()}
    return (wm, wq, op), g


# ---- the reference's golden vectors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f_idx", range(4))
def test_fused_matches_reference_golden(Nd, f_idx):
    z = load("train")
    f = int(z["frames"][f_idx])
    outs, g = fused(Nd, tensors(z, torch.float32, "cuda"), f)
    for o, k in zip(outs, OUTS):
        np.testing.assert_allclose(o.detach().cpu().numpy(), z[f"f{f}_{k}"], rtol=1e-5, atol=1e-6 if k != "wm" else 1e-5)
    for k in ("means", "quats", "logits"):
        assert rel(z[f"f{f}_grad_{k}"], g[k].cpu().numpy()) < 1e-5, k
    for k in ("instances_quats", "instances_trans"):
        gk = g[k].cpu().numpy()
        assert rel(z[f"f{f}_grad_{k}"], gk) < 1e-4, k
        assert np.abs(np.delete(gk, f, axis=0)).max() == 0.0


@pytest.mark.parametrize("f_idx", range(4))
def test_interpolated_forward_matches_golden(Nd, f_idx):
    z = load("interp")
    F = z["instances_fv"].shape[0]
    f = int(z["frames"][f_idx])
    interp = Nd.interpolates(True, f, F)
    with torch.no_grad():
        outs, _ = fused(Nd, tensors(z, torch.float32, "cuda"), f, interp, grad=False)
    for o, k in zip(outs, OUTS):
        np.testing.assert_allclose(o.cpu().numpy(), z[f"f{f}_{k}"], rtol=1e-5, atol=2e-5 if k == "wm" else 1e-6)


def test_interpolated_backward_raises(Nd):
    z = load("interp")
    t = tensors(z, torch.float32, "cuda")
    with pytest.raises(RuntimeError, match="interpolated"):
        fused(Nd, t, int(z["instances_fv"].shape[0]) - 2, True)


# ---- float64 over sizes and instance counts ---------------------------------------------------------------------------------------
def random_case(N, I, F=6, seed=0, shuffle=True):
    g = torch.Generator().manual_seed(seed * 1000 + N % 997 + I)
    ids = torch.randint(0, I, (N,), generator=g)
    if not shuffle:
        ids = torch.sort(ids).values
    d = dict(means=(torch.rand(N, 3, generator=g) - 0.5) * 6, quats=torch.randn(N, 4, generator=g), logits=torch.randn(N, 1, generator=g),
             instances_quats=torch.randn(F, I, 4, generator=g), instances_trans=torch.randn(F, I, 3, generator=g) * 10,
             w_m=torch.randn(N, 3, generator=g), w_q=torch.randn(N, 4, generator=g), w_o=torch.randn(N, 1, generator=g))
    d["instances_fv"] = torch.rand(F, I, generator=g) > 0.2
    d["point_ids"] = ids[:, None]
    return d


def on(d, dev="cuda", dtype=torch.float32):
    return {k: (v.to(dev) if v.dtype in (torch.int64, torch.bool) else v.to(device=dev, dtype=dtype)) for k, v in d.items()}


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 5000, 300000])
@pytest.mark.parametrize("I", [1, 7, 300])
def test_fused_matches_float64(Nd, N, I):
    d = random_case(N, I)
    f = 3
    outs, g = fused(Nd, on(d), f)
    r_outs, r_g = grads64(on(d, "cpu", torch.float64), f)
    for o, r in zip(outs, r_outs):
        assert o.shape == r.shape
        if N:
            np.testing.assert_allclose(o.detach().cpu().numpy(), r, rtol=1e-5, atol=1e-5)
    for k in INPUTS:
        gk = g[k].cpu().numpy()
        assert gk.shape == r_g[k].shape, k
        if N == 0:
            assert np.abs(gk).max(initial=0.0) == 0.0
            continue
        tol = 1e-4 if k.startswith("instances") else 1e-5
        assert rel(r_g[k], gk) < tol, (k, rel(r_g[k], gk))


def test_instance_gradients_are_deterministic(Nd):
    d = on(random_case(300000, 64, seed=5))
    (_, g1), (_, g2) = fused(Nd, d, 2), fused(Nd, d, 2)
    for k in INPUTS:
        assert torch.equal(g1[k], g2[k]), k
    assert float(g1["instances_quats"].abs().sum()) > 0


# ---- bad input ---------------------------------------------------------------------------------------------------------------------
def test_out_of_range_id_is_reported_not_read(Nd):
    d = on(random_case(5000, 7, seed=7))
    for bad in (7, -1, 1 << 40):
        ids = d["point_ids"].clone()
        ids[1234, 0] = bad
        with pytest.raises(IndexError, match="outside"):
            Nd.pose_transform(d["means"], d["quats"], d["logits"], ids, d["instances_quats"], d["instances_trans"], d["instances_fv"], 2)
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        wm, wq, op = Nd.pose_transform(d["means"], d["quats"], d["logits"], ids, d["instances_quats"], d["instances_trans"],
                                       d["instances_fv"], 2, flags=flags)
        assert flags.tolist() == [0, 1]
        assert torch.isnan(wm[1234]).all() and torch.isnan(op[1234]).all()
        ok = torch.ones(5000, dtype=torch.bool, device="cuda")
        ok[1234] = False
        r = Nd.framework_transform(d["means"][ok], d["quats"][ok], d["logits"][ok], ids[ok], d["instances_quats"], d["instances_trans"],
                                   d["instances_fv"], 2)
        torch.testing.assert_close(wm[ok], r[0], rtol=1e-5, atol=1e-5)


# ---- stand-ins with the reference's attribute layout -------------------------------------------------------------------------------
def _act(x):
    return x / x.norm(dim=-1, keepdim=True)


class StandInRigid(nn.Module):
    """RigidNodes' attribute layout (models/nodes/rigid.py); get_gaussians is the framework restatement of :445-493."""

    def __init__(self, N, I, F, seed, sh_degree=1):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        from tests.util import make_scene
        sc = make_scene(N, 96, 64, seed=seed)
        self.scene = sc
        self.point_ids = torch.randint(0, I, (N, 1), generator=g).cuda()
        q = torch.tensor([1.0, 0.0, 0.0, 0.0]) + 0.05 * torch.randn(F, I, 4, generator=g)
        self.instances_quats = nn.Parameter(q.cuda())
        self.instances_trans = nn.Parameter((0.05 * torch.randn(F, I, 3, generator=g)).cuda())
        fv = torch.rand(F, I, generator=g) > 0.2
        fv[:, 0] = True
        self.instances_fv = fv.cuda()
        self._means = nn.Parameter(sc["means"].cuda())
        self._quats = nn.Parameter(sc["quats"].cuda())
        self._scales = nn.Parameter(torch.log(sc["scales"]).cuda())
        self._opacities = nn.Parameter(torch.logit(sc["opacities"]).reshape(N, 1).cuda())
        K = (sh_degree + 1) ** 2
        self._features_dc = nn.Parameter((torch.rand(N, 3, generator=g) - 0.5).cuda())
        self._features_rest = nn.Parameter((0.1 * torch.randn(N, K - 1, 3, generator=g)).cuda())
        self.sh_degree, self.step, self.cur_frame, self.in_test_set = sh_degree, 7, 2, False
        self.ctrl_cfg = SimpleNamespace(sh_degree_interval=1, use_deformgs_for_nonrigid=True, use_deformgs_after=0,
                                        stop_optimizing_canonical_xyz=True)

    @property
    def num_frames(self):
        return self.instances_fv.shape[0]

    @property
    def get_scaling(self):
        return torch.exp(self._scales)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacities)

    @property
    def get_quats(self):
        return _act(self._quats)

    def quat_act(self, x):
        return _act(x)

    def _finish(self, cam, world_means, world_quats, opac, scales):
        from bilateral_driving_amd import gs_ops
        colors = torch.cat((self._features_dc[:, None, :], self._features_rest), dim=1)
        if self.sh_degree > 0:
            viewdirs = world_means.detach() - cam.camtoworlds.data[..., :3, 3]
            viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
            n = min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree)
            rgbs = torch.clamp(gs_ops.spherical_harmonics(n, viewdirs, colors) + 0.5, 0.0, 1.0)
        else:
            rgbs = torch.sigmoid(colors[:, 0, :])
        gs = dict(_means=world_means, _opacities=opac, _rgbs=rgbs, _scales=scales, _quats=world_quats)
        for k, v in gs.items():
            if torch.isnan(v).any():
                raise ValueError(f"NaN detected in gaussian {k} at step {self.step}")
            if torch.isinf(v).any():
                raise ValueError(f"Inf detected in gaussian {k} at step {self.step}")
        return gs

    def _transform(self, means, quats):
        from bilateral_driving_amd import nodes
        interp = nodes.interpolates(self.in_test_set, self.cur_frame, self.num_frames)
        return nodes.framework_transform(means, quats, self._opacities, self.point_ids, self.instances_quats, self.instances_trans,
                                         self.instances_fv, self.cur_frame, interp)

    def get_gaussians(self, cam):
        self.filter_mask = torch.ones_like(self._means[:, 0], dtype=torch.bool)
        wm, wq, op = self._transform(self._means, self._quats)
        scales = self.get_scaling
        gs = self._finish(cam, wm, wq, op, scales)
        self._gs_cache = {"_scales": scales}
        return gs


class StandInDeformable(StandInRigid):
    """DeformableNodes' layout (models/nodes/deformable.py): get_deformation through the deformation network (deform.py's fused
    ConditionalDeformNetwork), get_gaussians the framework restatement of :49-114."""

    def __init__(self, N, I, F, seed):
        super().__init__(N, I, F, seed)
        from bilateral_driving_amd import deform
        g = torch.Generator().manual_seed(seed + 1)
        self.deform_network = deform.ConditionalDeformNetwork(D=8, W=256, input_ch=3, embed_dim=16, deform_quat=True,
                                                              deform_scale=False).cuda()
        with torch.no_grad():
            for n_, p in self.deform_network.named_parameters():
                p.mul_(0.05 if "gaussian" in n_ else 1.0)
        self.instances_embedding = nn.Parameter((0.5 * torch.randn(I, 16, generator=g)).cuda())
        self.instances_size = (torch.rand(I, 3, generator=g) * 2 + 1).cuda()
        self.normalized_timestamps = torch.linspace(0, 1, F).cuda()

    def get_deformation(self, local_means):
        emb = self.instances_embedding[self.point_ids[..., 0]]
        h = self.instances_size[self.point_ids[..., 0]][..., 2]
        x = local_means.data / h[:, None] * 2
        t = self.normalized_timestamps[self.cur_frame].unsqueeze(0).repeat(self.point_ids.shape[0], 1)
        return self.deform_network(x, t, emb)

    def get_gaussians(self, cam):
        self.filter_mask = torch.ones_like(self._means[:, 0], dtype=torch.bool)
        dx, dq, ds = self.get_deformation(local_means=self._means)
        means = self._means.data + dx if self.ctrl_cfg.stop_optimizing_canonical_xyz else self._means + dx
        wm, wq, op = self._transform(means, self.get_quats + dq)
        scales = self.get_scaling + ds if ds is not None else self.get_scaling
        gs = self._finish(cam, wm, wq, op, scales)
        self._gs_cache = {"_scales": scales, "local_xyz_deformed": means}
        return gs


def _cam(m):
    vm = m.scene["viewmats"][0].cuda()
    return SimpleNamespace(camtoworlds=torch.linalg.inv(vm)[None])


def _render_loss(m, gs):
    from bilateral_driving_amd import rendering as R
    img, alpha, _ = R.rasterization(gs["_means"], gs["_quats"], gs["_scales"], gs["_opacities"].squeeze(-1), gs["_rgbs"],
                                    m.scene["viewmats"].cuda(), m.scene["Ks"].cuda(), 96, 64)
    wimg = torch.linspace(0, 1, img.numel(), device=img.device).reshape(img.shape)
    return (img * wimg).sum() + alpha.sum()


@pytest.mark.parametrize("cls", [StandInRigid, StandInDeformable])
def test_install_hook_matches_framework_through_rasterization(Nd, cls):
    def run(hooked):
        torch.manual_seed(0)
        m = cls(3000, 5, 6, seed=11)
        if hooked:
            Nd.install(cls)
        try:
            gs = m.get_gaussians(_cam(m))
            cache = dict(m._gs_cache)
            _render_loss(m, gs).backward()
        finally:
            if hooked:
                Nd.uninstall(cls)
        return gs, cache, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, m

    ref_gs, ref_cache, ref_g, _ = run(False)
    got_gs, got_cache, got_g, m = run(True)
    assert cls.get_gaussians is not Nd.rigid_get_gaussians and cls.get_gaussians is not Nd.deformable_get_gaussians
    assert m.filter_mask.all() and m.filter_mask.shape == (3000,)
    assert list(got_gs) == list(ref_gs) and sorted(got_cache) == sorted(ref_cache)
    for k in ref_gs:
        torch.testing.assert_close(got_gs[k], ref_gs[k], rtol=1e-5, atol=2e-5)
    for k, v in ref_cache.items():
        torch.testing.assert_close(got_cache[k], v, rtol=1e-5, atol=2e-5)
    assert sorted(got_g) == sorted(ref_g)
    for k in ref_g:
        assert float(ref_g[k].norm()) > 0, k
        assert rel(ref_g[k].cpu().numpy(), got_g[k].cpu().numpy()) < 2e-3, k


def test_install_and_uninstall_restore_the_original(Nd):
    class A(StandInRigid):
        pass

    class B(StandInDeformable):
        pass
    orig_a, orig_b = A.get_gaussians, B.get_gaussians
    Nd.install(A)
    Nd.install(B)
    assert A.get_gaussians is Nd.rigid_get_gaussians and B.get_gaussians is Nd.deformable_get_gaussians
    assert A._bds_reference_get_gaussians is orig_a and B._bds_reference_get_gaussians is orig_b
    Nd.install(A)                     # twice: the original is kept
    assert A._bds_reference_get_gaussians is orig_a
    Nd.uninstall(A)
    Nd.uninstall(B)
    assert A.get_gaussians is orig_a and B.get_gaussians is orig_b


@pytest.mark.parametrize("what,msg", [
    ("nan_mean", "NaN detected in gaussian _means at step 7"),
    ("zero_point_quat", "NaN detected in gaussian _quats at step 7"),
    ("zero_instance_quat", "NaN detected in gaussian _means at step 7"),
    ("inf_trans", "Inf detected in gaussian _means at step 7"),
    ("nan_logit", "NaN detected in gaussian _opacities at step 7"),
])
def test_nonfinite_inputs_raise_the_reference_message(Nd, what, msg):
    m = StandInRigid(2000, 4, 6, seed=3)
    with torch.no_grad():
        if what == "nan_mean":
            m._means[17, 1] = float("nan")
        elif what == "zero_point_quat":
            m._quats[5] = 0.0
        elif what == "zero_instance_quat":
            m.instances_quats[m.cur_frame, int(m.point_ids[0, 0])] = 0.0
        elif what == "inf_trans":
            m.instances_trans[m.cur_frame, int(m.point_ids[0, 0])] = float("inf")
        else:
            m._opacities[9] = float("nan")
    for hooked in (False, True):
        if hooked:
            Nd.install(StandInRigid)
        try:
            with pytest.raises(ValueError) as e:
                m.get_gaussians(_cam(m))
            assert str(e.value) == msg
        finally:
            if hooked:
                Nd.uninstall(StandInRigid)
