"""Shared by tests/test_smpl_skin_cpu.py and tests/test_gpu_55_smpl_skin.py (test infrastructure): synthetic humans for the SMPL nodes'
pose chain and skinning, ``bilateral_driving_amd.smpl.framework_transform`` evaluated with autograd in a chosen precision (float64:
the restatement every comparison is made against) and the error bound both files use.

The bound is MEASURED, not fixed: the worst error of framework_transform in float32 on the CPU against itself in float64 over the same
inputs (outputs and gradients; each tensor's largest error divided by max(1, the tensor's largest reference magnitude)), times 4 --
the factor covers another summation order and FMA contraction of equally accurate arithmetic -- with a floor of 1e-6.

Inputs are settled: matrix_to_quaternion picks the candidate with the largest q_abs and flips the sign to w >= 0, two decisions that
must not hang on float32 rounding.  A point whose two largest q_abs lie within GAP of each other in float64, or whose real part is
smaller than GAP, is drawn again (no row is excluded from a comparison)."""
import numpy as np
import torch

from bilateral_driving_amd import p3d
from bilateral_driving_amd.smpl import JOINTS, SMPL_PARENTS, framework_transform, frame_pose, normalize_coords, rigid_chain

GAP = 1e-4
PERMUTED_PARENTS = (-1, 0, 1, 0, 2, 1, 5, 3, 3, 8, 4, 10, 6, 6, 12, 9, 15, 11, 14, 14, 7, 20, 16, 0)     # valid: parents[j] < j
FIELDS = ((2, 2, 2), (3, 5, 7), (4, 16, 16))
INPUTS = ("means", "quats", "instances_quats", "smpl_quats", "instances_trans", "voxel_corr")


def template_kwargs(d, dtype=None, device=None):
    """The keyword arguments of framework_transform / skin_transform from an input dict."""
    conv = lambda t: None if t is None else t.to(dtype=dtype or t.dtype, device=device or t.device)
    kw = dict(J_canonical=conv(d["J_canonical"]), A0_inv=conv(d["A0_inv"]), parents=d["parents"])
    if d.get("voxel_base") is not None:
        kw.update(voxel_base=conv(d["voxel_base"]), offset=conv(d["offset"]), scale=conv(d["scale"]), ratio=d["ratio"], ratio_dim=d["ratio_dim"])
    else:
        kw.update(W=conv(d["W"]))
    return kw


def blend_margins(d, f, interpolate=False):
    """float64: per point of the present instances (q_abs gap between the two largest candidates, |real part| of the quaternion)."""
    t = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
    mask = t["instances_fv"][f]
    I = mask.shape[0]
    theta, _ = frame_pose(t["instances_quats"], t["smpl_quats"], t["instances_trans"], t["instances_fv"], f, interpolate)
    theta = theta[mask] / theta[mask].norm(dim=-1, keepdim=True)
    A = rigid_chain(p3d.quaternion_to_matrix(theta), t["J_canonical"][mask], t["parents"]) @ t["A0_inv"][mask]
    x = t["means"].reshape(I, -1, 3)
    if t.get("voxel_base") is not None:
        grid = normalize_coords(x, t["offset"], t["scale"], t["ratio"], t["ratio_dim"])[:, :, None, None]
        w = torch.nn.functional.grid_sample(t["voxel_base"] + t["voxel_corr"], grid, align_corners=True, mode="bilinear", padding_mode="border")
        w = w.squeeze(4).squeeze(3).permute(0, 2, 1)[mask]
    else:
        w = t["W"][mask]
    R = torch.einsum("bnj,bjrc->bnrc", w, A)[..., :3, :3]
    m00, m11, m22 = R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]
    q_abs = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1).clamp(min=0).sqrt()
    top = q_abs.topk(2, dim=-1).values
    real = p3d.matrix_to_quaternion(R)[..., 0].abs()
    gap, rl = torch.full(x.shape[:2], np.inf, dtype=torch.float64), torch.full(x.shape[:2], np.inf, dtype=torch.float64)
    gap[mask], rl[mask] = top[..., 0] - top[..., 1], real
    return gap, rl


def make_inputs(I, V, dhw, seed, parents=SMPL_PARENTS, absent=(), F=3, frames=(1,), field=True, settle=True, compact=False):
    """Float32 inputs on the CPU (``compact``: quats and the field hold float16 values and the loss weights small integers, which a
    fixture stores in a quarter of the bytes).  offset and scale are binary fractions, so the points placed on the upper faces (the first of every
    instance with V >= 4: x, y and -- where the ratio is a power of two -- z at normalised 1) sit there exactly; about a quarter of the
    points lie outside the box on some axis."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    d_, h_, w_ = dhw
    ratio = h_ / d_
    offset = torch.round(n(I, 1, 3) * 4) / 8
    scale = 2.0 ** torch.randint(-1, 2, (I, 1, 1), generator=g).float()

    def draw(rows):
        u = (r(rows, 3) * 2 - 1) * 1.1
        u[:, 2] /= ratio
        return u

    u = draw(I * V).reshape(I, V, 3)
    exact_z = float(np.log2(ratio)).is_integer()
    if V >= 4:
        u[:, 0, 0] = 1.0
        u[:, 1, 1] = 1.0
        u[:, 2, 2] = 1.0 / ratio if exact_z else u[:, 2, 2]
        u[:, 3, :2] = 1.0
    means = (offset + scale * u).reshape(I * V, 3)
    fv = torch.ones(F, I, dtype=torch.bool)
    for f in frames:
        for i in absent:
            fv[f, i] = False
    d = dict(means=means, quats=n(I * V, 4), instances_quats=n(F, I, 1, 4), smpl_quats=n(F, I, JOINTS - 1, 4), instances_trans=n(F, I, 3) * 5,
             instances_fv=fv, J_canonical=n(I, JOINTS, 3) * 0.3, A0_inv=torch.eye(4).expand(I, JOINTS, 4, 4) + n(I, JOINTS, 4, 4) * 0.2,
             parents=tuple(parents), w_m=n(I * V, 3), w_q=n(I * V, 4))
    if field:
        d.update(voxel_base=torch.softmax(n(I, JOINTS, d_, h_, w_) * 2, dim=1), voxel_corr=n(I, JOINTS, d_, h_, w_) * 0.01, offset=offset,
                 scale=scale, ratio=ratio, ratio_dim=-1, W=None)
    else:
        d.update(voxel_base=None, voxel_corr=None, W=torch.softmax(n(I, V, JOINTS) * 2, dim=-1))
    if compact:
        for k in ("quats", "voxel_base", "voxel_corr"):
            d[k] = d[k].half().float()
        d["w_m"], d["w_q"] = (torch.randint(-3, 4, s, generator=g).float() for s in ((I * V, 3), (I * V, 4)))
    if settle and fv[list(frames)].any():
        for _ in range(50):
            bad = torch.zeros(I, V, dtype=torch.bool)
            for f in frames:
                gap, real = blend_margins(d, f)
                bad |= (gap < GAP) | (real < GAP)
            if not bad.any():
                break
            assert field, "a fixed weight table cannot be settled by moving points"
            k = int(bad.sum())
            d["means"].reshape(I, V, 3)[bad] = (offset.expand(I, V, 3)[bad] + scale.expand(I, V, 3)[bad] * draw(k))
        assert not bad.any()
    return d


def run_framework(d, f, dtype=torch.float64, interpolate=False, ball=False, grad=True):
    """framework_transform on the CPU in ``dtype`` -> ({"wm", "wq"}: arrays, {input: dense gradient array}) of
    loss = sum(wm * w_m) + sum(wq * w_q)."""
    ts = {k: d[k].detach().cpu().to(dtype).clone().requires_grad_(grad) for k in INPUTS if d.get(k) is not None}
    wm, wq = framework_transform(ts["means"], None if ball else ts["quats"], ts["instances_quats"], ts["smpl_quats"], ts["instances_trans"],
                                 d["instances_fv"], f, voxel_corr=ts.get("voxel_corr"), interpolate=interpolate, ball=ball,
                                 **template_kwargs(d, dtype))
    outs = {"wm": wm.detach().numpy()}
    loss = (wm * d["w_m"].to(dtype)).sum()
    if not ball:
        outs["wq"] = wq.detach().numpy()
        loss = loss + (wq * d["w_q"].to(dtype)).sum()
    grads = {}
    if grad:
        loss.backward()
        grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for k, t in ts.items()}
    return outs, grads


def scaled_err(got, ref) -> float:
    """Worst |got - ref| of the tensor, divided by max(1, the tensor's largest |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def worst(got_outs, got_grads, ref):
    """The largest scaled error over the outputs and gradients present in ``got``."""
    o64, g64 = ref
    return max([scaled_err(v, o64[k]) for k, v in got_outs.items()] + [scaled_err(v, g64[k]) for k, v in got_grads.items()])


def measured_bound(d, f, ref=None, ball=False):
    """(bound, float32-vs-float64 figure) for inputs d at frame f; ``ref``: a float64 run_framework result to reuse."""
    ref = ref if ref is not None else run_framework(d, f, ball=ball)
    o32, g32 = run_framework(d, f, torch.float32, ball=ball)
    e32 = worst(o32, g32, ref)
    return max(4.0 * e32, 1e-6), e32


def load_golden(path):
    """tests/golden/smpl_skin.npz -> (the input dict as float32 tensors, the npz)."""
    z = np.load(path)
    d = {}
    for k in ("means", "quats", "instances_quats", "smpl_quats", "instances_trans", "J_canonical", "A0_inv", "voxel_base", "voxel_corr",
              "offset", "scale", "w_m", "w_q"):
        d[k] = torch.as_tensor(z[k].astype(np.float32))
    d.update(instances_fv=torch.as_tensor(z["instances_fv"]), parents=tuple(int(p) for p in z["parents"]), ratio=float(z["ratio"]),
             ratio_dim=int(z["ratio_dim"]), W=None)
    return d, z


# ---- a stand-in with SMPLNodes' attribute layout (models/nodes/smpl.py) ---------------------------------------------------------------
class _Ns:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class StandInNodes:
    """The attributes ``SMPLNodes.get_gaussians`` reads, and that method as framework ops (smpl.py:343-397)."""

    def __init__(self, d, device, sh_degree=1, ball=False, cur_frame=1):
        P = lambda t: torch.nn.Parameter(t.clone().to(device))
        g = torch.Generator().manual_seed(5)
        N = d["means"].shape[0]
        I = d["instances_fv"].shape[1]
        K = (sh_degree + 1) ** 2
        self._means, self._quats = P(d["means"]), P(d["quats"])
        self._scales = P(torch.randn(N, 1 if ball else 3, generator=g) * 0.3 - 3)
        self._opacities = P(torch.randn(N, 1, generator=g))
        self._features_dc, self._features_rest = P(torch.rand(N, 3, generator=g)), P(torch.randn(N, K - 1, 3, generator=g) * 0.2)
        self.instances_quats, self.smpl_qauts, self.instances_trans = P(d["instances_quats"]), P(d["smpl_quats"]), P(d["instances_trans"])
        self.instances_fv = d["instances_fv"].clone().to(device)
        self.point_ids = torch.arange(I).repeat_interleave(N // I)[:, None].to(device)
        vd = _Ns(lbs_voxel_base=d["voxel_base"].to(device), voxel_w_correction=P(d["voxel_corr"]), offset=d["offset"].to(device),
                 scale=d["scale"].to(device), ratio=torch.tensor(d["ratio"]), ratio_dim=d["ratio_dim"])
        self.template = _Ns(J_canonical=d["J_canonical"].to(device), A0_inv=d["A0_inv"].to(device), use_voxel_deformer=True, voxel_deformer=vd,
                            _template_layer=_Ns(parents=torch.tensor(d["parents"], dtype=torch.long)), W=None)
        self.cur_frame, self.in_test_set, self.step, self.sh_degree, self.ball_gaussians = cur_frame, False, 3000, sh_degree, ball
        self.ctrl_cfg = _Ns(sh_degree_interval=1000)

    def parameters(self):
        return {"_means": self._means, "_quats": self._quats, "_scales": self._scales, "_opacities": self._opacities,
                "_features_dc": self._features_dc, "_features_rest": self._features_rest, "instances_quats": self.instances_quats,
                "smpl_qauts": self.smpl_qauts, "instances_trans": self.instances_trans,
                "voxel_w_correction": self.template.voxel_deformer.voxel_w_correction}

    def get_gaussians(self, cam):
        from bilateral_driving_amd import gs_ops
        from bilateral_driving_amd.nodes import interpolates
        self.filter_mask = torch.ones_like(self._means[:, 0], dtype=torch.bool)
        mask = self.instances_fv[self.cur_frame]
        if mask.sum() == 0:
            return None
        vd = self.template.voxel_deformer
        wm, wq = framework_transform(self._means, self._quats, self.instances_quats, self.smpl_qauts, self.instances_trans, self.instances_fv,
                                     self.cur_frame, J_canonical=self.template.J_canonical, A0_inv=self.template.A0_inv,
                                     parents=[0] + [int(p) for p in self.template._template_layer.parents[1:]], voxel_base=vd.lbs_voxel_base,
                                     voxel_corr=vd.voxel_w_correction, offset=vd.offset, scale=vd.scale, ratio=float(vd.ratio),
                                     ratio_dim=vd.ratio_dim, ball=self.ball_gaussians,
                                     interpolate=interpolates(self.in_test_set, self.cur_frame, self.instances_fv.shape[0]))
        if self.ball_gaussians:
            wq = self._quats
        colors = torch.cat((self._features_dc[:, None, :], self._features_rest), dim=1)
        if self.sh_degree > 0:
            dirs = wm.detach() - cam.camtoworlds.data[..., :3, 3]
            dirs = dirs / dirs.norm(dim=-1, keepdim=True)
            rgbs = torch.clamp(gs_ops.spherical_harmonics(min(self.step // self.ctrl_cfg.sh_degree_interval, self.sh_degree), dirs, colors) + 0.5, 0.0, 1.0)
        else:
            rgbs = torch.sigmoid(colors[:, 0, :])
        op = torch.sigmoid(self._opacities) * mask[self.point_ids[..., 0]].float().unsqueeze(-1)
        sc = torch.exp(self._scales.repeat(1, 3)) if self.ball_gaussians else torch.exp(self._scales)
        gs = dict(_means=wm[self.filter_mask], _opacities=op[self.filter_mask], _rgbs=rgbs[self.filter_mask], _scales=sc[self.filter_mask],
                  _quats=(wq / wq.norm(dim=-1, keepdim=True))[self.filter_mask])
        for k, v in gs.items():
            if torch.isnan(v).any():
                raise ValueError(f"NaN detected in gaussian {k} at step {self.step}")
            if torch.isinf(v).any():
                raise ValueError(f"Inf detected in gaussian {k} at step {self.step}")
        self._gs_cache = {"_scales": sc[self.filter_mask]}
        return gs
