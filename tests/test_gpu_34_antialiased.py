"""-m gpu: rasterize_mode "antialiased" (render.antialiased, trainers/base.py:406 / :824) on every render path: the general operator
chain, the one-view node over activated parameters, the fused / captured views and the evaluation re-renders.

The oracle is built here from the oracle's own stages, per camera, in float64: project(calc_compensations=True), opacities * comp,
isect_tiles / isect_offset_encode / rasterize_to_pixels, then the ED normalisation.  Bounds are test_gpu_01's: images 1e-4; gradients
1e-3 in norm and 2e-3 per element outright.  An element above 2e-3 must belong to a Gaussian whose comp is near 0 (< NEAR0 in some
camera) and stay within 2x of the same oracle run in float32, with the float32 oracle's radii equal to the float64 ones (the project's
rule for what float32 itself cannot resolve)."""
NEAR0 = 0.2
import math

import pytest
import torch

from oracle import gs_oracle as G
from tests.util import aa_oracle, grad_errors, make_scene

pytestmark = pytest.mark.gpu

PARAMS = ("means", "quats", "scales", "opacities", "colors")


@pytest.fixture(scope="module")
def R():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    import bilateral_driving_amd.rendering as R
    return R


def _elem_check(k, got, ref, ref32, near0_rows, radii32_equal):
    """2e-3 per element (above 1e-3 of the largest one) outright; the 2x-float32 rule only for elements of rows with comp near 0."""
    got, ref, ref32 = got.detach().double().cpu(), ref.detach().double().cpu(), ref32.detach().double().cpu()
    big = ref.abs() > 1e-3 * ref.abs().max()
    e = (got - ref).abs() / ref.abs().clamp(min=1e-300)
    e32 = (ref32 - ref).abs() / ref.abs().clamp(min=1e-300)
    over = big & (e > 2e-3)
    if not bool(over.any()):
        return
    assert k != "viewmats" and radii32_equal, (k, float(e[over].max()))
    rows = over.reshape(over.shape[0], -1).any(-1)
    assert not bool((rows & ~near0_rows).any()), (k, "rows with comp >= NEAR0 above 2e-3", float(e[over].max()))
    assert bool((e[over] <= 2.0 * e32[over]).all()), (k, float(e[over].max()))


def _check(got_r, got_a, got_grads, sc, W, H, mode, backgrounds=None, sh_degree=None, seed=0, vm_grad=None):
    """oracle forward + backward of a random loss over the stable pixels in float64 and float32, then the bounds of the module doc."""
    ref, ref32 = {}, {}
    out = {}
    for dt, store in ((torch.float64, ref), (torch.float32, ref32)):
        p = {k: sc[k].to(dt).clone().requires_grad_(True) for k in PARAMS}
        vm = sc["viewmats"].to(dt).clone().requires_grad_(vm_grad is not None)
        probes = [] if dt == torch.float64 else None
        r, a, un, radii, comp = aa_oracle(p, vm, sc["Ks"].to(dt), W, H, mode, None if backgrounds is None else backgrounds.to(dt), sh_degree,
                                          probes=probes)
        if dt == torch.float64:
            stable = ~un
            g = torch.Generator().manual_seed(seed)
            out.update(r=r.detach(), a=a.detach(), stable=stable, wt=torch.randn(r.shape, generator=g) * stable[..., None],
                       wa=torch.randn(a.shape, generator=g) * stable[..., None], probes=probes, radii=radii, comp=comp)
        else:
            out["radii32_equal"] = bool(torch.equal(radii, out["radii"]))
        ((r * out["wt"].to(dt)).sum() + (a * out["wa"].to(dt)).sum()).backward()
        store.update({k: v.grad for k, v in p.items()})
        if vm_grad is not None:
            store["viewmats"] = vm.grad
    stable = out["stable"]
    assert stable.float().mean() > 0.98
    err = (got_r.detach().cpu().double() - out["r"]).abs() / out["r"].abs().clamp(min=1.0)
    assert float(err[stable].max()) < 1e-4, float(err[stable].max())
    assert float((got_a.detach().cpu().double() - out["a"]).abs()[stable].max()) < 1e-4
    grads = got_grads(out["wt"].cuda(), out["wa"].cuda())
    near0 = ((out["comp"] < NEAR0) & (out["radii"] > 0)).any(0)
    for k, gref in ref.items():
        if k not in grads:
            continue
        rel, _, _ = grad_errors(grads[k], gref)
        assert rel < 1e-3, (k, rel)
        _elem_check(k, grads[k], gref, ref32[k], near0, out["radii32_equal"])
    return out


def test_general_path_two_cameras_sh_backgrounds_rgbd(R):
    """C = 2, SH colours, backgrounds, RGB+D, with a viewmats gradient: the operator chain, whose backward now takes v_compensations."""
    W, H, N = 160, 112, 1500
    sc = make_scene(N, W, H, seed=21)
    g = torch.Generator().manual_seed(5)
    vm2 = sc["viewmats"][0].clone()
    vm2[:3, 3] += torch.tensor([0.15, -0.05, 0.1])
    sc["viewmats"] = torch.stack([sc["viewmats"][0], vm2])
    sc["Ks"] = sc["Ks"].expand(2, 3, 3).contiguous()
    sc["colors"] = torch.randn(N, 16, 3, generator=g) * 0.3
    bg = torch.rand(2, 3, generator=g)
    p = {k: sc[k].cuda().requires_grad_(True) for k in PARAMS}
    vm = sc["viewmats"].cuda().requires_grad_(True)
    r, a, meta = R.rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vm, sc["Ks"].cuda(), W, H, sh_degree=3,
                                 backgrounds=bg.cuda(), render_mode="RGB+D", rasterize_mode="antialiased")
    assert meta["opacities"].shape == (2, N)

    def grads(wt, wa):
        ((r * wt).sum() + (a * wa).sum()).backward()
        return dict({k: v.grad for k, v in p.items()}, viewmats=vm.grad)
    _check(r, a, grads, sc, W, H, "RGB+D", backgrounds=bg, sh_degree=3, seed=1, vm_grad=True)


@pytest.mark.parametrize("mode", ["RGB+ED", "RGB"])
def test_one_view_node(R, mode, monkeypatch):
    """C = 1, post-activation colours: the _RasterizeView node (never the operator chain: fully_fused_projection is made to raise),
    absgrad, .absgrad / retain_grad() on meta["means2d"], meta["opacities"] = opacity * comp [1,N]."""
    W, H, N = 200, 136, 2500
    sc = make_scene(N, W, H, seed=22)
    monkeypatch.setattr(R, "fully_fused_projection", lambda *a, **k: (_ for _ in ()).throw(AssertionError("general path taken")))
    p = {k: sc[k].cuda().requires_grad_(True) for k in PARAMS}
    r, a, meta = R.rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], sc["viewmats"].cuda(), sc["Ks"].cuda(),
                                 W, H, absgrad=True, render_mode=mode, rasterize_mode="antialiased")
    meta["means2d"].retain_grad()
    _, _, _, _, comp = G.project(sc["means"].double(), sc["quats"].double(), sc["scales"].double(), sc["viewmats"][0].double(),
                                 sc["Ks"][0].double(), W, H, calc_compensations=True)
    assert meta["opacities"].shape == (1, N)
    assert float((meta["opacities"][0].cpu().double() - sc["opacities"].double() * comp).abs().max()) < 1e-5

    def grads(wt, wa):
        ((r * wt).sum() + (a * wa).sum()).backward()
        return {k: v.grad for k, v in p.items()}
    _check(r, a, grads, sc, W, H, mode, seed=2)
    m2 = meta["means2d"]
    assert m2.absgrad.shape == (1, N, 2) and m2.grad is not None and m2.grad.shape == (1, N, 2)
    assert float(m2.absgrad.abs().max()) > 0


def test_one_view_absgrad_value(R):
    W, H, N = 128, 96, 1200
    sc = make_scene(N, W, H, seed=23)
    p = {k: sc[k].cuda().requires_grad_(True) for k in PARAMS}
    r, a, meta = R.rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], sc["viewmats"].cuda(), sc["Ks"].cuda(),
                                 W, H, absgrad=True, render_mode="RGB+ED", rasterize_mode="antialiased")
    box = {}

    def grads(wt, wa):
        ((r * wt).sum() + (a * wa).sum()).backward()
        box["ag"] = meta["means2d"].absgrad[0]
        return {k: v.grad for k, v in p.items()}
    out = _check(r, a, grads, sc, W, H, "RGB+ED", seed=3)
    ag_ref = G.absgrad_from_probe(out["probes"][0], N)
    assert float((box["ag"].cpu().double() - ag_ref).norm() / ag_ref.norm()) < 1e-3


def _fused_inputs(N, W, H, seed):
    from bilateral_driving_amd import harness as Hn
    cams = Hn.ring_cameras(W, H, yaws_deg=(0.0,), device="cuda")
    p = Hn.synthetic_scene(N, seed=seed, device="cuda")
    p["means"] = p["means"] * torch.tensor([0.3, 0.3, 1.0], device="cuda")
    return Hn, cams[0], p


def test_fused_view_against_the_one_view_node(R):
    """fused_view(antialiased=True): expected depth and alpha -- and their gradients into the RAW parameters (the raw list backward)
    -- against rasterization(rasterize_mode="antialiased") over the activated parameters (the one-view node, oracle-checked above)."""
    from bilateral_driving_amd import fused_view as FV
    W, H, N = 192, 128, 3000
    Hn, cam, p = _fused_inputs(N, W, H, 31)
    grids = Hn.make_grids(1, device="cuda")
    sky = torch.rand(H, W, 3, device="cuda")
    raw = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = FV.fused_view(raw, cam.viewmat, cam.K, W, H, grids, sky, Hn.FACTORS_3, cam_pos=cam.cam_pos, antialiased=True)
    ref_in = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    dep = torch.zeros(N, 3, device="cuda")
    r, a, _ = R.rasterization(ref_in["means"], ref_in["quats"], torch.exp(ref_in["log_scales"]), torch.sigmoid(ref_in["opacity_logits"]), dep,
                              cam.viewmat[None], cam.K[None], W, H, near_plane=0.1, render_mode="RGB+ED", rasterize_mode="antialiased")
    assert float((out["depth"] - r[0, ..., 3:]).abs().max() / r[0, ..., 3:].abs().max()) < 1e-4
    assert float((out["opacity"] - a[0]).abs().max()) < 1e-4
    assert float(a.mean()) > 0.2
    g = torch.Generator().manual_seed(4)
    wd, wa = torch.randn(H, W, 1, generator=g).cuda(), torch.randn(H, W, 1, generator=g).cuda()
    ((out["depth"] * wd).sum() + (out["opacity"] * wa).sum()).backward()
    ((r[0, ..., 3:] * wd).sum() + (a[0] * wa).sum()).backward()
    for k in ("means", "quats", "log_scales", "opacity_logits"):
        got, ref = raw[k].grad, ref_in[k].grad
        assert float((got - ref).norm() / ref.norm()) < 1e-3, (k, float((got - ref).norm() / ref.norm()))
    # classic differs: the mode really reaches the kernels
    cl = FV.fused_view({k: v.detach() for k, v in p.items()}, cam.viewmat, cam.K, W, H, grids, sky, Hn.FACTORS_3, cam_pos=cam.cam_pos)
    assert not torch.equal(cl["opacity"], out["opacity"].detach())


def test_frame_graph_equals_eager_frame(R):
    """FrameGraph(antialiased=True) == the eager antialiased frame (test_gpu_09 for classic): images bit-equal; gradients of the five
    per-Gaussian parameters, the grids, the skies and the camera poses, and every view's absgrad, to test_gpu_09's bounds (float atomics
    in the compositor backward: the order of the sums varies)."""
    from bilateral_driving_amd import fused_view as FV
    from bilateral_driving_amd import graph_view as GV
    from bilateral_driving_amd import harness as Hn
    from tests.util import rel_err
    W, H, N = 256, 160, 5000
    cams = Hn.ring_cameras(W, H, yaws_deg=(0.0, 120.0), device="cuda")
    for c in cams:
        c.viewmat.requires_grad_(True)
    p = Hn.synthetic_scene(N, seed=3, device="cuda")
    p["means"] = p["means"] * torch.tensor([0.4, 0.4, 1.0], device="cuda")
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(len(cams), device="cuda")]
    gen = torch.Generator().manual_seed(14)
    skies = [torch.rand(H, W, 3, generator=gen).cuda().requires_grad_(True) for _ in cams]
    targets = [torch.rand(H, W, 3, generator=gen).cuda() for _ in cams]
    old = FV.SH_IN_PACK
    FV.SH_IN_PACK = FV.SH_IN_PACK_DEV          # (the same SH arithmetic in both forms: see test_gpu_09)
    try:
        eager = []
        for v, cam in enumerate(cams):
            out = FV.fused_view(p, cam.viewmat, cam.K, W, H, grids, skies[v], Hn.FACTORS_3, cam_pos=cam.cam_pos, tile_cull=Hn.TILE_CULL,
                                img_idx=v, antialiased=True)
            loss = Hn.training_loss(out, targets[v], grids)
            loss.backward()
            eager.append((out["rgb"].detach().clone(), out["depth"].detach().clone(), float(loss), out["info"]["means2d"].absgrad[0].clone()))
        g_ref = {k: t.grad.clone() for k, t in p.items()}
        g_ref.update({f"grid{i}": g.grad.clone() for i, g in enumerate(grids)})
        sky_ref, vm_ref = [s.grad.clone() for s in skies], [c.viewmat.grad.clone() for c in cams]
        classic = FV.fused_view({k: t.detach() for k, t in p.items()}, cams[0].viewmat.detach(), cams[0].K, W, H, [g.detach() for g in grids],
                                skies[0].detach(), Hn.FACTORS_3, cam_pos=cams[0].cam_pos, img_idx=0)
        assert not torch.equal(classic["rgb"], eager[0][0])
        frame = GV.FrameGraph(p, cams, grids, skies, targets, antialiased=True)
        for rep in range(2):
            assert frame.step() is True
            for v, vg in enumerate(frame.views):
                assert torch.equal(vg.rgb, eager[v][0]) and torch.equal(vg.depth, eager[v][1]), (rep, v)
                assert abs(float(vg.loss) - eager[v][2]) < 1e-6 * max(1.0, abs(eager[v][2]))
                assert rel_err(vg.v_sky, sky_ref[v]) < 1e-6 and rel_err(vg.v_viewmat, vm_ref[v]) < 1e-4, (rep, v)
                assert rel_err(frame.g2d[v][1], eager[v][3]) < 2e-4, (rep, v)
            for k, t in p.items():
                assert rel_err(t.grad, g_ref[k]) < 2e-4, (rep, k)
            for i, g in enumerate(grids):
                assert rel_err(g.grad, g_ref[f"grid{i}"]) < 3e-5, (rep, i)
    finally:
        FV.SH_IN_PACK = old


def test_raw_node_through_marshalling(R):
    """The reference's own call sequence (models/trainers/base.py:385-419 with render.antialiased) over marshalling.install's
    placeholders: the raw one-view node _RasterizeRawView runs (nothing else), and its image, alphas, the gradients of the six raw
    parameters, means2d.absgrad / .grad and meta["opacities"] (opacity * comp, [1,N]) equal the eager antialiased _RasterizeView over
    the dense activations (test_one_view_node ties that one to the oracle) -- test_gpu_23's bounds."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd import marshalling as M
    W, H, N = 320, 192, 12000
    cam = Hn.ring_cameras(W, H, yaws_deg=(20.0,), device="cuda")[0]
    p = Hn.synthetic_scene(N, seed=6, device="cuda")
    model = Hn.VanillaModel(p)
    gen = torch.Generator().manual_seed(6)
    w3, w1, wa = (torch.randn(H, W, c, generator=gen).cuda() for c in (3, 1, 1))

    def sequence():
        for t in model.parameters():
            t.grad = None
        gs = model.get_gaussians(Hn.reference_camera(cam))
        gs = {k: torch.cat([v], dim=0) for k, v in gs.items()}
        renders, alphas, info = R.rasterization(means=gs["_means"], quats=gs["_quats"], scales=gs["_scales"],
                                                opacities=gs["_opacities"].squeeze(), colors=gs["_rgbs"], viewmats=cam.viewmat[None],
                                                Ks=cam.K[None], width=W, height=H, packed=False, absgrad=True, sparse_grad=False,
                                                rasterize_mode="antialiased", near_plane=0.1, render_mode="RGB+ED")
        info["means2d"].retain_grad()
        rgb, depth = torch.split(renders[0], [3, 1], dim=-1)
        ((rgb * w3).sum() + (depth * w1).sum() + (alphas[0] * wa).sum()).backward()
        return (rgb.detach().clone(), depth.detach().clone(), alphas[0].detach().clone(), [t.grad.clone() for t in model.parameters()],
                info["means2d"].absgrad.clone(), info["means2d"].grad.clone(), info["opacities"].detach().clone())

    eager = sequence()
    seen = []
    raw_apply, one_apply = R._RasterizeRawView.apply, R._RasterizeView.apply
    M.install(Hn.VanillaModel)
    try:
        R._RasterizeRawView.apply = staticmethod(lambda *a: (seen.append("raw"), raw_apply(*a))[1])
        R._RasterizeView.apply = staticmethod(lambda *a: (seen.append("one"), one_apply(*a))[1])
        raw = sequence()
    finally:
        R._RasterizeRawView.apply, R._RasterizeView.apply = raw_apply, one_apply
        M.uninstall(Hn.VanillaModel)
    assert seen == ["raw"]
    for a, b, n in zip(raw[:3], eager[:3], ("rgb", "depth", "alphas")):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max())), n
    names = ["means", "quats", "scales", "opacities", "features_dc", "features_rest"]
    for n, a, b in zip(names, raw[3], eager[3]):
        assert a.shape == b.shape, n
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-9, (n, float((a - b).abs().max()), float(b.abs().max()))
    for a, b, n in ((raw[4], eager[4], "absgrad"), (raw[5], eager[5], "grad")):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-12, n
    assert raw[6].shape == (1, N) and eager[6].shape == (1, N)
    assert float((raw[6] - eager[6]).abs().max()) <= 2e-5     # (activations in-kernel vs dense torch ones: rounding, as the image)
    # opacity * comp: below the plain opacity wherever the splat is seen
    assert bool((raw[6][0] <= torch.sigmoid(p["opacity_logits"]) + 1e-7).all()) and float((raw[6][0] - torch.sigmoid(p["opacity_logits"])).abs().max()) > 1e-2


def test_render_classes(R):
    """render_classes(antialiased=True): each mask multiplies the effective opacity -- against rasterization(opacities * mask,
    rasterize_mode="antialiased")."""
    from bilateral_driving_amd import fused_view as FV
    W, H, N = 160, 120, 2500
    Hn, cam, p = _fused_inputs(N, W, H, 32)
    gen = torch.Generator().manual_seed(6)
    masks = {"half": (torch.rand(N, generator=gen) < 0.5).cuda(), "all": torch.ones(N, dtype=torch.bool, device="cuda")}
    out = FV.render_classes(p, cam.viewmat, cam.K, W, H, masks, cam_pos=cam.cam_pos, antialiased=True)
    scales, opac = torch.exp(p["log_scales"]), torch.sigmoid(p["opacity_logits"])
    from bilateral_driving_amd.gs_ops import spherical_harmonics
    col = torch.clamp(spherical_harmonics(3, p["means"] - cam.cam_pos, p["sh"]) + 0.5, 0.0, 1.0)     # (test_gpu_07's recipe)
    quats = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
    for name, m in masks.items():
        r, a, _ = R.rasterization(p["means"], quats, scales, opac * m.float(), col, cam.viewmat[None], cam.K[None], W, H, near_plane=0.1,
                                  render_mode="RGB+ED", rasterize_mode="antialiased")
        # (the general form evaluates activations / SH in separate kernels: rounding-level differences, test_gpu_07's tolerances)
        torch.testing.assert_close(out[name + "_opacity"], a[0], rtol=1e-4, atol=1e-5, msg=name)
        torch.testing.assert_close(out[name + "_rgb"], r[0, ..., :3].clamp(max=1.0), rtol=1e-4, atol=1e-5, msg=name)
    assert torch.equal(out["all_rgb"], out["rgb_gaussians"])


@pytest.mark.parametrize("case", range(40))
def test_random_sweep(R, case):
    """Random scenes with test_gpu_25's edge populations (needles, sub-pixel splats, splats at the FOV clamp and behind the near plane)
    through the one-view node and (every third case) the two-camera operator chain."""
    g = torch.Generator().manual_seed(700 + case)
    W, H = int(torch.randint(48, 200, (1,), generator=g)), int(torch.randint(40, 150, (1,), generator=g))
    N = int(torch.randint(200, 1500, (1,), generator=g))
    sc = make_scene(N, W, H, seed=800 + case, spread=1.3)
    k = N // 5
    sc["scales"][:k, 1:] *= 0.05                       # needles
    sc["scales"][k:2 * k] *= 0.02                      # sub-pixel splats
    sc["means"][2 * k:2 * k + k // 4, 2] = -sc["means"][2 * k:2 * k + k // 4, 2]   # behind the camera
    mode = ("RGB", "RGB+ED", "RGB+D")[case % 3]
    two = case % 3 == 2
    if two:
        vm2 = sc["viewmats"][0].clone()
        vm2[:3, 3] += torch.tensor([0.1, 0.05, -0.1])
        sc["viewmats"] = torch.stack([sc["viewmats"][0], vm2])
        sc["Ks"] = sc["Ks"].expand(2, 3, 3).contiguous()
    p = {kk: sc[kk].cuda().requires_grad_(True) for kk in PARAMS}
    r, a, _ = R.rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], sc["viewmats"].cuda(), sc["Ks"].cuda(), W, H,
                              render_mode=mode, rasterize_mode="antialiased")

    def grads(wt, wa):
        ((r * wt).sum() + (a * wa).sum()).backward()
        return {kk: v.grad for kk, v in p.items()}
    _check(r, a, grads, sc, W, H, mode, seed=case)
