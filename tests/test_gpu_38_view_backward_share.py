"""-m gpu: what the one-view nodes share (fused_view._composite / _composite_backward / _project_backward), pinned on one tiny scene:
N = 2 000 on 96x64 -- neither side a multiple of the 64-px list tile, the height none of the 16-px compositing tile -- one camera,
RGB+ED, absgrad, a loss with an image term, an alpha term and a term on means2d itself, the camera pose differentiated.  Each drop-in
node against the operator chain, the fused training view against the drop-in call sequence; classic and antialiased; and a camera
that sees nothing (n_vis == 0).  Bounds and protocol: those of test_gpu_01's end-to-end test -- image 1e-4 and the loss over the
pixels whose discrete decisions (alpha cut, saturation stop) the float64 oracle calls stable; gradients 1e-3 in norm, 2e-3
element-wise over the entries above 1e-3 of the largest.  (Over ALL pixels the antialiased raw node and fused view differ from the
chain in one pixel, by 3e-4: opacity * comp from the projection kernel against the dense product, one alpha cut apart.)"""
import math

import pytest
import torch

from oracle import gs_oracle as G
from tests.util import aa_oracle, grad_errors, make_scene

pytestmark = pytest.mark.gpu
N, W, H = 2000, 96, 64


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib, harness as Hn
    _lib.lib()  # fails loudly if libbds.so is missing
    sc64 = make_scene(N, W, H, seed=21, dtype=torch.float64)
    act = {k: sc64[k] for k in ("means", "quats", "scales", "opacities", "colors")}
    unstable = {False: G.rasterization(*act.values(), sc64["viewmats"], sc64["Ks"], W, H, near_plane=0.1, render_mode="RGB+ED",
                                       return_unstable=True)[2]["unstable"][0],
                True: aa_oracle(act, sc64["viewmats"], sc64["Ks"], W, H, "RGB+ED", near_plane=0.1)[2][0]}
    sc = {k: v.float().cuda() for k, v in sc64.items()}
    g = torch.Generator().manual_seed(5)
    sh = torch.cat([(sc["colors"].cpu()[:, None] - 0.5) / 0.28209479177387814, 0.05 * torch.randn(N, 15, 3, generator=g)], 1).cuda()
    raw = dict(means=sc["means"], quats=sc["quats"], log_scales=sc["scales"].log(), opacity_logits=torch.logit(sc["opacities"]), sh=sh)
    away = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])).cuda() @ sc["viewmats"][0]      # turned round: every Gaussian behind it
    return dict(sc=sc, raw=raw, away=away, stable={aa: (~u)[..., None].cuda() for aa, u in unstable.items()}, grids=Hn.make_grids(1, device="cuda"), sky=torch.rand(H, W, 3, generator=g).cuda(),
                wt=torch.randn(H, W, 4, generator=g).cuda(), wa=torch.randn(H, W, 1, generator=g).cuda())


def _loss(s, aa, rgb, depth, alpha, means2d):
    wt, wa = s["wt"] * s["stable"][aa], s["wa"] * s["stable"][aa]
    return (rgb * wt[..., :3]).sum() + (depth * wt[..., 3:]).sum() + (alpha * wa).sum() + 1e-5 * (means2d ** 2).sum()


def _dropin(s, raw: bool, fused: bool, aa: bool, viewmat, monkeypatch):
    """rasterization() over the activated tensors or over a class's raw parameters (marshalling.install); ``fused`` False: BDS_API_FUSED=0."""
    import bilateral_driving_amd.rendering as R
    from bilateral_driving_amd import harness as Hn, marshalling as Marsh
    monkeypatch.setattr(R, "_ONE_VIEW_NODE", fused)
    model = Hn.VanillaModel(s["raw"])
    vm = viewmat.clone().requires_grad_(True)
    cam = Hn.Camera(viewmat, s["sc"]["Ks"][0], W, H, torch.linalg.inv(viewmat)[:3, 3].contiguous())
    if raw:
        Marsh.install(Hn.VanillaModel)
    try:
        gs = model.get_gaussians(Hn.reference_camera(cam))
        r, a, meta = R.rasterization(gs["_means"], gs["_quats"], gs["_scales"], gs["_opacities"].squeeze(), gs["_rgbs"], vm[None], cam.K[None], W, H,
                                     packed=False, absgrad=True, near_plane=0.1, render_mode="RGB+ED",
                                     rasterize_mode="antialiased" if aa else "classic")
        m2 = meta["means2d"]
        m2.retain_grad()
        _loss(s, aa, r[0, ..., :3], r[0, ..., 3:4], a[0], m2).backward()
    finally:
        if raw:
            Marsh.uninstall(Hn.VanillaModel)
    names = ("means", "quats", "log_scales", "logits", "dc", "rest")
    return (dict(rgb=r[0, ..., :3].detach(), depth=r[0, ..., 3:4].detach(), alpha=a[0].detach(), radii=meta["radii"]),
            dict({k: t.grad for k, t in zip(names, model.parameters())}, viewmat=vm.grad, means2d_grad=m2.grad, means2d_absgrad=m2.absgrad))


def _harness(s, fused: bool, aa: bool, viewmat, monkeypatch):
    """harness.render_view (the fused training view) or render_view_api (the drop-in call sequence over the activated node)."""
    import bilateral_driving_amd.rendering as R
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.fused_view import fused_view
    p = {k: v.clone().requires_grad_(True) for k, v in s["raw"].items()}
    grids = [g.clone().requires_grad_(True) for g in s["grids"]]
    cam = Hn.Camera(viewmat.clone().requires_grad_(True), s["sc"]["Ks"][0], W, H, torch.linalg.inv(viewmat)[:3, 3].contiguous())
    if fused and aa:       # (render_view with the one argument it does not pass on)
        out = fused_view(p, cam.viewmat, cam.K, W, H, grids, s["sky"], Hn.FACTORS_3, cam_pos=cam.cam_pos, img_idx=0, antialiased=True)
    elif fused:
        out = Hn.render_view(p, cam, grids, 0, s["sky"])
    else:
        if aa:
            plain = R.rasterization
            monkeypatch.setattr(R, "rasterization", lambda *a, **k: plain(*a, **dict(k, rasterize_mode="antialiased")))
        out = Hn.render_view_api(p, cam, grids, 0, s["sky"])
    m2 = out["info"]["means2d"]
    m2.retain_grad()
    _loss(s, aa, out["rgb"], out["depth"], out["opacity"], m2).backward()
    return (dict(rgb=out["rgb"].detach(), depth=out["depth"].detach(), alpha=out["opacity"].detach(), radii=out["info"]["radii"]),
            dict({k: t.grad for k, t in p.items()}, viewmat=cam.viewmat.grad, means2d_grad=m2.grad, means2d_absgrad=m2.absgrad,
                 **{f"grid{i}": g.grad for i, g in enumerate(grids)}))


_PATHS = {"activated_node": lambda *a: _dropin(a[0], False, *a[1:]), "raw_node": lambda *a: _dropin(a[0], True, *a[1:]), "fused_view": _harness}


@pytest.mark.parametrize("aa", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("path", list(_PATHS))
def test_shared_backward_equals_operator_chain(scene, path, aa, monkeypatch):
    vm = scene["sc"]["viewmats"][0]
    (img_ref, g_ref), (img, g) = (_PATHS[path](scene, fused, aa, vm, monkeypatch) for fused in (False, True))
    stable = scene["stable"][aa]
    assert float(stable.float().mean()) > 0.995
    assert torch.equal(img.pop("radii"), img_ref.pop("radii"))
    img_err = {k: ((img[k] - ref).abs() / ref.abs().clamp(min=1.0)) * stable for k, ref in img_ref.items()}
    g_err = {k: grad_errors(g[k], ref)[:2] for k, ref in g_ref.items()}
    print(path, aa, {k: (float(e.max()), int((e >= 1e-4).sum())) for k, e in img_err.items()}, g_err)     # (worst, values over the bound)
    for k, e in img_err.items():
        assert float(e.max()) < 1e-4, (k, float(e.max()))
    assert float(img_ref["alpha"].mean()) > 0.3
    for k, (rel, elem) in g_err.items():
        assert float(g_ref[k].abs().max()) > 0, k
        assert rel < 1e-3 and elem < 2e-3, (k, rel, elem)


@pytest.mark.parametrize("path", list(_PATHS))
def test_camera_that_sees_nothing(scene, path, monkeypatch):
    """n_vis == 0: every launch returns OK over the one record row both helpers keep, images and gradients are zeros."""
    img, g = _PATHS[path](scene, True, False, scene["away"], monkeypatch)
    assert img["radii"].numel() == N and int((img["radii"] > 0).sum()) == 0      # n_vis == 0: the camera sees no Gaussian at all
    assert float(img["alpha"].abs().max()) == 0.0 and float(img["depth"].abs().max()) == 0.0
    if path != "fused_view":       # (the training view's rgb is the transformed sky)
        assert float(img["rgb"].abs().max()) == 0.0
    for k, v in g.items():
        if not k.startswith("grid"):
            assert v is not None and math.isfinite(float(v.sum())) and float(v.abs().max()) == 0.0, k
