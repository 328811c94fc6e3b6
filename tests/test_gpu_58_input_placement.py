"""-m gpu: the public entries at the pointer alignments contiguous views hand them.  Almost every other test builds its inputs with
``torch.rand(...).cuda()`` or ``.clone()``: fresh allocations, 512-byte aligned.  A row slice ``t[k:]`` of an [N,3] tensor, the gradient
autograd hands a node behind a ``torch.cat`` and a view into a flat buffer are contiguous at 4-byte alignment only, and the library
has host-side decisions (``aligned16``: 16-byte loads or float by float), entries that answer BDS_EINVAL for a misaligned array and
8- / 16-byte loads issued at whatever phase the pointer has.  tests/placement.py puts inputs and incoming gradients at a chosen phase.

Every case runs its entry (1) with every tensor input in a fresh allocation, (2) with every tensor input placed, the offsets cycled
over the inputs so that neighbours differ and rotated so that every input sees every offset, (3) with one input at a time placed, for
the inputs a host-side decision names.  Every placement is held to
  (a) the op's float64 reference at the bound of the op's existing test (named per test; no bound is new);
  (b) bit-equality with run (1) where the op's existing tests assert determinism or bit-equality;
  (c) the wrapper accepting the input: no BdsError, no assertion on alignment;
and every case asserts the phase it meant to produce (``placed`` does).  The sizes: a handful of rows, and one workgroup piece of the
kernel plus a ragged rest.

What reads each placed input, with what load, and what happens at 4-byte alignment (read from the code before anything ran):
  SH dirs, masks, v_out                        sh.hip                     scalar                     same form
  SH coeffs                                    sh.hip                     float4 / scalar            the host picks scalar (:477, :503)
  projection inputs and gradients              project.hip                scalar                     same form
  isect means2d, radii, depths, conics, opac.  tiles.hip                  scalar                     same form
  rasterize_to_pixels means2d                  splat_pack_kernel          float2                     the wrapper copies (rasterize.hip:1007)
  conics, colors, opacities, bg, v_render, ..  rasterize.hip              scalar                     same form
  raw node quats                               nonfinite_flags kind 2     16-byte, aligned(4)        plain global load, issued unaligned
  raw node dc / rest                           splat_pack_sh_kernel       scalar / 16-byte aligned(4) plain global load; the LDS rows keep their own phase
  fused view sh                                sh_view_fwd / pack         float4 / scalar            host and Python pick scalar (sh.hip:548, fused_view.py:273)
  L1 rgb, target                               loss.hip, bilagrid.hip     float4                     the wrapper copies
  train_view target                            bilagrid_ms.h              scalar (16-byte required)  Python takes the one-launch loss (fused_view.py:1004)
  ssim maps                                    loss.hip                   scalar                     same form
  pixel_loss, reg_losses, image_terms maps     image_loss_math.h          scalar                     same form (one kernel set)
  bilagrid rgb, alpha, sky, v_out              bilagrid_ms.h              scalar                     same form
  slice xy, rgb, v_out (three forms)           bilagrid.hip               scalar                     same form
  head feats, v_aff                            mlp_head.hip               float4                     the wrapper copies
  head / image rgb, v_out                      mlp_head.hip               scalar                     same form
  Adam p, g, m, v; deferred rows               optim.hip                  float4 / scalar            the host picks scalar (:99, :325)
  node, smpl, pvg, deform data inputs          nodes / smpl / pvg / deform scalar                    same form
  cube map tex, dirs, v_out                    envlight.hip               scalar                     same form
  error maps pred, gt, dyn, maps               error_buffer.hip           float4 / scalar            the device picks scalar (:121)
  union mask                                   exchange.hip               uint4 / bytes              the device picks bytes, per piece (:26)
No placed input goes through an LDS-direct or a buffer load (tiles.hip's buffer loads read its own workspace; bilagrid_ms.h reads staged
copies)."""
import math

import numpy as np
import pytest
import torch

from oracle import bilagrid_oracle as BO
from oracle import gs_oracle as G
from oracle import loss_oracle as LO
from tests.placement import OFFSETS, cat_grad, phase, placed, regrad
from tests.util import make_scene, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()


def offs_for(t):
    return OFFSETS[t.dtype]


def fresh(t):
    return None if t is None else placed(t, 0)


def all_placed(tensors, rot):
    """Every tensor of the dict placed: input i at the (i + rot)-th offset of its dtype's list, so that neighbours differ."""
    out = {}
    for i, (k, t) in enumerate(tensors.items()):
        if t is None:
            out[k] = None
            continue
        o = offs_for(t)
        out[k] = placed(t, o[(i + rot) % len(o)])
        assert phase(out[k]) != 0
    return out


def placements(tensors, named=()):
    """[(label, {name: tensor})]: fresh; all placed, three rotations; each of ``named`` alone at every offset of its dtype."""
    runs = [("aligned", {k: fresh(t) for k, t in tensors.items()})]
    for rot in range(3):
        runs.append((f"all-rot{rot}", all_placed(tensors, rot)))
    for name in named:
        for o in offs_for(tensors[name]):
            run = {k: fresh(t) for k, t in tensors.items()}
            run[name] = placed(tensors[name], o)
            assert phase(run[name]) == (o * tensors[name].element_size()) % 16 != 0
            runs.append((f"{name}-off{o}", run))
    assert runs[0][0] == "aligned" and all(phase(t) == 0 for t in runs[0][1].values() if t is not None)
    return runs


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def leaf(t):
    """A new leaf over ``t``'s memory (same base: the placement is kept)."""
    return t.detach().requires_grad_(True)


# =====================================================================================================================================
# A. the drop-in ops (gs_ops)
# =====================================================================================================================================
SH_CASES = [(K, deg) for K in (1, 4, 9, 16) for deg in range(4) if (deg + 1) ** 2 <= K]


@pytest.mark.parametrize("n", [5, 1027])
@pytest.mark.parametrize("K,deg", SH_CASES, ids=[f"K{K}-deg{d}" for K, d in SH_CASES])
def test_spherical_harmonics(K, deg, n):
    """gs_ops.spherical_harmonics against oracle/gs_oracle.py in float64 at the bounds of tests/test_gpu_01_gs_parity.py
    test_sh_fwd_bwd (1e-5 on the colours and d/d coeffs, 1e-4 on d/d dirs), with and without masks.  Named by a host-side decision:
    ``coeffs`` (csrc/sh.hip bds_sh_fwd: the 16-byte forms for rows of K * 3 % 4 == 0 floats on 16-byte boundaries, else float by
    float).  No (b): the two forward forms are two instantiations of the arithmetic (csrc/sh.hip:18, the note at :85-87)."""
    from bilateral_driving_amd import gs_ops as ops
    g = torch.Generator().manual_seed(1000 * K + 10 * deg + n)
    dirs, coeffs = torch.randn(n, 3, generator=g) * 2, torch.randn(n, K, 3, generator=g)
    masks = (torch.rand(n, generator=g) > 0.2).to(torch.uint8)
    v = torch.randn(n, 3, generator=g)
    for use_masks in (False, True):
        d_ref, c_ref = leaf(dirs.double()), leaf(coeffs.double())
        ref = G.spherical_harmonics(deg, d_ref, c_ref, masks.double() if use_masks else None)
        (ref * v.double()).sum().backward()
        src = dict(dirs=dirs.cuda(), coeffs=coeffs.cuda(), masks=masks.cuda() if use_masks else None, v=v.cuda())
        for label, p in placements(src, named=("coeffs",)):
            d_g, c_g = leaf(p["dirs"]), leaf(p["coeffs"])
            out = ops.spherical_harmonics(deg, d_g, c_g, p["masks"])
            torch.autograd.backward([out], [p["v"]])
            tag = (label, use_masks)
            assert rel_err(out.cpu(), ref.detach()) < 1e-5, tag
            assert rel_err(c_g.grad.cpu(), c_ref.grad) < 1e-5, tag
            if deg > 0:
                assert rel_err(d_g.grad.cpu(), d_ref.grad) < 1e-4, tag


W_, H_ = 96, 64


def _scene(N):
    return make_scene(N, W_, H_, seed=N, spread=1.0 if N > 100 else 0.5)


@pytest.mark.parametrize("N", [5, 1027])
def test_fully_fused_projection(N):
    """gs_ops.fully_fused_projection against oracle/gs_oracle.py ``project`` in float64 at the bounds of tests/test_gpu_01_gs_parity.py
    test_projection_fwd_bwd; the incoming gradients through ``regrad``.  (b): every output and the gradients of means / quats / scales
    bit-equal to the aligned run (one thread per Gaussian, float-by-float loads whatever the phase).  The pose gradient is summed
    over the workgroups with float atomics (csrc/project.hip:91): (a) only."""
    from bilateral_driving_amd import gs_ops as ops
    sc = _scene(N)
    ref_in = {k: leaf(sc[k].double()) for k in ("means", "quats", "scales")}
    vm = leaf(sc["viewmats"].double())
    radii_r, m2_r, d_r, c_r, _ = G.project(ref_in["means"], ref_in["quats"], ref_in["scales"], vm[0], sc["Ks"][0].double(), W_, H_)
    g = torch.Generator().manual_seed(N)
    w2, wd, wc = torch.randn(N, 2, generator=g), torch.randn(N, generator=g), torch.randn(N, 3, generator=g)
    in32 = {k: leaf(sc[k].detach().clone().float()) for k in ("means", "quats", "scales")}
    _, m2_32, d_32, c_32, _ = G.project(in32["means"], in32["quats"], in32["scales"], sc["viewmats"][0].float(), sc["Ks"][0].float(), W_, H_)
    src = {k: sc[k].cuda() for k in ("means", "quats", "scales", "viewmats", "Ks")}
    base, done_ref = None, False
    for r_i, (label, p) in enumerate(placements(src)):
        gi = {k: leaf(p[k]) for k in ("means", "quats", "scales", "viewmats")}
        radii, m2, d, c, comp = ops.fully_fused_projection(gi["means"], gi["quats"], gi["scales"], gi["viewmats"], p["Ks"], W_, H_)
        assert comp is None
        same = radii[0].cpu() == radii_r
        assert same.float().mean() >= 0.999, label
        vis = (radii_r > 0) & same
        assert int(vis.sum()) > N // 10
        assert rel_err(m2[0].cpu()[vis], m2_r[vis]) < 1e-5, label
        assert rel_err(d[0].cpu()[vis], d_r[vis]) < 1e-6, label
        assert ((c[0].cpu()[vis].double() - c_r[vis]).abs() / c_r[vis].abs().clamp(min=1e-3)).max() < 5e-4, label
        m = same.double()
        if not done_ref:
            ((m2_r * w2.double() * m[:, None]).sum() + (d_r * wd.double() * m).sum() + (c_r * wc.double() * m[:, None]).sum()).backward()
            ((m2_32 * w2 * m.float()[:, None]).sum() + (d_32 * wd * m.float()).sum() + (c_32 * wc * m.float()[:, None]).sum()).backward()
            done_ref = True
        mg = same.cuda().float()
        o = (0, 0, 0) if label == "aligned" else tuple((r_i + j) % 3 + 1 for j in range(3))
        ((regrad(m2, o[0])[0] * w2.cuda() * mg[:, None]).sum() + (regrad(d, o[1])[0] * wd.cuda() * mg).sum()
         + (regrad(c, o[2])[0] * wc.cuda() * mg[:, None]).sum()).backward()
        for k in ("means", "quats", "scales"):
            got, ref = gi[k].grad.cpu().double(), ref_in[k].grad
            e, e32 = float((got - ref).norm() / ref.norm()), float((in32[k].grad.double() - ref).norm() / ref.norm())
            assert e < max(1e-4, 2.0 * e32), (label, k, e, e32)
        got, ref = gi["viewmats"].grad.cpu().double()[0, :3], vm.grad[0, :3]
        assert float((got - ref).norm() / ref.norm()) < 1e-4, label
        res = [radii, m2, d, c] + [gi[k].grad for k in ("means", "quats", "scales")]
        if base is None:
            base = res
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (label, i)


@pytest.mark.parametrize("N", [5, 1027])
def test_isect_tiles(N):
    """gs_ops.isect_tiles on placed means2d / radii / depths (and, culling, conics / opacities): the integer contract of
    tests/test_gpu_01_gs_parity.py test_isect_bit_exact / tests/test_gpu_33 -- bit-exact against the oracle on the same projected
    values -- and every list bit-equal to the aligned run's."""
    from bilateral_driving_amd import gs_ops as ops
    sc = _scene(N)
    radii, m2, d, con, _ = ops.fully_fused_projection(sc["means"].cuda(), sc["quats"].cuda(), sc["scales"].cuda(), sc["viewmats"].cuda(),
                                                      sc["Ks"].cuda(), W_, H_)
    tw, th = (W_ + 15) // 16, (H_ + 15) // 16
    t, k, v = G.isect_tiles(m2[0].cpu(), radii[0].cpu(), d[0].cpu(), 16, tw, th)
    ref_off = torch.searchsorted((k >> 32).contiguous(), torch.arange(tw * th)).to(torch.int32).reshape(1, th, tw)
    assert k.numel() > 0
    src = dict(means2d=m2.detach(), radii=radii, depths=d.detach(), conics=con.detach(), opacities=sc["opacities"].cuda()[None].contiguous())
    base = None
    for label, p in placements(src):
        tpg, iids, fids, offs = ops.isect_tiles(p["means2d"], p["radii"], p["depths"], 16, tw, th)
        assert torch.equal(tpg.cpu()[0], t) and torch.equal(iids.cpu(), k) and torch.equal(fids.cpu().long(), v.long()), label
        assert torch.equal(offs.cpu(), ref_off), label
        culled = ops.isect_tiles(p["means2d"], p["radii"], p["depths"], 16, tw, th, conics=p["conics"], opacities=p["opacities"])
        if base is None:
            base = culled
            assert culled[2].numel() <= fids.numel()
        for a, b in zip(culled, base):
            assert same_bits(a, b), label


@pytest.mark.parametrize("N", [5, 1027])
def test_rasterize_to_pixels(N):
    """gs_ops.rasterize_to_pixels (means2d, conics, colors, opacities, backgrounds; v_render, v_alphas through ``regrad``) against
    oracle/gs_oracle.py ``rasterize_to_pixels`` in float64 on the same projected values and lists: the image at 1e-4 of max(1, |ref|)
    on the oracle's stable pixels and every gradient at 1e-3 norm-relative (tests/test_gpu_01_gs_parity.py: test_rasterization_end_to_end,
    test_backward_schedule_is_a_permutation_and_invisible).  (b): the forward compositor bit-equal to the aligned run; the backward
    sums with float atomics: (a) only.  Named: ``means2d`` -- bds_splat_pack reads a centre as one 8-byte load and refuses a base
    that is not 8-byte aligned (csrc/rasterize.hip:113,1007); the wrapper copies."""
    from bilateral_driving_amd import gs_ops as ops
    sc = _scene(N)
    with torch.no_grad():
        radii, m2, d, con, _ = ops.fully_fused_projection(sc["means"].cuda(), sc["quats"].cuda(), sc["scales"].cuda(), sc["viewmats"].cuda(),
                                                          sc["Ks"].cuda(), W_, H_)
    tw, th = (W_ + 15) // 16, (H_ + 15) // 16
    col = sc["colors"].cuda()[None].contiguous()
    op = sc["opacities"].cuda()[None].contiguous()
    bg = torch.rand(1, 3, generator=torch.Generator().manual_seed(99)).cuda()
    _, _, fids, offs = ops.isect_tiles(m2, radii, d, 16, tw, th, conics=con, opacities=op)
    assert fids.numel() > 0
    l64 = {k: leaf(v.detach().cpu().double()) for k, v in dict(m2=m2, con=con, col=col, op=op, bg=bg).items()}
    r64, a64, _, unstable = G.rasterize_to_pixels(l64["m2"][0], l64["con"][0], l64["col"][0], l64["op"][0], W_, H_, 16, offs.cpu()[0],
                                                  fids.cpu().long(), l64["bg"][0], return_unstable=True)
    stable = ~unstable
    assert stable.float().mean() > 0.99
    gen = torch.Generator().manual_seed(N)
    wt = torch.randn(r64.shape, generator=gen) * stable[..., None]
    wa = torch.randn(a64.shape, generator=gen) * stable[..., None]
    ((r64 * wt.double()).sum() + (a64 * wa.double()).sum()).backward()
    src = dict(m2=m2, con=con, col=col, op=op, bg=bg, wt=wt[None].cuda(), wa=wa[None].cuda())
    base = None
    for r_i, (label, p) in enumerate(placements(src, named=("m2",))):
        lv = {k: leaf(p[k]) for k in ("m2", "con", "col", "op", "bg")}
        r, a = ops.rasterize_to_pixels(lv["m2"], lv["con"], lv["col"], lv["op"], W_, H_, 16, offs, fids, backgrounds=lv["bg"], absgrad=True)
        err = (r[0].detach().cpu().double() - r64.detach()).abs() / r64.detach().abs().clamp(min=1.0)
        assert float(err[stable].max()) < 1e-4, (label, float(err[stable].max()))
        assert float((a[0].detach().cpu().double() - a64.detach()).abs()[stable].max()) < 1e-4, label
        if base is None:
            base = (r.detach().clone(), a.detach().clone())
        assert same_bits(r.detach(), base[0]) and same_bits(a.detach(), base[1]), label
        torch.autograd.backward([r, a], [p["wt"], p["wa"]])      # (the incoming gradients already placed)
        for kk in ("m2", "con", "col", "op", "bg"):
            ref, got = l64[kk].grad, lv[kk].grad.cpu().double()
            assert float(ref.abs().max()) > 0
            assert float((got - ref).norm() / ref.norm()) < 1e-3, (label, kk)


# =====================================================================================================================================
# B. the raw one-view node's finite check
# =====================================================================================================================================
@pytest.mark.parametrize("off", [1, 2, 3])
def test_raw_node_sees_a_zero_quaternion_behind_a_misaligned_base(off):
    """The raw one-view node with ``check_finite`` and ``_quats`` a contiguous view ``off`` floats behind a 16-byte boundary: a clean
    model renders, a zero quaternion row (0 / 0 after normalisation) raises ValueError naming ``quats`` as the reference does
    (tests/test_gpu_23_lazy_gaussians.py test_raw_node_raises_on_what_the_activations_make_nonfinite)."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd import marshalling as M
    from bilateral_driving_amd import rendering as R
    assert R._CHECK_FINITE
    cam = Hn.ring_cameras(W_, H_, yaws_deg=(20.0,), device="cuda")[0]
    p = Hn.synthetic_scene(1027, seed=5, device="cuda")
    grids = Hn.make_grids(1, device="cuda")
    sky = torch.rand(H_, W_, 3, generator=torch.Generator().manual_seed(5)).cuda()
    model = Hn.VanillaModel(p)
    model._quats = leaf(placed(model._quats, off))
    assert model._quats.is_contiguous() and phase(model._quats) == 4 * off
    seen = []
    raw_apply = R._RasterizeRawView.apply
    M.install(Hn.VanillaModel)
    try:
        R._RasterizeRawView.apply = staticmethod(lambda *a: (seen.append(phase(a[1])), raw_apply(*a))[1])
        with torch.no_grad():
            Hn.render_view_model(model, cam, grids, 0, sky)                       # clean: no raise
            assert seen == [4 * off]                                              # the node was handed the misaligned view itself
            for row in (0, 99, 1026):
                keep = model._quats[row].clone()
                model._quats[row] = 0.0
                with pytest.raises(ValueError, match="quats"):
                    Hn.render_view_model(model, cam, grids, 0, sky)
                model._quats[row] = keep
            Hn.render_view_model(model, cam, grids, 0, sky)
    finally:
        R._RasterizeRawView.apply = raw_apply
        M.uninstall(Hn.VanillaModel)


@pytest.mark.parametrize("mode", ["RGB+ED", "RGB"])
def test_one_view_node_on_activated_slices(mode):
    """rendering.rasterization for one camera (the activated one-view node) with means / quats / scales / opacities / colours as
    contiguous views at 4-byte alignment (``t[k:]`` of a longer tensor; for the [N,4] quaternions, whose rows are 16 bytes, a view
    into a flat buffer) against oracle/gs_oracle.py ``rasterization`` in float64 at the bounds of tests/test_gpu_01_gs_parity.py
    test_rasterization_end_to_end (image and alphas 1e-4 on the oracle's stable pixels, equal radii, gradients 1e-3 norm-relative).
    (b): image, alphas, means2d, radii, depths and conics bit-equal to the aligned run; the gradients are summed with float
    atomics: (a) only."""
    from bilateral_driving_amd import rendering as R
    N = 1027
    sc = _scene(N)
    names = ("means", "quats", "scales", "opacities", "colors")
    ref_in = {k: leaf(sc[k].double()) for k in names}
    r_ref, a_ref, m_ref = G.rasterization(ref_in["means"], ref_in["quats"], ref_in["scales"], ref_in["opacities"], ref_in["colors"],
                                          sc["viewmats"].double(), sc["Ks"].double(), W_, H_, render_mode=mode, return_unstable=True)
    stable = ~m_ref["unstable"][0]
    assert stable.float().mean() > 0.99
    gen = torch.Generator().manual_seed(7)
    wt = torch.randn(r_ref.shape, generator=gen) * stable[None, ..., None]
    wa = torch.randn(a_ref.shape, generator=gen) * stable[None, ..., None]
    ((r_ref * wt.double()).sum() + (a_ref * wa.double()).sum()).backward()
    src = {k: sc[k].cuda() for k in names}
    src.update(viewmats=sc["viewmats"].cuda(), Ks=sc["Ks"].cuda())
    base = None
    for r_i, (label, p) in enumerate(placements(src)):
        gi = {k: leaf(p[k]) for k in names}
        r, a, meta = R.rasterization(gi["means"], gi["quats"], gi["scales"], gi["opacities"], gi["colors"], p["viewmats"], p["Ks"], W_, H_,
                                     packed=False, absgrad=True, render_mode=mode)
        assert torch.equal(meta["radii"].cpu(), m_ref["radii"]), "pick another seed: fp32/fp64 radius decisions differ"
        rc, ac = r[0].detach().cpu().double(), a[0].detach().cpu().double()
        err = (rc - r_ref[0].detach()).abs() / r_ref[0].detach().abs().clamp(min=1.0)
        assert float(err[stable].max()) < 1e-4, (label, float(err[stable].max()))
        assert float((ac - a_ref[0].detach()).abs()[stable].max()) < 1e-4, label
        o = (0, 0) if label == "aligned" else ((r_i % 3) + 1, ((r_i + 1) % 3) + 1)
        ((regrad(r, o[0]) * wt.cuda()).sum() + (regrad(a, o[1]) * wa.cuda()).sum()).backward()
        for k in names:
            ref, got = ref_in[k].grad, gi[k].grad.cpu().double()
            assert float((got - ref).norm() / ref.norm()) < 1e-3, (label, k)
        res = [r.detach(), a.detach(), meta["means2d"].detach(), meta["radii"], meta["depths"].detach(), meta["conics"].detach()]
        if base is None:
            base = res
        for i, (x, y) in enumerate(zip(res, base)):
            assert same_bits(x, y), (label, i)


def test_raw_one_view_node_on_placed_parameters():
    """The reference's call sequence with ``marshalling.install`` (the raw one-view node, SH degree 3) over a class whose six raw
    parameters are contiguous views at 4-byte alignment.  (a): every run, the aligned one included, against the eager mirror of
    ``get_gaussians`` (dense activations + dense SH, the activated node: what tests/test_gpu_03 / 06 tie to the oracle) at the bounds of
    tests/test_gpu_23_lazy_gaussians.py test_installed_sequence_equals_the_eager_mirror -- equal radii, images within 2e-5 of
    max(1, largest entry), the loss within 1e-5, the six parameters' gradients within 1e-4 of their largest entry.  (b): rgb, depth,
    opacity and the radii bit-equal to the run over fresh allocations (the projection and the record pack read float by float or
    with 16-byte loads at 4-byte alignment: the same values either way; the forward compositor is deterministic); the gradients
    are summed with float atomics: (a) only."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd import marshalling as M
    from bilateral_driving_amd import rendering as R
    N = 1027
    cam = Hn.ring_cameras(W_, H_, yaws_deg=(20.0,), device="cuda")[0]
    p0 = Hn.synthetic_scene(N, seed=5, device="cuda")
    grids = [leaf(x) for x in Hn.make_grids(1, device="cuda")]
    gen = torch.Generator().manual_seed(5)
    sky, target = torch.rand(H_, W_, 3, generator=gen).cuda(), torch.rand(H_, W_, 3, generator=gen).cuda()
    attrs = ("_means", "_quats", "_scales", "_opacities", "_features_dc", "_features_rest")

    def run(model):
        for t in grids:
            t.grad = None
        out = Hn.render_view_model(model, cam, grids, 0, sky)
        loss = Hn.training_loss(out, target, grids) + 0.1 * out["depth"].mean() + 0.1 * out["opacity"].mean()
        loss.backward()
        return ([out[k].detach() for k in ("rgb", "depth", "opacity")] + [out["info"]["radii"]], float(loss.detach()),
                [getattr(model, k).grad for k in attrs])

    ref_img, ref_loss, ref_g = run(Hn.VanillaModel(p0, sh_degree=3))      # the eager mirror (nothing installed)
    assert int((ref_img[3] > 0).sum()) > 100
    seen = []
    raw_apply = R._RasterizeRawView.apply
    M.install(Hn.VanillaModel)
    try:
        R._RasterizeRawView.apply = staticmethod(lambda *a: (seen.append([phase(t) for t in a[:6]]), raw_apply(*a))[1])
        base = None
        for rot in (None, 0, 1, 2):
            model = Hn.VanillaModel(p0, sh_degree=3)
            want = []
            for i, k in enumerate(attrs):
                off = 0 if rot is None else (i + rot) % 3 + 1
                setattr(model, k, leaf(placed(getattr(model, k), off)))
                want.append(4 * off)
            img, loss, grads = run(model)
            assert seen[-1] == want, (seen[-1], want)      # the node was handed the placed views themselves
            assert torch.equal(img[3], ref_img[3]), rot
            for k, x, y in zip(("rgb", "depth", "opacity"), img, ref_img):
                err = float((x - y).abs().max())
                assert err <= 2e-5 * max(1.0, float(y.abs().max())), (rot, k, err)
            assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), (rot, loss, ref_loss)
            for k, x, y in zip(attrs, grads, ref_g):
                assert x.shape == y.shape and float(y.abs().max()) > 0, k
                assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-9, (rot, k, float((x - y).abs().max()), float(y.abs().max()))
            if base is None:
                base = img
            for i, (x, y) in enumerate(zip(img, base)):
                assert same_bits(x, y), (rot, i)
    finally:
        R._RasterizeRawView.apply = raw_apply
        M.uninstall(Hn.VanillaModel)


# =====================================================================================================================================
# C. losses
# =====================================================================================================================================
IMG_SIZES = [(13, 21), (37, 53)]


@pytest.mark.parametrize("H,W", IMG_SIZES)
def test_photometric_tv(H, W):
    """losses.photometric_tv_loss (the node) and photometric_tv_train (one launch) with rgb / target placed -- a cropped image ``img[1:]``
    of a width that is no multiple of 4 floats -- against mean|rgb - target| + sum_l w_l TV(grid_l) in float64 (TV:
    oracle/bilagrid_oracle.py) at the bounds of tests/test_gpu_00_bilagrid_parity.py for this loss: the value 1e-6 relative (2e-6 for the
    one-launch form), d/d rgb rtol 1e-6, the grids' gradients rtol 1e-5 / atol 1e-9 (the one-launch form's, added to what the
    accumulators held: rtol 1e-4 / atol 5e-7), sign(0) = 0 at an exact tie, and d/d rgb bit-equal between the two forms and to the
    aligned run.  The grids and their gradients stay aligned.  Named: ``rgb``, ``target`` (bds_l1_mean_fwd and bds_l1_tv_train require
    16-byte aligned arrays: the wrapper copies)."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.losses import photometric_tv_loss, photometric_tv_train
    g = torch.Generator().manual_seed(11 + H)
    rgb0, target0 = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g)
    target0[0, 0] = rgb0[0, 0]
    for n_grids in (0, 2):
        grids0 = Hn.make_grids(3, seed=3)[:n_grids]
        wts = [0.01 * 0.5 * math.sqrt(x.shape[4] * x.shape[3] * x.shape[2]) for x in grids0]
        pre0 = [torch.randn(x.shape, generator=g) for x in grids0]
        r64, g64 = leaf(rgb0.double()), [leaf(x.double()) for x in grids0]
        loss64 = (r64 - target0.double()).abs().mean()
        for x, w in zip(g64, wts):
            loss64 = loss64 + w * BO.total_variation_loss(x)
        (1.7 * loss64).backward()
        base = None
        for label, p in placements(dict(rgb=rgb0.cuda(), target=target0.cuda()), named=("rgb", "target")):
            tag = (label, n_grids)
            rgb, grids = leaf(p["rgb"]), [leaf(x.cuda()) for x in grids0]
            loss = photometric_tv_loss(rgb, p["target"], grids, wts)
            (1.7 * loss).backward()
            assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-6 * abs(float(loss64.detach())), tag
            assert phase(rgb.grad) == 0 and rgb.grad.shape == rgb.shape
            assert torch.allclose(rgb.grad.cpu().double(), r64.grad, rtol=1e-6, atol=0), tag
            assert float(rgb.grad[0, 0].abs().max()) == 0.0, tag
            for x, x64 in zip(grids, g64):
                assert torch.allclose(x.grad.cpu().double(), x64.grad, rtol=1e-5, atol=1e-9), tag
            # the one-launch form, upstream gradient 1
            acc = [a.cuda() for a in pre0]
            got, v_rgb = photometric_tv_train(p["rgb"], p["target"], [x.detach() for x in grids], wts, acc)
            assert abs(float(got) - float(loss64.detach())) <= 2e-6 * abs(float(loss64.detach())), tag
            assert torch.allclose(v_rgb.cpu().double(), r64.grad / 1.7, rtol=1e-6, atol=0) and float(v_rgb[0, 0].abs().max()) == 0.0, tag
            for a, b, x64 in zip(acc, pre0, g64):
                assert torch.allclose((a - b.cuda()).cpu().double(), x64.grad / 1.7, rtol=1e-4, atol=5e-7), tag
            if base is None:
                base = (rgb.grad.clone(), v_rgb.clone())
            assert same_bits(rgb.grad, base[0]) and same_bits(v_rgb, base[1]), tag


@pytest.mark.parametrize("H,W", IMG_SIZES)
def test_ssim(H, W):
    """losses.ssim / ssim_loss with pred / target placed against oracle/loss_oracle.py ``ssim`` in float64 at the bounds of
    tests/test_gpu_29_losses_random_sweep.py test_ssim_random_size (2e-5 on the value, 1e-4 of the largest entry on d/d pred).  Float
    by float loads: no host-side decision."""
    from bilateral_driving_amd.losses import ssim, ssim_loss
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + 0.15 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    p_ref = leaf(pred.clone().double())
    s_ref = LO.ssim(gt.double(), p_ref)
    (1.7 * (1 - s_ref)).backward()
    gref = p_ref.grad.float()
    for label, p in placements(dict(pred=pred.cuda(), gt=gt.cuda())):
        pp = leaf(p["pred"])
        s = ssim(pp, p["gt"])
        (1.7 * ssim_loss(pp, p["gt"])).backward()
        assert abs(float(s.detach()) - float(s_ref.detach())) < 2e-5, (label, float(s.detach()), float(s_ref.detach()))
        assert float((pp.grad.cpu() - gref).abs().max()) <= 1e-4 * float(gref.abs().max()) + 1e-9, label
        with torch.no_grad():
            assert abs(float(ssim(p["pred"], p["gt"])) - float(s)) < 1e-6, label


@pytest.mark.parametrize("depth_loss_type,with_ego", [("l1", True), ("l2", False)])
def test_pixel_loss(depth_loss_type, with_ego):
    """losses.pixel_loss with every map placed against oracle/loss_oracle.py ``pixel_loss`` in float64 (pinned to the reference's own
    models/losses.py by the goldens of tests/test_oracle_losses.py) at the bound of tests/test_gpu_00_bilagrid_parity.py
    test_pixel_loss_matches_reference_goldens: 3e-6 of max(1, |term|) on the three terms, 3e-6 of the largest entry on the gradients."""
    from bilateral_driving_amd.losses import pixel_loss
    H, W = 37, 53
    g = torch.Generator().manual_seed(29 + with_ego)
    r = lambda *s: torch.rand(*s, generator=g)
    t = dict(rgb=r(H, W, 3), opacity=r(H, W, 1) * 0.98 + 0.01, depth=r(H, W, 1) * 30 + 0.2, pixels=r(H, W, 3),
             sky=(r(H, W) > 0.7).float(), lidar=torch.where(r(H, W) > 0.6, r(H, W) * 60, torch.zeros(H, W)),
             ego=(r(H, W) > 0.85).float() if with_ego else None)
    w = (0.8, 0.05, 0.01)
    d = lambda k: None if t[k] is None else t[k].double()
    ref = LO.pixel_loss(d("rgb"), d("pixels"), d("opacity"), d("sky"), d("depth"), d("lidar"), d("ego"), w=w, depth_l2=depth_loss_type == "l2")
    for label, p in placements({k: (None if v is None else v.cuda()) for k, v in t.items()}):
        rgb, opacity, depth = leaf(p["rgb"]), leaf(p["opacity"]), leaf(p["depth"])
        terms = pixel_loss(rgb, opacity, depth, p["pixels"], p["sky"], p["lidar"], p["ego"], w[0], w[1], w[2], depth_loss_type)
        terms.sum().backward()
        for i, k in enumerate(("rgb_loss", "sky_loss", "depth_loss")):
            got_i = float(terms[i].detach())
            assert abs(got_i - float(ref[k])) <= 3e-6 * max(1.0, abs(float(ref[k]))), (label, k, got_i, float(ref[k]))
        for x, k in ((rgb, "v_rgb"), (opacity, "v_opacity"), (depth, "v_depth")):
            err = float((x.grad.cpu().double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-30)
            assert float(ref[k].abs().max()) > 0 and err <= 3e-6, (label, k, err)


def test_reg_losses():
    """losses.reg_losses, every term on, with every map placed against oracle/loss_oracle.py ``reg_losses`` in float64 at the bounds of
    tests/test_gpu_29_losses_random_sweep.py test_reg_losses_random_size_and_terms (terms rtol 2e-5 / atol 1e-7, gradients 2e-5
    norm-relative)."""
    from bilateral_driving_amd import losses as Ls
    H, W = 37, 53
    g = torch.Generator().manual_seed(12058)
    r = lambda *s: torch.rand(*s, generator=g)
    t = dict(pix=r(H, W, 3), rgb=r(H, W, 3) * 1.1, op=r(H, W, 1), dep=r(H, W, 1) * 30 + 0.2, dyn=r(H, W, 1), ego=(r(H, W) > 0.8).float())
    t["op"][0, 0, 0], t["op"][-1, -1, 0] = 0.0, 1.0
    w = torch.rand(3, generator=g) + 0.2
    o64 = {k: leaf(t[k].double()) for k in ("op", "dep", "rgb")}
    t_ref = LO.reg_losses(t["pix"].double(), o64["op"], o64["dep"], o64["rgb"], t["dyn"].double(), t["ego"].double())
    (t_ref * w.double()).sum().backward()
    assert all(float(o64[k].grad.abs().max()) > 0 for k in o64)
    for label, p in placements({k: v.cuda() for k, v in t.items()}):
        c = {k: leaf(p[k]) for k in ("op", "dep", "rgb")}
        tt = Ls.reg_losses(p["pix"], c["op"], c["dep"], c["rgb"], p["dyn"], p["ego"])
        (tt * w.cuda()).sum().backward()
        assert torch.allclose(tt.cpu().double(), t_ref.detach(), rtol=2e-5, atol=1e-7), (label, tt, t_ref)
        for k in ("op", "dep", "rgb"):
            ref, got = o64[k].grad, c[k].grad
            assert float((got.cpu().double() - ref).norm() / ref.norm()) < 2e-5, (label, k)


# =====================================================================================================================================
# D. colour transform
# =====================================================================================================================================
def test_bilagrid_transform():
    """bilagrid.bilagrid_transform (two levels, sky blend) with rgb / alpha / sky placed, the image gradient re-placed, and the grids
    handed over as slices ``g[1:2]`` of an [n,12,L,gy,gx] stack as modules.py does (12 floats per node: such a slice keeps its 16-byte
    phase) against oracle/bilagrid_oracle.py at the bounds of tests/test_gpu_26_bilagrid_random_sweep.py: the image within max(1e-4, 3 x
    the float32 oracle's error), every gradient within max(1e-3, 3 x the float32 oracle's) norm-relative.  The image arrays are read
    float by float; the grids' gradients are summed with atomics: (a) only."""
    import bilateral_driving_amd.bilagrid as B
    H, W, factors, levels = 37, 53, [4, 2], [(4, 4, 2), (8, 8, 4)]
    g = torch.Generator().manual_seed(9058)
    rgb = torch.rand(H, W, 3, generator=g) * 1.5 - 0.2
    alpha, sky, wt = torch.rand(H, W, generator=g), torch.rand(H, W, 3, generator=g), torch.randn(H, W, 3, generator=g)
    stacks = []
    for gx, gy, gl in levels:
        ident = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(12, 1, 1, 1).repeat(1, gl, gy, gx)
        stacks.append(ident[None] + 0.1 * torch.randn(3, 12, gl, gy, gx, generator=g))

    def oracle(dt):
        r, a, s_ = (leaf(x.to(dt)) for x in (rgb, alpha, sky))
        gs = [leaf(x.to(dt)) for x in stacks]
        out = BO.multiscale_transform([x[1] for x in gs], BO.sky_blend(r, a[..., None], s_), factors, neighbours=None)
        (out * wt.to(dt)).sum().backward()
        return out.detach(), dict(rgb=r.grad, alpha=a.grad, sky=s_.grad, **{f"grid{i}": x.grad for i, x in enumerate(gs)})

    ref, g64 = oracle(torch.float64)
    o32, g32 = oracle(torch.float32)
    nrm = lambda got, r: float((got.detach().double().cpu() - r.double()).norm() / r.double().norm().clamp(min=1e-300))
    err = lambda x: float(((x.detach().cpu().double() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    for label, p in placements(dict(rgb=rgb.cuda(), alpha=alpha.cuda(), sky=sky.cuda(), wt=wt.cuda())):
        rg, ag, sg = leaf(p["rgb"]), leaf(p["alpha"]), leaf(p["sky"])
        gg = [leaf(x.cuda()) for x in stacks]
        slices = [x[1:2] for x in gg]
        assert all(phase(x) == 0 and x.is_contiguous() for x in slices)
        out = B.bilagrid_transform(rg, slices, factors, alpha=ag, sky=sg)
        (regrad(out, phase(p["wt"]) // 4) * p["wt"]).sum().backward()
        assert err(out) < max(1e-4, 3.0 * err(o32)), (label, err(out), err(o32))
        got = dict(rgb=rg.grad, alpha=ag.grad, sky=sg.grad, **{f"grid{i}": x.grad for i, x in enumerate(gg)})
        for k, gref in g64.items():
            assert float(gref.abs().max()) > 0 and bool(torch.isfinite(got[k]).all()), k
            e, e32 = nrm(got[k], gref), nrm(g32[k], gref)
            assert e < max(1e-3, 3.0 * e32), (label, k, e, e32)
            if k.startswith("grid"):
                assert float(got[k][0].abs().max()) == 0.0 and float(got[k][2].abs().max()) == 0.0, (label, k)


def _torch_head(feats, rgb, w1, w2, w3, residual):
    A = torch.tanh(torch.tanh(feats @ w1.T) @ w2.T) @ w3.T
    M = A.reshape(-1, 3, 4)
    out = (M[..., :3] @ rgb[..., None])[..., 0] + M[..., 3]
    return (out + rgb if residual else out), A


def _rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


@pytest.mark.parametrize("F", [8, 24])
@pytest.mark.parametrize("P,residual", [(31, False), (1000, True)])
def test_mlp_head(F, P, residual):
    """mlp_head.transform_and_maps with feats / rgb placed (views into a flat buffer: rows of F = 8 or 24 floats keep a row slice on a
    16-byte boundary) and both incoming gradients re-placed by ``regrad`` (the colours' gradient is what a ``cat`` hands over,
    test_mlp_head_behind_a_real_cat) against the float64 framework expression at the bounds of tests/test_gpu_12_neural_modules.py
    test_fused_head_equals_framework_modules.  (b): outputs and every gradient bit-equal to the aligned run (no atomics anywhere,
    test_fused_head_single_outputs_and_saturation).  Named: ``feats``, ``v_aff`` (bds_mlp_head_fwd / _bwd require them 16-byte
    aligned: the wrapper copies); the weights are parameters of their own and stay fresh."""
    from bilateral_driving_amd import mlp_head
    g = torch.Generator().manual_seed(P + F)
    r = lambda *s: torch.randn(*s, generator=g)
    feats0, rgb0, w1, w2, w3 = r(P, F), torch.rand(P, 3, generator=g), r(64, F) * 0.3, r(64, 64) * 0.2, r(12, 64) * 0.2
    v_out, v_aff = r(P, 3), r(P, 12)
    ref_in = [leaf(x.double()) for x in (feats0, rgb0, w1, w2, w3)]
    r_out, r_aff = _torch_head(*ref_in, residual)
    ((r_out * v_out.double()).sum() + (r_aff * v_aff.double()).sum()).backward()
    src = dict(feats=feats0.cuda(), rgb=rgb0.cuda(), v_out=v_out.cuda(), v_aff=v_aff.cuda())
    runs = placements(src, named=("feats",))
    base = None
    for r_i, (label, p) in enumerate(runs + [(f"v_aff-off{o}", dict(runs[0][1], aff_off=o)) for o in (1, 2, 3)]):
        # the gradients' phases: those of the placed v_out / v_aff of this run (regrad re-places what autograd computed)
        o_out, o_aff = phase(p["v_out"]) // 4, p.get("aff_off", phase(p["v_aff"]) // 4)
        feats, rgb = leaf(p["feats"]), leaf(p["rgb"])
        ws = [leaf(x.cuda()) for x in (w1, w2, w3)]
        out, aff = mlp_head.transform_and_maps(feats, rgb, *ws, residual=residual)
        ((regrad(out, o_out) * p["v_out"]).sum() + (regrad(aff, o_aff) * p["v_aff"]).sum()).backward()
        assert _rel(out.double().cpu(), r_out.detach()) < 2e-6 and _rel(aff.double().cpu(), r_aff.detach()) < 2e-6, label
        torch.testing.assert_close(out.double().cpu(), r_out.detach(), rtol=1e-4, atol=2e-5)
        torch.testing.assert_close(aff.double().cpu(), r_aff.detach(), rtol=1e-4, atol=2e-5)
        got = [feats.grad, rgb.grad] + [x.grad for x in ws]
        for name, gg, rr in zip(("feats", "rgb", "w1", "w2", "w3"), got, ref_in):
            assert _rel(gg.double().cpu(), rr.grad) < (3e-5 if name.startswith("w") else 3e-6), (label, name)
        res = [out.detach(), aff.detach()] + got
        if base is None:
            base = res
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (label, i)


def test_mlp_head_behind_a_real_cat():
    """No ``regrad``: two heads' colours concatenated along dim 0, as a caller that batches two views does.  Autograd hands the second
    head ``grad.narrow(0, P0, P1)``: contiguous, P0 * 3 floats in, which for P0 = 31 is 4-byte aligned only (the [P,12] maps' rows are
    48 bytes: a ``cat`` of those never leaves a 16-byte boundary; a view into a flat buffer does).  The node accepts it and its
    gradients equal those of the same head run alone on a fresh gradient, bit for bit."""
    from bilateral_driving_amd import mlp_head
    g = torch.Generator().manual_seed(58)
    r = lambda *s: torch.randn(*s, generator=g)
    P0, P1, F = 31, 45, 24
    w = [x.cuda() for x in (r(64, F) * 0.3, r(64, 64) * 0.2, r(12, 64) * 0.2)]
    f0, f1, c0, c1 = r(P0, F).cuda(), r(P1, F).cuda(), torch.rand(P0, 3, generator=g).cuda(), torch.rand(P1, 3, generator=g).cuda()
    v = r(P0 + P1, 3).cuda()
    seen = []
    bwd = mlp_head._MlpHead.backward
    try:
        mlp_head._MlpHead.backward = staticmethod(lambda ctx, vo, va: (seen.append((vo.shape[0], vo.is_contiguous(), phase(vo))), bwd(ctx, vo, va))[1])
        a0, a1 = leaf(f0), leaf(f1)
        o0 = mlp_head.transform_and_maps(a0, c0, *w)[0]
        o1 = mlp_head.transform_and_maps(a1, c1, *w)[0]
        (cat_grad([o0, o1]) * v).sum().backward()
    finally:
        mlp_head._MlpHead.backward = bwd
    assert (P0 * 3 * 4) % 16 != 0 and (P1, True, (P0 * 3 * 4) % 16) in seen, seen      # autograd itself produced the misaligned view
    alone = leaf(f1)
    (mlp_head.transform_and_maps(alone, c1, *w)[0] * placed(v[P0:], 0)).sum().backward()
    assert same_bits(a1.grad, alone.grad)


def test_neural_image_transform():
    """mlp_head.image_transform (slice + head + application in one kernel, the "single24" module at 37 x 301) with rgb placed and the
    image gradient re-placed, against the two-step path at the bounds of tests/test_gpu_12_neural_modules.py
    test_fused_image_transform_equals_two_step_path.  (b): the image and d/d rgb bit-equal to the aligned run (written once per
    pixel; the grids' gradient is summed with atomics: the bound only).  rgb and v_out are read float by float."""
    from bilateral_driving_amd import mlp_head
    from bilateral_driving_amd.modules import NeuralBilateralAffineTransform
    H, W = 37, 301
    mod = NeuralBilateralAffineTransform("Affine", 3, 16, 16, 8, feature_dim=24, hidden_dim=64)
    g = torch.Generator().manual_seed(H + W)
    with torch.no_grad():
        for n, prm in mod.named_parameters():
            prm.copy_((torch.randn(prm.shape, generator=g) * (0.5 if "grids" in n else 0.25)).cuda())
    assert mlp_head.image_supported(H, W, [mod.bil_grids.grids[0]], 64)
    rgb0 = (torch.rand(H, W, 3, generator=g) * 1.2 - 0.1).cuda()
    v = torch.randn(H, W, 3, generator=g).cuda()
    infos = {"img_idx": 1}
    rgb = leaf(rgb0)
    A = mod(rgb, infos)[0]
    ref = (A[..., :3] @ rgb[..., None])[..., 0] + A[..., 3] + rgb
    (ref * v).sum().backward()
    want = {n: prm.grad.clone() for n, prm in mod.named_parameters()}
    want["rgb"] = rgb.grad.clone()
    base = None
    for label, p in placements(dict(rgb=rgb0, v=v)):
        for prm in mod.parameters():
            prm.grad = None
        rgb = leaf(p["rgb"])
        out = mod.transform(rgb, infos)
        (regrad(out, phase(p["v"]) // 4) * p["v"]).sum().backward()
        torch.testing.assert_close(out.detach(), ref.detach(), rtol=1e-4, atol=5e-5)
        got = {n: prm.grad for n, prm in mod.named_parameters()}
        got["rgb"] = rgb.grad
        for n in want:
            scale = float(want[n].abs().max())
            torch.testing.assert_close(got[n], want[n], rtol=0, atol=2e-4 * scale + 1e-7, msg=lambda m, n=n: f"{label} {n}: {m}")
        if base is None:
            base = (out.detach().clone(), rgb.grad.clone())
        assert same_bits(out.detach(), base[0]) and same_bits(rgb.grad, base[1]), label


# =====================================================================================================================================
# E. optimisers
# =====================================================================================================================================
ADAM_N = [1, 7, 4099, 2 * 256 * 4 + 5]      # the last: one workgroup's piece of bds_adam_step's 16-byte form (2 x 256 float4) plus 5


@pytest.mark.parametrize("n", ADAM_N)
@pytest.mark.parametrize("multi", [0, 1])
@pytest.mark.parametrize("consume", [False, True])
def test_fused_adam(n, multi, consume, monkeypatch):
    """optim.FusedAdam over a parameter, its gradient and its moments that are views into flat buffers: each of the four alone and all
    together at every offset.  Bit-equal to the aligned run (every form is the same element-wise arithmetic: tests/test_gpu_10_optim.py)
    and within 5e-6 of torch.optim.Adam (tests/test_gpu_31_adam_random_sweep.py).  BDS_ADAM_MULTI = 0 reaches
    adam_step_kernel<false, *>, which only a misaligned array selects (csrc/optim.hip:99); consuming, the gradient is cleared where
    it lies."""
    from bilateral_driving_amd import optim as O
    monkeypatch.setenv("BDS_ADAM_MULTI", str(multi))
    g = torch.Generator().manual_seed(58000 + n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10.0 ** (i - 2) for i in range(3)]
    cfg = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)

    pa = leaf(p0.clone().cuda())
    oa = torch.optim.Adam([pa], **cfg)
    for gr in grads:
        pa.grad = gr.cuda()
        oa.step()

    def run(o_p, o_g, o_m, o_v):
        p = leaf(placed(p0.cuda(), o_p))
        opt = O.FusedAdam([p], consume_grads=consume, **cfg)
        assert opt.multi_tensor == bool(multi)
        opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=placed(torch.zeros(n, device="cuda"), o_m),
                            exp_avg_sq=placed(torch.zeros(n, device="cuda"), o_v))
        for gr in grads:
            p.grad = placed(gr.cuda(), o_g)
            opt.step()
            if consume:
                assert float(p.grad.abs().max()) == 0.0
            else:
                assert torch.equal(p.grad, gr.cuda())
        st = opt.state[p]
        assert [phase(x) for x in (p, st["exp_avg"], st["exp_avg_sq"])] == [4 * o_p, 4 * o_m, 4 * o_v]      # stepped in place
        return p.detach(), st["exp_avg"], st["exp_avg_sq"]

    base = run(0, 0, 0, 0)
    sa = oa.state[pa]
    for a, b, what in ((pa, base[0], "param"), (sa["exp_avg"], base[1], "exp_avg"), (sa["exp_avg_sq"], base[2], "exp_avg_sq")):
        err = float((a.detach() - b).abs().max()) / max(float(a.detach().abs().max()), 1e-30)
        assert err < 5e-6, (what, err)
    combos = [tuple(o if i == j else 0 for i in range(4)) for j in range(4) for o in (1, 2, 3)]
    combos += [tuple((rot + i) % 3 + 1 for i in range(4)) for rot in range(3)] + [(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)]
    for c in combos:
        got = run(*c)
        for a, b, what in zip(got, base, ("param", "exp_avg", "exp_avg_sq")):
            assert same_bits(a, b), (c, what)


@pytest.mark.parametrize("K", [4, 16])
def test_deferred_row_adam(K):
    """optim.DeferredRowAdam over one [N,K,3] tensor whose storage, ``.grad`` and moments are views into flat buffers, each alone and
    all together off a 16-byte boundary: catch-ups, steps over lists (and, above ``dense_above``, over all rows), a step without a
    view, the ring table's wrap (``table_steps`` = 8) and flushes, BIT FOR BIT equal to the dense FusedAdam pass over the two
    split tensors, as tests/test_gpu_32_deferred_adam_random_sweep.py.  K * 3 is a multiple of 4 for both K: the float-by-float form of
    bds_adam_rows_advance is then reached through misalignment only (csrc/optim.hip:325)."""
    from bilateral_driving_amd.optim import DeferredRowAdam, FusedAdam
    N, steps, wd = 1027, 12, 0.01
    gen = torch.Generator().manual_seed(58000 + K)
    ri = lambda a, b: int(torch.randint(a, b + 1, (1,), generator=gen))
    sh0 = torch.randn(N, K, 3, generator=gen)
    sched = []
    for it in range(steps):
        lists = []
        for _ in range((1, 2, 0, 1)[it % 4]):
            n = (N // 5, N // 3, N)[ri(0, 2)] if it != 5 else 0
            ids = torch.randperm(N, generator=gen)[:n].sort().values.to(torch.int32)
            cap = n + ri(1, 7)
            pad = torch.full((cap,), -1, dtype=torch.int32)
            pad[:n] = ids
            lists.append((pad, n, ids.long(), cap, torch.randn(n, K, 3, generator=gen) * 0.01))
        sched.append(lists)

    def run(o_p, o_g, o_m, o_v, dense):
        if dense:
            dc, rest = leaf(sh0[:, :1].contiguous().cuda()), leaf(sh0[:, 1:].contiguous().cuda())
            opt = FusedAdam([{"params": [dc], "lr": 2.5e-3, "weight_decay": wd}, {"params": [rest], "lr": 2.5e-3 / 20, "weight_decay": wd}],
                            lr=0.0, eps=1e-15)
        else:
            sh = leaf(placed(sh0.cuda(), o_p))
            opt = DeferredRowAdam([{"params": [sh], "lr": 2.5e-3, "lr_b": 2.5e-3 / 20, "col_split": 3, "deferred_rows": True, "weight_decay": wd}],
                                  lr=0.0, eps=1e-15, table_steps=8)
            st = opt.state[sh]
            st["exp_avg"], st["exp_avg_sq"] = placed(st["exp_avg"], o_m), placed(st["exp_avg_sq"], o_v)
            sh.grad = placed(torch.zeros(N, K, 3, device="cuda"), o_g)
            assert [phase(x) for x in (sh, sh.grad, st["exp_avg"], st["exp_avg_sq"])] == [4 * o for o in (o_p, o_g, o_m, o_v)]
        for it, lists in enumerate(sched):
            dev_lists = [(pad.cuda(), torch.tensor([n], dtype=torch.int64).cuda(), rows.cuda(), cap, gr.cuda()) for pad, n, rows, cap, gr in lists]
            g = torch.zeros(N, K, 3, device="cuda")
            for ids, cnt, rows, cap, gr in dev_lists:
                if not dense:
                    opt.catchup(cap, cnt.data_ptr(), ids)
                g[rows] += gr
            for grp in opt.param_groups:
                grp["lr"] *= 0.98
                if "lr_b" in grp:
                    grp["lr_b"] *= 0.98
            if dense:
                dc.grad, rest.grad = g[:, :1].contiguous(), g[:, 1:].contiguous()
                opt.step()
            else:
                sh.grad.copy_(g)
                opt.step(lists=[(cap, cnt.data_ptr(), ids) for ids, cnt, rows, cap, gr in dev_lists])
                if it == 6:
                    opt.flush()
        if dense:
            cat = lambda a, b: torch.cat([a.detach(), b.detach()], 1)
            return (cat(dc, rest), cat(opt.state[dc]["exp_avg"], opt.state[rest]["exp_avg"]),
                    cat(opt.state[dc]["exp_avg_sq"], opt.state[rest]["exp_avg_sq"]))
        opt.flush()
        st = opt.state[sh]
        assert [phase(x) for x in (sh, sh.grad, st["exp_avg"], st["exp_avg_sq"])] == [4 * o for o in (o_p, o_g, o_m, o_v)]      # in place
        return sh.detach(), st["exp_avg"], st["exp_avg_sq"]

    want = run(0, 0, 0, 0, True)
    combos = [(0, 0, 0, 0)] + [tuple(o if i == j else 0 for i in range(4)) for j in range(4) for o in (1, 2, 3)]
    combos += [tuple((rot + i) % 3 + 1 for i in range(4)) for rot in range(3)] + [(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)]
    for c in combos:
        got = run(*c, False)
        for a, b, what in zip(got, want, ("param", "exp_avg", "exp_avg_sq")):
            assert same_bits(a, b), (c, what)


# =====================================================================================================================================
# F. class nodes
# =====================================================================================================================================
@pytest.mark.parametrize("N", [5, 1027])
def test_node_pose_transform(N):
    """nodes.pose_transform with its data inputs placed (means, quats, logits, the int64 ids, the bool presence table; the instance
    poses are parameters of their own) and its incoming gradients arriving through a real ``torch.cat`` behind another node's five
    rows -- the scene graph concatenates every class's world means and quats before rasterisation; 5 * 3 and 5 * 1 floats in front
    leave the second node's gradients of the means and opacities 4-byte aligned only, which the test asserts on what autograd hands
    over (no ``regrad``).  Against tests/node_pose_ref64.py at the bounds of tests/test_gpu_36_node_pose.py test_fused_matches_float64
    (outputs rtol / atol 1e-5, gradients 1e-5, the instance tables' 1e-4).  (b): outputs and every gradient bit-equal to the aligned
    run (include/bds.h: the instance gradients are reduced in a fixed order; test_instance_gradients_are_deterministic)."""
    from bilateral_driving_amd import nodes as Nd
    from tests.node_pose_ref64 import INPUTS, grads64, rel

    def case(n, seed):
        g = torch.Generator().manual_seed(seed * 1000 + n)
        F, I = 6, 7
        d = dict(means=(torch.rand(n, 3, generator=g) - 0.5) * 6, quats=torch.randn(n, 4, generator=g), logits=torch.randn(n, 1, generator=g),
                 instances_quats=torch.randn(F, I, 4, generator=g), instances_trans=torch.randn(F, I, 3, generator=g) * 10,
                 w_m=torch.randn(n, 3, generator=g), w_q=torch.randn(n, 4, generator=g), w_o=torch.randn(n, 1, generator=g))
        d["instances_fv"] = torch.rand(F, I, generator=g) > 0.2
        d["point_ids"] = torch.randint(0, I, (n,), generator=g)[:, None]
        return d

    f = 3
    first, d = case(5, 1), case(N, 2)
    to64 = lambda x: {k: (v if v.dtype in (torch.int64, torch.bool) else v.double()) for k, v in x.items()}
    r_outs, r_g = grads64(to64(d), f)
    cu = lambda x: {k: v.cuda() for k, v in x.items()}
    first_c = cu(first)
    data = ("means", "quats", "logits", "point_ids", "instances_fv")
    src = {k: d[k].cuda() for k in data}
    w = [torch.cat([first[k], d[k]]).cuda() for k in ("w_m", "w_q", "w_o")]
    base = None
    for label, p in placements(src):
        ts = {k: leaf(p[k]) for k in ("means", "quats", "logits")}
        ts.update({k: leaf(d[k].cuda()) for k in ("instances_quats", "instances_trans")})
        a = Nd.pose_transform(first_c["means"].requires_grad_(True), first_c["quats"], first_c["logits"], first_c["point_ids"],
                              first_c["instances_quats"], first_c["instances_trans"], first_c["instances_fv"], f)
        b = Nd.pose_transform(ts["means"], ts["quats"], ts["logits"], p["point_ids"], ts["instances_quats"], ts["instances_trans"],
                              p["instances_fv"], f)
        seen = []
        for o in b:
            o.register_hook(lambda g_, seen=seen: seen.append((phase(g_), g_.is_contiguous())))
        sum((cat_grad([x, y]) * ww).sum() for x, y, ww in zip(a, b, w)).backward()
        # what autograd itself handed the second node: contiguous views 15 / 20 / 5 floats into the cat's gradient
        assert sorted(seen) == sorted([((5 * 3 * 4) % 16, True), ((5 * 4 * 4) % 16, True), ((5 * 1 * 4) % 16, True)]), seen
        assert (5 * 3 * 4) % 16 != 0 and (5 * 1 * 4) % 16 != 0
        for o, r in zip(b, r_outs):
            np.testing.assert_allclose(o.detach().cpu().numpy(), r, rtol=1e-5, atol=1e-5, err_msg=label)
        for k in INPUTS:
            gk = ts[k].grad.cpu().numpy()
            assert gk.shape == r_g[k].shape, k
            assert rel(r_g[k], gk) < (1e-4 if k.startswith("instances") else 1e-5), (label, k, rel(r_g[k], gk))
        res = [o.detach() for o in b] + [ts[k].grad for k in INPUTS]
        if base is None:
            base = res
        for i, (x, y) in enumerate(zip(res, base)):
            assert same_bits(x, y), (label, i)


@pytest.mark.parametrize("N", [5, 1027])
def test_deform_network(N):
    """deform.ConditionalDeformNetwork (quaternion and scale heads on) with x / t / cond placed (the network's weights are parameters of
    their own) and the heads' gradients arriving through a real ``torch.cat`` behind five rows of another call: 15 floats in front of
    d_xyz's and d_scale's gradients (asserted on what autograd hands over).  Against tests/deform_ref64.py run over the rows of BOTH
    calls (the parameters' gradients hold the first call's five rows too) at the bounds of tests/test_gpu_35_deform_network.py
    test_against_float64: outputs rtol 1e-4 / atol 2e-5; gradients 1e-4 norm-wise below 1000 points and, from 1000 points on, 1e-2
    (parameters) / 5e-3 (data), where float32 meets ReLU-boundary decisions; state and inputs drawn with that test's seeds for this
    configuration.  (b): outputs and every gradient bit-equal to the aligned run (test_deterministic)."""
    from bilateral_driving_amd import deform as D
    from tests import test_gpu_35_deform_network as T35
    from tests.deform_ref64 import grads64, rel
    m = T35.make(D, "cond", True, True).cuda()
    sd = T35.seeded_state(m, 7 + 2)      # (the state and input seeds of test_against_float64's ("cond", True, True) rows)
    m.load_state_dict(sd, strict=True)
    x, t, c = T35.inputs(N, 16, seed=N + 2)
    x0, t0, c0 = T35.inputs(5, 16, seed=3)
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(N, k, generator=g).cuda() for k in (3, 4, 3)]
    ws0 = [torch.randn(5, k, generator=g).cuda() for k in (3, 4, 3)]
    both = lambda a, b: torch.cat([a, b])
    ref_outs, ref = grads64({k: v.double().cuda() for k, v in sd.items()}, both(x0, x), both(t0, t), both(c0, c),
                            [both(a, b) for a, b in zip(ws0, ws)])
    params = dict(m.named_parameters())
    p_tol, d_tol = (1e-2, 5e-3) if N + 5 >= 1000 else (1e-4, 1e-4)
    base = None
    for label, p in placements(dict(x=x, t=t, cond=c)):
        m.zero_grad(set_to_none=True)
        first = m(x0, t0, c0)
        xs, ts, cs = leaf(p["x"]), leaf(p["t"]), leaf(p["cond"])
        outs = m(xs, ts, cs)
        seen = []
        for o in outs:
            o.register_hook(lambda g_, seen=seen: seen.append((phase(g_), g_.is_contiguous())))
        sum((cat_grad([a, b]) * both(wa, wb)).sum() for a, b, wa, wb in zip(first, outs, ws0, ws)).backward()
        assert sorted(seen) == sorted([((5 * k * 4) % 16, True) for k in (3, 4, 3)]) and (5 * 3 * 4) % 16 != 0, seen
        for o, r in zip(outs, ref_outs):
            torch.testing.assert_close(o.detach().double(), r[5:], rtol=1e-4, atol=2e-5)
        got = {k: prm.grad for k, prm in params.items()}
        for k in params:
            assert float(ref[k].norm()) > 0 and rel(got[k], ref[k]) < p_tol, (label, k, rel(got[k], ref[k]))
        got.update(x=xs.grad, t=ts.grad, cond=cs.grad)
        for k in ("x", "t", "cond"):
            assert float(ref[k][5:].norm()) > 0 and rel(got[k], ref[k][5:]) < d_tol, (label, k, rel(got[k], ref[k][5:]))
        res = [o.detach() for o in outs] + [got[k] for k in sorted(got)]
        if base is None:
            base = res
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (label, i)


@pytest.mark.parametrize("N", [5, 1027])
def test_pvg_time_transform(N):
    """pvg.time_transform with its nine raw inputs placed and the gradients of its five compacted outputs arriving through a real
    ``torch.cat`` behind five rows of another tensor (15 / 5 / 15 / 15 / 20 floats in front: all but the quaternions' 4-byte aligned
    only, asserted on what autograd hands over).  Against tests/pvg_ref64.py at the bound of tests/test_gpu_37_pvg.py
    test_fused_matches_float64_over_sizes (``measured_bound``: 4 x the float32 framework's own error against float64, at least 1e-6),
    equal masks, dropped rows' gradients exactly zero.  (b): outputs and gradients bit-equal to the aligned run
    (test_two_runs_are_bit_identical)."""
    from bilateral_driving_amd import pvg as P
    from tests.pvg_ref64 import OUTS, RAW, SETTINGS, T, WEIGHTS, measured_bound, random_rows, run_framework, scaled_err, settle_clamp
    d = random_rows(N, 100 + N % 89)
    setting = SETTINGS[1 + N % 2]
    settle_clamp(d, setting, 3)
    ref = run_framework(d, setting, 3, sh=G.spherical_harmonics)
    bound, _ = measured_bound(d, setting, 3, ref)
    ro, rm, rg = ref
    assert 0 < int(rm.sum()) < N
    cur, dt, smooth = setting
    widths = (3, 1, 3, 3, 4)
    base = None
    for label, p in placements({k: d[k].cuda().float() for k in RAW}):
        ts = {k: leaf(p[k]) for k in RAW}
        *outs, mask = P.time_transform(*[ts[k] for k in RAW], d["cam_pos"].cuda(), cur, dt, smooth, T, 3)
        np.testing.assert_array_equal(mask.cpu().numpy(), rm)
        seen = []
        for o in outs:
            o.register_hook(lambda g_, seen=seen: seen.append((phase(g_), g_.is_contiguous())))
        heads = [torch.zeros(5, k, device="cuda", requires_grad=True) for k in widths]
        sum((cat_grad([h, o]) * torch.cat([torch.ones(5, k, device="cuda"), d[w].cuda()[mask]])).sum()
            for h, o, k, w in zip(heads, outs, widths, WEIGHTS)).backward()
        assert sorted(seen) == sorted(((5 * k * 4) % 16, True) for k in widths), seen
        for k, o in zip(OUTS, outs):
            assert scaled_err(o.detach().cpu().numpy(), ro[k]) <= bound, (label, k, scaled_err(o.detach().cpu().numpy(), ro[k]), bound)
        for k in RAW:
            gk = ts[k].grad.cpu().numpy()
            assert scaled_err(gk, rg[k]) <= bound, (label, k, scaled_err(gk, rg[k]), bound)
            assert np.abs(gk[~rm]).max(initial=0.0) == 0.0, (label, k)
        res = [o.detach() for o in outs] + [ts[k].grad for k in RAW]
        if base is None:
            base = res
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (label, i)


@pytest.mark.parametrize("I,V", [(1, 5), (13, 79)], ids=["N5", "N1027"])
def test_smpl_skin_transform(I, V):
    """smpl.skin_transform with the points' means / quats placed (the pose tables, the template and the correction field are
    parameters and buffers of their own) and the gradients of the world means / quats arriving through a real ``torch.cat`` behind five
    rows (15 floats in front of the means' gradient: 4-byte aligned only, asserted).  Against tests/smpl_skin_ref64.py at the bound
    of tests/test_gpu_55_smpl_skin.py test_fused_matches_float64 (``measured_bound``).  (b): the outputs and the gradients of means,
    quats and the three pose tables bit-equal to the aligned run, as test_poisoned_allocations_and_determinism asserts run to run; the
    correction field's gradient is summed with float atomics in an unspecified order (include/bds.h:956): the bound only."""
    from bilateral_driving_amd import smpl as S
    from tests import smpl_skin_ref64 as R
    d = R.make_inputs(I, V, (3, 5, 7), seed=7 * I + V, absent=(1,) if I > 1 else ())
    assert I * V in (5, 1027)
    ref = R.run_framework(d, 1)
    bound, _ = R.measured_bound(d, 1, ref)
    kw = R.template_kwargs(d, device="cuda")
    base = None
    for label, p in placements(dict(means=d["means"].cuda(), quats=d["quats"].cuda())):
        ts = {k: leaf(d[k].cuda().clone()) for k in R.INPUTS if d.get(k) is not None}
        ts["means"], ts["quats"] = leaf(p["means"]), leaf(p["quats"])
        wm, wq = S.skin_transform(ts["means"], ts["quats"], ts["instances_quats"], ts["smpl_quats"], ts["instances_trans"],
                                  d["instances_fv"].cuda(), 1, voxel_corr=ts.get("voxel_corr"), interpolate=False, ball=False, **kw)
        seen = []
        for o in (wm, wq):
            o.register_hook(lambda g_, seen=seen: seen.append((phase(g_), g_.is_contiguous())))
        heads = [torch.zeros(5, k, device="cuda", requires_grad=True) for k in (3, 4)]
        sum((cat_grad([h, o]) * torch.cat([torch.ones_like(h), d[w].cuda()])).sum() for h, o, w in zip(heads, (wm, wq), ("w_m", "w_q"))).backward()
        assert sorted(seen) == sorted([((5 * 3 * 4) % 16, True), ((5 * 4 * 4) % 16, True)]) and (5 * 3 * 4) % 16 != 0, seen
        outs = {"wm": wm.detach().cpu().numpy(), "wq": wq.detach().cpu().numpy()}
        grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy() for k, t in ts.items()}
        worst = R.worst(outs, grads, ref)
        assert worst <= bound, (label, worst, bound)
        res = [wm.detach(), wq.detach()] + [ts[k].grad for k in ("means", "quats", "instances_quats", "smpl_quats", "instances_trans")]
        if base is None:
            base = res
        assert len(res) == len(base)
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (label, i)


# =====================================================================================================================================
# G. the error-driven sampler's maps
# =====================================================================================================================================
@pytest.mark.parametrize("h,w", [(5, 7), (6, 7), (17, 23)], ids=["5x7-odd", "6x7-even", "17x23-odd"])
@pytest.mark.parametrize("with_dyn", [True, False], ids=["dyn", "nodyn"])
def test_error_maps(h, w, with_dyn):
    """sampler.error_maps with pred / gt / dyn / maps (and the statistics, the int64 slots and image ids) placed: all together at every
    offset, and each of the four arrays the device-side choice names alone (csrc/error_buffer.hip:121: four pixels at a time only when
    all four are 16-byte aligned), for an even and an odd number of pixels.  Against tests/error_buffer_ref64.py by the checks of
    tests/test_gpu_52_error_buffer.py (``check_outputs``: the maps bit-equal to the float32 restatement, 6 * 2^-24 from float64, the
    mean within 2^-23, min / max equal, the other rows untouched), and maps and statistics bit-equal to the aligned run, as there."""
    from bilateral_driving_amd import sampler as S
    from tests import test_gpu_52_error_buffer as T52
    B = 3
    pred, gt, dyn, ref = T52.case(h, w, B)
    f32, f64 = ref[with_dyn]
    F, num_imgs = B + T52.EXTRA_MAPS, B + T52.EXTRA_STATS
    rng = np.random.default_rng(7)
    fill_maps, fill_stats = rng.uniform(-9, -1, (F, h, w)).astype(np.float32), rng.uniform(-9, -1, (num_imgs, 3)).astype(np.float32)
    slots, ids = T52.ids_for(B, F), T52.ids_for(B, num_imgs)
    src = dict(pred=T52.dev(pred), gt=T52.dev(gt), dyn=T52.dev(dyn) if with_dyn else None, maps=T52.dev(fill_maps), stats=T52.dev(fill_stats),
               slots=T52.dev(np.int64(slots)), ids=T52.dev(np.int64(ids)))
    base = None
    for label, p in placements(src, named=("pred", "gt", "maps") + (("dyn",) if with_dyn else ())):
        S.error_maps(p["pred"], p["gt"], p["dyn"], p["maps"], p["slots"], p["stats"], p["ids"])
        maps, stats = T52.host(p["maps"]), T52.host(p["stats"])
        T52.check_outputs(maps, stats, fill_maps, fill_stats, slots, ids, f32, f64, f"{h}x{w} {label}")
        if base is None:
            base = (maps, stats)
        assert T52.same_bits(maps, base[0]) and T52.same_bits(stats, base[1]), label


@pytest.mark.parametrize("H,W,res", [(50, 70, 32), (13, 21, 7)], ids=["50x70-tiled", "13x21-per-tap"])
def test_cubemap_sample(H, W, res):
    """envlight.cubemap_sample with the texture, the directions (image-shaped [H,W,3]: the backward that pre-sums pixel tiles, from 16 x 16
    pixels on; and flat [H*W,3]) and the incoming gradient placed, against oracle/cubemap_oracle.py at the bounds of
    tests/test_gpu_13_envlight.py: the lookup within 2e-6 of the float32 oracle in all but 2e-4 of the pixels (a floor() on a texel
    boundary may flip) and the 99.5th percentile within 5e-4 of the float64 oracle (test_forward_and_texture_gradient_equal_oracle);
    the texture gradient within 1e-4 of its largest entry
    (test_image_shaped_directions_use_the_tiled_gradient_and_equal_oracle).  Float-by-float loads; the gradient is summed with float
    atomics: (a) only."""
    from bilateral_driving_amd.envlight import cubemap_sample
    from oracle import cubemap_oracle as CO
    rng = np.random.default_rng(H + W)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    f = 0.5 * W / np.tan(np.radians(35.0))
    d = np.stack([(jj - W / 2) / f, (ii - H / 2) / f, np.ones_like(jj)], -1).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d[0, 0] = np.nan; d[-1, -1] = 0
    tex = rng.random((6, res, res, 3)).astype(np.float32)
    v = (rng.standard_normal((H, W, 3)) * (rng.random((H, W, 1)) < 0.4)).astype(np.float32)
    rot = CO.TO_OPENGL.astype(np.float32)
    ref32 = CO.cubemap_fwd(tex, d, rot, dtype=np.float32)
    ref64 = CO.cubemap_fwd(tex.astype(np.float64), d.astype(np.float64), rot.astype(np.float64))
    g_ref = CO.cubemap_bwd(tex.shape, d, v, rot, dtype=np.float32)
    denom = np.abs(g_ref).max() + 1e-12
    assert np.abs(g_ref).sum() > 0
    src = dict(tex=torch.from_numpy(tex).cuda(), dirs=torch.from_numpy(d).cuda(), v=torch.from_numpy(v).cuda(), rot=torch.from_numpy(rot).cuda())
    for label, p in placements(src):
        for shaped in (True, False):
            t_tex = leaf(p["tex"])
            out = cubemap_sample(t_tex, p["dirs"] if shaped else p["dirs"].reshape(-1, 3), p["rot"])
            assert p["dirs"].reshape(-1, 3).data_ptr() == p["dirs"].data_ptr()
            got = out.detach().cpu().numpy().reshape(H, W, 3)
            ok = ~(np.isnan(ref32) | np.isnan(ref64))      # (test_gpu_13's comparisons pass over what the oracle leaves undefined)
            assert ok.mean() > 0.99 and not np.isnan(got[ok]).any(), (label, shaped)
            assert (np.abs(got - ref32)[ok] > 2e-6).mean() < 2e-4, (label, shaped)
            assert np.percentile(np.abs(got - ref64)[ok], 99.5) < 5e-4, (label, shaped)
            out.backward(p["v"].reshape(out.shape))      # (the incoming gradient already placed)
            assert phase(p["v"].reshape(out.shape)) == phase(p["v"])
            assert np.abs(t_tex.grad.cpu().numpy() - g_ref).max() / denom < 1e-4, (label, shaped)


def test_slice_entries():
    """bilagrid.slice (12 channels), slice_feature (8 feature channels, the point form) and slice_feature_image (24 channels over the
    pixel grid: ``_SliceImage``) with xy / rgb placed and the incoming gradient re-placed, 37 x 53 points, the grid picked out of a
    stack of three.  Against oracle/bilagrid_oracle.py ``slice_grid`` (+ ``apply_affine``) in float64 at the bounds of these entries'
    existing tests in tests/test_gpu_00_bilagrid_parity.py: ``slice`` -- maps and colours rtol 1e-4 / atol 1e-5, d/d rgb rtol 2e-3 /
    atol 2e-4, d/d grids 2e-4 of max(1, largest entry) (test_slice_api_vs_reference_golden); the feature forms -- features 2e-5, both
    gradients 5e-5 of the largest entry (test_feature_grid_slice_matches_reference_goldens; tests/test_gpu_12_neural_modules.py holds
    the image form bit-equal to the point form).  Float-by-float loads; the grids' gradients are summed with atomics: (a) only."""
    import bilateral_driving_amd.bilagrid as B
    H, W = 37, 53
    P = H * W
    g = torch.Generator().manual_seed(58)
    xy, rgb = torch.rand(P, 2, generator=g), torch.rand(P, 3, generator=g) * 1.2 - 0.1
    idx = torch.ones(P, 1, dtype=torch.long)
    bg = B.BilateralGrid(3, grid_X=5, grid_Y=7, grid_W=3).cuda()
    net = B.NeuralBilateralGrid(3, 5, 7, 3, feature_dim=8).cuda()
    net_img = B.NeuralBilateralGrid(3, 16, 16, 8, feature_dim=24).cuda()
    from bilateral_driving_amd import _lib as L
    assert L.lib().bds_bilagrid_slice_feat_image_ok(24, 16, 16, 8)
    with torch.no_grad():
        for mod in (bg, net, net_img):
            mod.grids.add_(0.3 * torch.randn(mod.grids.shape, generator=g).cuda())
    w3, w8, w24 = torch.randn(P, 3, generator=g), torch.randn(P, 8, generator=g), torch.randn(H, W, 24, generator=g)
    img = rgb.reshape(H, W, 3)

    def ref64(mod, x, y, colour, w, apply):
        gr, c = leaf(mod.grids.detach().double().cpu()), leaf(colour.double())
        val = BO.slice_grid(gr[1], x.double(), y.double(), BO.rgb2gray(c))
        mats = val
        if apply:
            val = BO.apply_affine(val, c)
        (val * w.double()).sum().backward()
        return val.detach(), mats.detach(), c.grad, gr.grad

    r_slice = ref64(bg, xy[:, 0], xy[:, 1], rgb, w3, True)
    r_feat = ref64(net, xy[:, 0], xy[:, 1], rgb, w8, False)
    ys, xs = torch.meshgrid(torch.linspace(0, 1.0, H, dtype=torch.float64), torch.linspace(0, 1.0, W, dtype=torch.float64), indexing="ij")
    r_img = ref64(net_img, xs, ys, img, w24, False)
    src = dict(xy=xy.cuda(), rgb=rgb.cuda(), idx=idx.cuda(), w3=w3.cuda(), w8=w8.cuda(), w24=w24.cuda())
    for label, p in placements(src):
        o3, o8, o24 = (phase(p[k]) // 4 for k in ("w3", "w8", "w24"))
        # slice
        bg.grids.grad = None
        c = leaf(p["rgb"])
        res = B.slice(bg, p["xy"], c, p["idx"])
        (regrad(res["rgb"], o3) * p["w3"]).sum().backward()
        np.testing.assert_allclose(res["rgb_affine_mats"].reshape(-1, 12).detach().cpu().numpy(), r_slice[1].numpy(), rtol=1e-4, atol=1e-5, err_msg=label)
        np.testing.assert_allclose(res["rgb"].detach().cpu().numpy(), r_slice[0].numpy(), rtol=1e-4, atol=1e-5, err_msg=label)
        np.testing.assert_allclose(c.grad.cpu().numpy(), r_slice[2].numpy(), rtol=2e-3, atol=2e-4, err_msg=label)
        ref = r_slice[3].numpy()
        assert np.abs(ref[1]).max() > 0 and np.abs(bg.grids.grad.cpu().numpy() - ref).max() < 2e-4 * max(1.0, np.abs(ref).max()), label
        # slice_feature, the point form
        net.grids.grad = None
        c = leaf(p["rgb"])
        feats = B.slice_feature(net, p["xy"], c, p["idx"])["affine_features"]
        (regrad(feats, o8) * p["w8"]).sum().backward()
        assert feats.shape == (P, 8)
        assert rel_err(feats.cpu(), r_feat[0]) < 2e-5 and rel_err(c.grad.cpu(), r_feat[2]) < 5e-5, label
        assert rel_err(net.grids.grad.cpu(), r_feat[3]) < 5e-5, label
        # the image form
        net_img.grids.grad = None
        c = leaf(p["rgb"].view(H, W, 3))
        assert phase(c) == phase(p["rgb"])
        fi = B.slice_feature_image(net_img, c, 1)
        assert fi.shape == (1, H, W, 24)
        (regrad(fi[0], o24) * p["w24"]).sum().backward()
        assert rel_err(fi[0].cpu(), r_img[0]) < 2e-5 and rel_err(c.grad.cpu(), r_img[2]) < 5e-5, label
        assert rel_err(net_img.grids.grad.cpu(), r_img[3]) < 5e-5, label


# =====================================================================================================================================
# B (continued). the fused training view: harness.render_view and fused_view.train_view
# =====================================================================================================================================
@pytest.mark.parametrize("sh_in_pack", [False, True], ids=["dense-sh", "sh-in-pack"])
def test_fused_view_and_train_view(sh_in_pack, monkeypatch):
    """harness.render_view (+ training_loss, backward) and harness.train_view (fused_view.train_view, no autograd graph) with the
    [N,16,3] SH tensor and the target image as contiguous views at 4-byte alignment, each alone and both.  Two host-side decisions take
    their other branch: bilateral_driving_amd/fused_view.py:273 (the record pack evaluates the colours only from 16-byte aligned
    coefficient rows: else the dense SH pass, float by float) and :1004 (the loss rides on the colour transform's launch only for a
    16-byte aligned target: else the one-launch loss, whose wrapper copies).  Held to the aligned run at the bounds of
    tests/test_gpu_38_view_backward_share.py: equal radii, rgb / depth / opacity within 1e-4 of max(1, |ref|), every gradient 1e-3
    norm-relative and 2e-3 element-wise (tests/util.py ``grad_errors``); the loss within 2e-6 (tests/test_gpu_09_graph_frame.py
    test_loss_on_the_transform_launch_equals_the_separate_loss_launch).  The aligned run is what tests/test_gpu_03 / _38 tie to the
    oracle."""
    from bilateral_driving_amd import fused_view as FV
    from bilateral_driving_amd import harness as Hn
    from tests.util import grad_errors
    monkeypatch.setattr(FV, "SH_IN_PACK", sh_in_pack)
    N = 1027
    cam = Hn.ring_cameras(W_, H_, yaws_deg=(20.0,), device="cuda")[0]
    p0 = Hn.synthetic_scene(N, seed=5, device="cuda")
    grids0 = Hn.make_grids(1, device="cuda")
    gen = torch.Generator().manual_seed(5)
    sky0, target0 = torch.rand(H_, W_, 3, generator=gen).cuda(), torch.rand(H_, W_, 3, generator=gen).cuda()
    assert p0["sh"].shape == (N, 16, 3)

    def run(o_sh, o_t, direct):
        p = {k: leaf(placed(v, o_sh if k == "sh" else 0)) for k, v in p0.items()}
        grids, sky, target = [leaf(x.clone()) for x in grids0], leaf(sky0.clone()), placed(target0, o_t)
        assert phase(p["sh"]) == 4 * o_sh and phase(target) == 4 * o_t
        cam.viewmat.grad = None
        cam.viewmat.requires_grad_(True)
        if direct:
            gg = [torch.zeros_like(x) for x in grids]
            out = Hn.train_view(p, cam, grids, 0, sky, target, grid_grads=gg)
            loss, g_grids = float(out["loss"]), gg
        else:
            out = Hn.render_view(p, cam, grids, 0, sky)
            lt = Hn.training_loss(out, target, grids)
            lt.backward()
            loss, g_grids = float(lt.detach()), [x.grad for x in grids]
        torch.cuda.synchronize()
        img = {k: out[k].detach().clone() for k in ("rgb", "depth", "opacity")}
        grads = dict({k: t.grad.clone() for k, t in p.items()}, sky=sky.grad.clone(), viewmat=cam.viewmat.grad.clone(),
                     **{f"grid{i}": x.clone() for i, x in enumerate(g_grids)},
                     **({f"grid{i}_transform": x.grad.clone() for i, x in enumerate(grids)} if direct else {}))
        return img, out["info"]["radii"].clone(), loss, grads

    for direct in (False, True):
        ref_img, ref_radii, ref_loss, ref_g = run(0, 0, direct)
        assert int((ref_radii > 0).sum()) > 100
        for o_sh, o_t in [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 2), (2, 3), (3, 1)]:
            tag = (direct, o_sh, o_t)
            img, radii, loss, grads = run(o_sh, o_t, direct)
            assert torch.equal(radii, ref_radii), tag
            for k, ref in ref_img.items():
                e = float(((img[k] - ref).abs() / ref.abs().clamp(min=1.0)).max())
                assert e < 1e-4, (tag, k, e)
            assert abs(loss - ref_loss) <= 2e-6 * abs(ref_loss), (tag, loss, ref_loss)
            for k, ref in ref_g.items():
                assert float(ref.abs().max()) > 0, k
                rel, elem, _ = grad_errors(grads[k], ref)
                assert rel < 1e-3 and elem < 2e-3, (tag, k, rel, elem)


# =====================================================================================================================================
# G (continued). the exchange's union mask
# =====================================================================================================================================
@pytest.mark.parametrize("n", [5, 4096 + 37], ids=["5", "one-tile-plus-37"])
def test_union_slots_mask_placement(n):
    """bds_union_slots with the uint8 visibility mask 1 and 5 bytes behind a 16-byte boundary.  dist.FrameExchange allocates its masks
    itself (fresh allocations: no public entry hands the kernel a caller's mask), so the entry is driven directly, as
    tests/test_gpu_05_exchange.py test_union_slots_kernel_equals_the_framework_formulation drives it: the byte-by-byte arm of
    csrc/exchange.hip:26 (taken per 16-byte piece, on the device) gives the slot map, id list, cleared rows and count of the
    framework formulation, bit-equal to the aligned run's."""
    from bilateral_driving_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(n)
    mask0 = (torch.rand(n, generator=g) < 0.4).to(torch.uint8).cuda()
    mask0[0] = mask0[-1] = 1
    cap, K = max(2, int(mask0.sum()) - 1), 16      # (one member beyond the capacity: its slot is clamped)
    base = None
    for off in (0,) + OFFSETS[torch.uint8]:
        mask = placed(mask0, off)
        assert phase(mask) == off
        row_map = torch.empty(n, dtype=torch.int32, device="cuda")
        ids = torch.empty(cap, dtype=torch.int32, device="cuda")
        bufs = [torch.full(s, 7.0, device="cuda") for s in ((cap, 3), (cap, 4), (cap, 3), (cap,), (cap, K, 3))]
        cnt = torch.zeros(1, dtype=torch.int64).pin_memory()
        cnt_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
        wsb = lib.bds_union_slots_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        L.check(lib.bds_union_slots(n, L.ptr(mask), cap, K, L.ptr(row_map), L.ptr(ids), *[L.ptr(b) for b in bufs], L.ptr(ws), wsb,
                                    L.ptr(cnt_dev), cnt.data_ptr(), L.stream()), "bds_union_slots")
        torch.cuda.synchronize()
        count = int(mask0.sum())
        assert int(cnt[0]) == count == int(cnt_dev[0]), off
        slot = torch.cumsum(mask0, 0, dtype=torch.int32) - 1
        members = mask0.nonzero().squeeze(1)
        assert torch.equal(row_map[members], slot[members].clamp(max=cap - 1)), off
        kept = min(count, cap)
        assert torch.equal(ids[:kept], members[:kept].to(torch.int32)) and bool((ids[kept:] == -1).all()), off
        for b in bufs:
            assert float(b[:kept].abs().max()) == 0.0 and (kept == cap or bool((b[kept:] == 7.0).all())), off
        res = [row_map[members], ids] + bufs
        if base is None:
            base = res
        for i, (a, b) in enumerate(zip(res, base)):
            assert same_bits(a, b), (off, i)
