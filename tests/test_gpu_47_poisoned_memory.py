"""-m gpu: every HIP op on recycled, poisoned memory with guard bands (tests/poison.py; the audit behind the integer poison is
docs/poisoned_memory.md).

A case is a small closure over fixed inputs that calls a public entry point and returns named result tensors -- outputs, every
gradient, every info tensor a caller may read.  The harness runs it once as it is and once under ``poisoned_allocations``: every
``torch.empty`` / ``empty_like`` / ``new_empty`` / ``fused_view._empty`` buffer then lies between two 4 KiB guard bands, holds a NaN of
a known payload (integers: 0x7F bytes) and

* no guard may change (a store before or behind a buffer),
* no returned tensor may hold the poison pattern (an element no kernel wrote), outside a region its wrapper's docstring declares
  undefined (``masks``, with the quote),
* the results pass the check the op's own test makes against its float64 oracle or golden, at that test's bound,
* ops documented as deterministic return the same bits as the unpoisoned run.

BDS_POISON_FLOAT_ONLY=1 leaves the integer bodies zeroed (the first run on a new machine)."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import bilagrid_oracle as BO
from oracle import cubemap_oracle as CO
from oracle import gs_oracle as G
from tests import poison
from tests.util import grad_errors, make_scene, rel_err

pytestmark = pytest.mark.gpu

FLOAT_ONLY = os.environ.get("BDS_POISON_FLOAT_ONLY", "0") == "1"
CASES = {}


def case(name, int_bodies=True, deterministic=False):
    """Register ``fn() -> SimpleNamespace(run, check, masks={})`` (built once: the oracle runs once per case).  ``int_bodies``: the
    case's entries passed the audit of docs/poisoned_memory.md.  ``deterministic``: the op's docstring or test says so -- True for every
    result, or the names of the results it holds for (a forward documented as deterministic beside gradients summed with atomics)."""
    def deco(fn):
        CASES[name] = SimpleNamespace(name=name, build=functools.lru_cache(None)(fn), int_bodies=int_bodies, deterministic=deterministic)
        return fn
    return deco


def _bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8, 2: torch.int16}[t.element_size()])


def _guarded(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except RuntimeError as e:
        if poison.is_gpu_fault(e):
            pytest.exit(f"GPU fault in the unpoisoned run of {name}: {e}", returncode=3)
        raise


def pytest_generate_tests(metafunc):
    if "name" in metafunc.fixturenames:      # (the cases are registered further down in this module)
        metafunc.parametrize("name", list(CASES))


def test_case_on_poisoned_memory(name):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    c = CASES[name]
    b = c.build()
    plain = _guarded(name, b.run)
    with poison.poisoned_allocations(c.int_bodies and not FLOAT_ONLY, name=name) as pz:
        got = b.run()
        torch.cuda.synchronize()
        handed_out = len(pz.records)
    # (a wrapper whose every buffer is torch.zeros hands out nothing: the case then pins the values and the bits alone)
    assert handed_out > 0 or getattr(b, "zero_filled_only", False), "the case reached no allocation of a wrapper"
    assert set(got) == set(plain)
    masks = getattr(b, "masks", {})
    for k, t in got.items():
        if t is None:
            assert plain[k] is None, k
            continue
        bad = poison.holds_poison(t)
        if k in masks:
            undefined = masks[k](got)
            assert undefined.shape == t.shape and not bool(undefined.all()), k
            bad = bad & ~undefined
        assert not bool(bad.any()), f"poison in result {k}: {int(bad.sum())} of {t.numel()} elements, first at {bad.nonzero()[0].tolist()}"
    b.check(got)
    if c.deterministic:
        bitwise = set(got) if c.deterministic is True else set(c.deterministic)
        assert bitwise <= set(got), bitwise - set(got)
        for k, t in got.items():
            if t is not None and k in bitwise:
                same = _bits(t) == _bits(plain[k])
                if k in masks:
                    same = same | masks[k](got).reshape(same.shape)
                assert bool(same.all()), f"{k}: not the bits of the unpoisoned run"


def _cuda(x, grad=False):
    return x.detach().clone().float().cuda().requires_grad_(grad)


# ===================================================================================================================================
# gs_ops
# ===================================================================================================================================
def _sh_case(n, deg, masked):
    import bilateral_driving_amd.gs_ops as ops
    g = torch.Generator().manual_seed(n + deg)
    dirs, coeffs = torch.randn(n, 3, generator=g) * 2, torch.randn(n, 16, 3, generator=g)
    m = (torch.arange(n) % 5 != 1) if masked else None
    v = torch.randn(n, 3, generator=g)
    d_ref, c_ref = dirs.double().requires_grad_(True), coeffs.double().requires_grad_(True)
    ref = G.spherical_harmonics(deg, d_ref, c_ref, None if m is None else m.double())
    (ref * v.double()).sum().backward()

    def run():
        d_g, c_g = _cuda(dirs, True), _cuda(coeffs, True)
        out = ops.spherical_harmonics(deg, d_g, c_g, None if m is None else m.cuda())
        (out * v.cuda()).sum().backward()
        return dict(out=out.detach(), v_coeffs=c_g.grad, v_dirs=d_g.grad)

    def check(r):      # tests/test_gpu_01_gs_parity.py test_sh_fwd_bwd
        assert rel_err(r["out"].cpu(), ref.detach()) < 1e-5
        assert rel_err(r["v_coeffs"].cpu(), c_ref.grad) < 1e-5
        if deg > 0:
            assert rel_err(r["v_dirs"].cpu(), d_ref.grad) < 1e-4
        else:
            assert float(r["v_dirs"].abs().max()) == 0.0      # (degree 0 does not depend on the direction)
        if m is not None and bool((~m).any()):
            assert float(r["out"][~m.cuda()].abs().max()) == 0.0 and float(r["v_coeffs"][~m.cuda()].abs().max()) == 0.0
    return SimpleNamespace(run=run, check=check)


for _n in (1, 65):
    for _deg in (0, 3):
        for _masked in (False, True):
            case(f"sh_n{_n}_deg{_deg}{'_masks' if _masked else ''}")(functools.partial(_sh_case, _n, _deg, _masked))


def _third_behind(sc, phase=1):
    """The scene with the rows i % 3 == phase mirrored through the camera centre (behind the near plane)."""
    vm = sc["viewmats"][0].double()
    R, t = vm[:3, :3], vm[:3, 3]
    pc = sc["means"].double() @ R.T + t
    pc[phase::3] *= -1.0
    sc = dict(sc)
    sc["means"] = ((pc - t) @ R).float()
    return sc


def _projection_case(N, phase=1):
    import bilateral_driving_amd.gs_ops as ops
    W, H, Cn = 100, 37, 2
    sc = _third_behind(make_scene(N, W, H, seed=2 + N, spread=1.5), phase)
    vm2 = sc["viewmats"][0].clone()
    vm2[:3, 3] += torch.tensor([0.2, 0.05, -0.1])
    vms, Ks = torch.stack([sc["viewmats"][0], vm2]), sc["Ks"].expand(2, 3, 3).contiguous()
    g = torch.Generator().manual_seed(N)
    w2, wd, wc, wp = (torch.randn(Cn, N, k, generator=g) for k in (2, 1, 3, 1))
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = {k: sc[k].to(dt).clone().requires_grad_(True) for k in ("means", "quats", "scales")}
        vm = vms.to(dt).clone().requires_grad_(True)
        outs = [G.project(leaves["means"], leaves["quats"], leaves["scales"], vm[c], Ks[c].to(dt), W, H, calc_compensations=True) for c in range(Cn)]
        ref[dt] = dict(leaves=leaves, vm=vm, radii=torch.stack([o[0] for o in outs]), m2=torch.stack([o[1] for o in outs]),
                       d=torch.stack([o[2] for o in outs]), c=torch.stack([o[3] for o in outs]), comp=torch.stack([o[4] for o in outs]))
    r64 = ref[torch.float64]

    def loss(m2, d, c, comp, same, dt):
        m = same.to(dt)
        return ((m2 * w2.to(m2) * m[..., None]).sum() + (d * wd[..., 0].to(d) * m).sum() + (c * wc.to(c) * m[..., None]).sum()
                + (comp * wp[..., 0].to(comp) * m).sum())

    def run():
        p = {k: _cuda(sc[k], True) for k in ("means", "quats", "scales")}
        vm_g = _cuda(vms, True)
        radii, m2, d, c, comp = ops.fully_fused_projection(p["means"], p["quats"], p["scales"], vm_g, Ks.cuda(), W, H, calc_compensations=True)
        same = (radii.cpu() == r64["radii"])
        loss(m2, d, c, comp, same.cuda(), torch.float32).backward()
        return dict(radii=radii, means2d=m2.detach(), depths=d.detach(), conics=c.detach(), compensations=comp.detach(),
                    v_means=p["means"].grad, v_quats=p["quats"].grad, v_scales=p["scales"].grad, v_viewmats=vm_g.grad)

    def check(r):      # tests/test_gpu_01_gs_parity.py test_projection_fwd_bwd, per camera, + the compensations at the conics' bound
        same = r["radii"].cpu() == r64["radii"]
        assert same.float().mean() >= 0.999
        vis = (r64["radii"] > 0) & same
        behind = len(range(phase, N, 3))
        assert int(vis.sum()) >= (max(1, Cn * N // 10) if behind < N else 0)
        assert int((r64["radii"] == 0).sum()) >= Cn * behind
        cull = r["radii"].cpu() == 0
        if bool(cull.any()):      # the meta tensors of culled rows are zeros (tests/test_gpu_25_gs_random_sweep.py)
            for k in ("means2d", "depths", "conics", "compensations"):
                assert float(r[k].cpu()[cull].abs().max()) == 0.0, k
        if not bool(vis.any()):      # the only row is culled in both cameras: every gradient is exactly zero
            assert bool(cull.all())
            for name in ("v_means", "v_quats", "v_scales", "v_viewmats"):
                assert float(r[name].abs().max()) == 0.0, name
            return
        assert rel_err(r["means2d"].cpu()[vis], r64["m2"].detach()[vis]) < 1e-5
        assert rel_err(r["depths"].cpu()[vis], r64["d"].detach()[vis]) < 1e-6
        assert ((r["conics"].cpu()[vis].double() - r64["c"].detach()[vis]).abs() / r64["c"].detach()[vis].abs().clamp(min=1e-3)).max() < 5e-4
        assert ((r["compensations"].cpu()[vis].double() - r64["comp"].detach()[vis]).abs() / r64["comp"].detach()[vis].abs().clamp(min=1e-3)).max() < 5e-4
        if "grads" not in ref:
            for dt in (torch.float64, torch.float32):
                q = ref[dt]
                loss(q["m2"], q["d"], q["c"], q["comp"], same, dt).backward()
            ref["grads"] = True
        for k, name in (("means", "v_means"), ("quats", "v_quats"), ("scales", "v_scales")):
            want = r64["leaves"][k].grad
            e = float((r[name].cpu().double() - want).norm() / want.norm())
            e32 = float((ref[torch.float32]["leaves"][k].grad.double() - want).norm() / want.norm())
            assert e < max(1e-4, 2.0 * e32), (k, e, e32)
        want = r64["vm"].grad[:, :3]
        assert float((r["v_viewmats"].cpu().double()[:, :3] - want).norm() / want.norm()) < 1e-4
    return SimpleNamespace(run=run, check=check)


for _n in (1, 257):
    case(f"projection_C2_N{_n}")(functools.partial(_projection_case, _n))
case("projection_C2_N1_culled")(functools.partial(_projection_case, 1, 0))      # the single row behind both cameras


def _raster_case(W, H, N, visible, CH):
    """isect_tiles + rasterize_to_pixels on fixed projected inputs, with a background and absgrad."""
    import bilateral_driving_amd.gs_ops as ops
    sc = make_scene(N, W, H, seed=W + N + CH)
    with torch.no_grad():
        radii, m2, d, con, _ = ops.fully_fused_projection(sc["means"].cuda(), sc["quats"].cuda(), sc["scales"].cuda(), sc["viewmats"].cuda(),
                                                          sc["Ks"].cuda(), W, H)
    if not visible:
        radii = torch.zeros_like(radii)
    g = torch.Generator().manual_seed(7)
    col = torch.rand(1, N, CH, generator=g)
    op = sc["opacities"][None].contiguous()
    bg = torch.rand(1, CH, generator=g)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    # oracle: the lists bit for bit, the blend in float64 on the kernels' own inputs and lists
    tpg_o, iids_o, fids_o = G.isect_tiles(m2[0].cpu(), radii[0].cpu(), d[0].cpu(), 16, tw, th)
    offs_o = G.isect_offset_encode(iids_o, tw, th)
    lv = {k: v.detach().cpu().double().requires_grad_(True) for k, v in dict(m2=m2[0], con=con[0], col=col[0], op=op[0], bg=bg[0]).items()}
    probe = []
    r64, a64, _, unstable = G.rasterize_to_pixels(lv["m2"], lv["con"], lv["col"], lv["op"], W, H, 16, offs_o, fids_o, lv["bg"], return_unstable=True,
                                                  absgrad_probe=probe)
    stable = ~unstable
    wt = torch.randn(r64.shape, generator=g) * stable[..., None]
    wa = torch.randn(a64.shape, generator=g) * stable[..., None]
    ((r64 * wt.double()).sum() + (a64 * wa.double()).sum()).backward()
    absgrad_ref = G.absgrad_from_probe(probe, N) if fids_o.numel() else torch.zeros(N, 2, dtype=torch.float64)

    def run():
        tpg, iids, fids, offs = ops.isect_tiles(m2, radii, d, 16, tw, th)
        x = {k: _cuda(v, True) for k, v in dict(m2=m2, con=con, col=col, op=op, bg=bg).items()}
        r, a = ops.rasterize_to_pixels(x["m2"], x["con"], x["col"], x["op"], W, H, 16, offs, fids, backgrounds=x["bg"], absgrad=True)
        ((r * wt.cuda()[None]).sum() + (a * wa.cuda()[None]).sum()).backward()
        return dict(tiles_per_gauss=tpg, isect_ids=iids, flatten_ids=fids, isect_offsets=offs, render=r.detach(), alphas=a.detach(),
                    v_means2d=x["m2"].grad, v_conics=x["con"].grad, v_colors=x["col"].grad, v_opacities=x["op"].grad, v_backgrounds=x["bg"].grad,
                    absgrad=x["m2"].absgrad)

    def check(r):
        # tests/test_gpu_01_gs_parity.py: test_isect_bit_exact; test_rasterization_end_to_end (images, absgrad);
        # test_backward_schedule_is_a_permutation_and_invisible (gradients on the kernels' own lists: 1e-3)
        assert torch.equal(r["tiles_per_gauss"][0].cpu(), tpg_o) and torch.equal(r["isect_ids"].cpu(), iids_o)
        assert torch.equal(r["flatten_ids"].cpu().long(), fids_o.long()) and torch.equal(r["isect_offsets"][0].cpu(), offs_o.reshape(th, tw).to(torch.int32))
        rc, ac = r["render"][0].cpu().double(), r["alphas"][0].cpu().double()
        err = (rc - r64.detach()).abs() / r64.detach().abs().clamp(min=1.0)
        assert float(err[stable].max()) < 1e-4 and float((ac - a64.detach()).abs()[stable].max()) < 1e-4
        names = dict(m2="v_means2d", con="v_conics", col="v_colors", op="v_opacities", bg="v_backgrounds")
        if not visible:
            assert float(ac.abs().max()) == 0.0 and torch.equal(r["render"][0].cpu(), bg[0].expand(H, W, CH))
            for k, name in names.items():
                if k != "bg":
                    assert float(r[name].abs().max()) == 0.0, name
            assert float(r["absgrad"].abs().max()) == 0.0 and r["flatten_ids"].numel() == 0
        for k, name in names.items():
            want, got = lv[k].grad, r[name][0].cpu().double()
            if want is not None and float(want.abs().max()) > 0:
                assert float((got - want).norm() / want.norm()) < 1e-3, name
        if float(absgrad_ref.abs().max()) > 0:
            assert float((r["absgrad"][0].cpu().double() - absgrad_ref).norm() / absgrad_ref.norm()) < 1e-3
    return SimpleNamespace(run=run, check=check)


# ("forward is deterministic": tests/test_gpu_01_gs_parity.py test_permutation_and_determinism; the gradients sum with float atomics)
RASTER_FORWARD = ("tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets", "render", "alphas")
for _w, _h in ((17, 9), (65, 33)):
    for _ch in (1, 3, 4):
        case(f"isect_rasterize_{_w}x{_h}_N40_ch{_ch}", deterministic=RASTER_FORWARD)(functools.partial(_raster_case, _w, _h, 40, True, _ch))
    case(f"isect_rasterize_{_w}x{_h}_nothing_visible", deterministic=RASTER_FORWARD)(functools.partial(_raster_case, _w, _h, 40, False, 3))


# ===================================================================================================================================
# rendering.rasterization
# ===================================================================================================================================
PARAMS = ("means", "quats", "scales", "opacities", "colors")


def _render_oracle(p, vms, Ks, W, H, mode, bg, sh_degree, aa, probes=None):
    """The oracle's stages camera by camera (tests/util.py aa_oracle, with the classic mode and the depth-only modes beside it)."""
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    rs, als, uns, rad = [], [], [], []
    for c in range(vms.shape[0]):
        radii, m2, dep, con, comp = G.project(p["means"], p["quats"], p["scales"], vms[c], Ks[c], W, H, calc_compensations=True)
        cam_pos = torch.linalg.inv(vms[c])[:3, 3]
        col = torch.clamp_min(G.spherical_harmonics(sh_degree, p["means"] - cam_pos, p["colors"], masks=radii > 0) + 0.5, 0.0)
        if mode in ("RGB+D", "RGB+ED"):
            col = torch.cat([col, dep[:, None]], -1)
        elif mode in ("D", "ED"):
            col = dep[:, None]
        b = None
        if bg is not None:
            b = {"RGB": bg[c], "D": bg.new_zeros(1), "ED": bg.new_zeros(1)}.get(mode, torch.cat([bg[c], bg.new_zeros(1)]))
        _, iids, fids = G.isect_tiles(m2, radii, dep, 16, tw, th)
        probe = None
        if probes is not None:
            probe = []
            probes.append(probe)
        r, a, _, un = G.rasterize_to_pixels(m2, con, col, p["opacities"] * comp if aa else p["opacities"], W, H, 16,
                                            G.isect_offset_encode(iids, tw, th), fids, b, return_unstable=True, absgrad_probe=probe)
        if mode in ("ED", "RGB+ED"):
            r = torch.cat([r[..., :-1], r[..., -1:] / a.clamp(min=1e-10)], -1)
        rs.append(r); als.append(a); uns.append(un); rad.append(radii)
    return torch.stack(rs), torch.stack(als), torch.stack(uns), torch.stack(rad)


def _rasterization_case(mode, visible=True, aa=False):
    import bilateral_driving_amd.rendering as R
    W, H, N = 65, 33, 200
    sc = make_scene(N, W, H, seed=31)
    g = torch.Generator().manual_seed(5)
    vm2 = sc["viewmats"][0].clone()
    vm2[:3, 3] += torch.tensor([0.15, -0.05, 0.1])
    vms, Ks = torch.stack([sc["viewmats"][0], vm2]), sc["Ks"].expand(2, 3, 3).contiguous()
    sc["colors"] = torch.randn(N, 16, 3, generator=g) * 0.3
    if not visible:      # every centre behind both cameras
        pc = sc["means"].double() @ vms[0, :3, :3].double().T + vms[0, :3, 3].double()
        pc[:, 2] = -pc[:, 2] - 5.0
        sc["means"] = ((pc - vms[0, :3, 3].double()) @ vms[0, :3, :3].double()).float()
    bg = torch.rand(2, 3, generator=g)
    ref, ref32 = {}, {}
    o = {}
    for dt, store in ((torch.float64, ref), (torch.float32, ref32)):
        p = {k: sc[k].to(dt).clone().requires_grad_(True) for k in PARAMS}
        vm = vms.to(dt).clone().requires_grad_(True)
        r, a, un, radii = _render_oracle(p, vm, Ks.to(dt), W, H, mode, bg.to(dt), 3, aa)
        if dt == torch.float64:
            stable = ~un
            gg = torch.Generator().manual_seed(1)
            o.update(r=r.detach(), a=a.detach(), stable=stable, wt=torch.randn(r.shape, generator=gg) * stable[..., None],
                     wa=torch.randn(a.shape, generator=gg) * stable[..., None], radii=radii)
        else:
            o["radii32_equal"] = bool(torch.equal(radii, o["radii"]))
        loss = (r * o["wt"].to(dt)).sum() + (a * o["wa"].to(dt)).sum()
        if loss.requires_grad:      # (nothing visible: the image is the background alone)
            loss.backward()
        store.update({k: v.grad for k, v in p.items()}, viewmats=vm.grad)

    def run():
        p = {k: _cuda(sc[k], True) for k in PARAMS}
        vm = _cuda(vms, True)
        r, a, meta = R.rasterization(p["means"], p["quats"], p["scales"], p["opacities"], p["colors"], vm, Ks.cuda(), W, H, sh_degree=3,
                                     backgrounds=bg.cuda(), render_mode=mode, absgrad=True, rasterize_mode="antialiased" if aa else "classic")
        ((r * o["wt"].cuda()).sum() + (a * o["wa"].cuda()).sum()).backward()
        out = dict(render=r.detach(), alphas=a.detach(), v_viewmats=vm.grad, absgrad=meta["means2d"].absgrad)
        out.update({"v_" + k: v.grad for k, v in p.items()})
        out.update({"meta_" + k: meta[k].detach() for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss", "flatten_ids",
                                                             "isect_offsets")})
        return out

    def check(r):
        # tests/test_gpu_01_gs_parity.py test_rasterization_end_to_end: equal radii, images 1e-4, gradients 1e-3 in norm, 2e-3 / 3e-4 per
        # element (worst / 99th percentile) and within 2x of the same oracle in float32
        assert torch.equal(r["meta_radii"].cpu(), o["radii"].to(torch.int32)), "fp32 / fp64 cull decisions differ: pick another seed"
        stable = o["stable"]
        assert stable.float().mean() > 0.98
        err = (r["render"].cpu().double() - o["r"]).abs() / o["r"].abs().clamp(min=1.0)
        assert float(err[stable].max()) < 1e-4, float(err[stable].max())
        assert float((r["alphas"].cpu().double() - o["a"]).abs()[stable].max()) < 1e-4
        cull = r["meta_radii"].cpu() == 0
        for k in ("meta_means2d", "meta_depths", "meta_conics"):
            if bool(cull.any()):
                assert float(r[k].cpu()[cull].abs().max()) == 0.0, k
        if not visible:      # the image is the background, alphas are 0, every gradient is exactly zero
            assert float(r["alphas"].abs().max()) == 0.0
            want = {"RGB": bg, "D": bg.new_zeros(2, 1), "ED": bg.new_zeros(2, 1)}.get(mode, torch.cat([bg, bg.new_zeros(2, 1)], -1))
            assert torch.equal(r["render"].cpu(), want[:, None, None, :].expand(2, H, W, want.shape[-1]))
            for k in list(PARAMS) + ["viewmats"]:
                assert r["v_" + k] is None or float(r["v_" + k].abs().max()) == 0.0, k
            assert float(r["absgrad"].abs().max()) == 0.0
            return
        assert float(o["a"].mean()) > 0.2
        for k, gref in ref.items():
            got = r["v_" + k]
            if gref is None or float(gref.abs().max()) == 0.0:      # e.g. the colours in the depth-only modes
                assert got is None or float(got.abs().max()) == 0.0, k
                continue
            rel, elem, elem99 = grad_errors(got, gref)
            assert rel < 1e-3, (k, rel)
            assert elem < 2e-3 and elem99 < 3e-4, (k, elem, elem99)
            if o["radii32_equal"] and k in PARAMS:      # (the camera pose: the bounds above alone, as tests/test_gpu_34 holds it)
                _, elem32, elem99_32 = grad_errors(ref32[k], gref)
                assert elem <= 2.0 * elem32 + 1e-4 and elem99 <= 2.0 * elem99_32 + 2e-5, (k, elem, elem32, elem99, elem99_32)
    return SimpleNamespace(run=run, check=check)


RENDER_FORWARD = ("render", "alphas", "meta_radii", "meta_means2d", "meta_depths", "meta_conics", "meta_opacities", "meta_tiles_per_gauss", "meta_flatten_ids", "meta_isect_offsets")
for _mode in ("RGB", "D", "ED", "RGB+D", "RGB+ED"):
    case(f"rasterization_C2_sh3_{_mode}", deterministic=RENDER_FORWARD)(functools.partial(_rasterization_case, _mode))
case("rasterization_C2_sh3_nothing_visible", deterministic=RENDER_FORWARD)(functools.partial(_rasterization_case, "RGB+ED", False))
case("rasterization_C2_sh3_antialiased", deterministic=RENDER_FORWARD)(functools.partial(_rasterization_case, "RGB+D", True, True))


# ===================================================================================================================================
# envlight
# ===================================================================================================================================
def _cubemap_case(res, shape):
    from bilateral_driving_amd.envlight import cubemap_sample
    rng = np.random.default_rng(res + len(shape))
    n = int(np.prod(shape[:-1]))
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d[0] = (np.nan, 1, 0)
    d[1] = (0, 0, 0)
    d[2:5] = [(1, 0, 0), (1, 1, 1), (-1, 1 + 1e-4, -1)]
    d = d.reshape(shape)
    tex = rng.random((6, res, res, 3)).astype(np.float32)
    rot = CO.TO_OPENGL.astype(np.float32)
    v = rng.standard_normal(tuple(shape[:-1]) + (3,)).astype(np.float32)
    v.reshape(-1, 3)[::3] = 0
    ref32 = CO.cubemap_fwd(tex, d, rot, dtype=np.float32)
    g_ref = CO.cubemap_bwd(tex.shape, d, v, rot, dtype=np.float32)

    def run():
        t = torch.from_numpy(tex).cuda().requires_grad_(True)
        out = cubemap_sample(t, torch.from_numpy(d).cuda(), torch.from_numpy(rot).cuda())
        out.backward(torch.from_numpy(v).cuda())
        return dict(out=out.detach(), v_tex=t.grad)

    def check(r):      # tests/test_gpu_13_envlight.py: forward 2e-6 against the float32 oracle, gradient 1e-3 (flat) / 1e-4 (image-shaped)
        got = r["out"].cpu().numpy()
        assert got.shape == ref32.shape and not (np.abs(got - ref32) > 2e-6).any()
        assert (got.reshape(-1, 3)[:2] == 0).all()                   # the NaN and the zero direction
        denom = np.abs(g_ref).max() + 1e-12
        assert np.abs(r["v_tex"].cpu().numpy() - g_ref).max() / denom < (1e-4 if len(shape) == 3 else 1e-3)
    return SimpleNamespace(run=run, check=check)


for _res in (1, 7):
    case(f"cubemap_res{_res}_dirs5")(functools.partial(_cubemap_case, _res, (5, 3)))
    case(f"cubemap_res{_res}_dirs16x16")(functools.partial(_cubemap_case, _res, (16, 16, 3)))


# ===================================================================================================================================
# fused_view through the harness
# ===================================================================================================================================
VIEW_W, VIEW_H, VIEW_N = 65, 33, 300
VIEW_FORWARD = ("rgb", "depth", "opacity", "radii", "means2d", "visible_ids", "flatten_ranks", "isect_offsets", "tiles_per_gauss")


@functools.lru_cache(None)
def _view_setup():
    """Scene, camera, grids, sky, target (CPU) and the float64 oracle of ``__graft_entry__.smoke_check`` -- forward, loss, every
    gradient, absgrad -- computed once for the three cases that share it."""
    from bilateral_driving_amd.harness import FACTORS_3, make_grids, ring_cameras, synthetic_scene
    W, H, N = VIEW_W, VIEW_H, VIEW_N
    cam = ring_cameras(W, H, yaws_deg=(0.0,))[0]
    p = synthetic_scene(N, seed=0)
    p["means"] = p["means"] * torch.tensor([0.25, 0.25, 1.0])
    grids = make_grids(2)
    gen = torch.Generator().manual_seed(3)
    sky, target = torch.rand(H, W, 3, generator=gen), torch.rand(H, W, 3, generator=gen)
    q = {k: v.double().requires_grad_(True) for k, v in p.items()}
    g64 = [g.double().requires_grad_(True) for g in grids]
    vm = cam.viewmat.double().requires_grad_(True)
    sky64 = sky.double().requires_grad_(True)
    dirs = q["means"].detach() - torch.linalg.inv(vm.detach())[:3, 3]
    col = torch.clamp(G.spherical_harmonics(3, dirs, q["sh"]) + 0.5, 0.0, 1.0)
    probes = []
    r, a, meta = G.rasterization(q["means"], q["quats"] / q["quats"].norm(dim=-1, keepdim=True), torch.exp(q["log_scales"]),
                                 torch.sigmoid(q["opacity_logits"]), col, vm[None], cam.K.double()[None], W, H, near_plane=0.1,
                                 render_mode="RGB+ED", return_unstable=True, absgrad_probes=probes)
    blended = BO.sky_blend(r[0, ..., :3], a[0], sky64)
    rgb_ref = BO.multiscale_transform([g[1] for g in g64], blended, list(FACTORS_3))
    loss_ref = (rgb_ref - target.double()).abs().mean() + 0.01 * BO.multiscale_tv(g64)
    loss_ref.backward()
    return SimpleNamespace(cam=cam, p=p, grids=grids, sky=sky, target=target, rgb=rgb_ref.detach(), alpha=a[0].detach(), stable=~meta["unstable"][0],
                           radii=meta["radii"], loss=float(loss_ref.detach()), grads={k: v.grad for k, v in q.items()},
                           grid_grads=[g.grad for g in g64], vm_grad=vm.grad, sky_grad=sky64.grad, absgrad=G.absgrad_from_probe(probes[0], N),
                           rgb_g=r[0, ..., :3].detach(), depth=r[0, ..., 3:4].detach())


def _view_inputs(s):
    from bilateral_driving_amd.harness import Camera
    cam = Camera(_cuda(s.cam.viewmat, True), s.cam.K.cuda(), s.cam.width, s.cam.height, s.cam.cam_pos.cuda())
    return (cam, {k: _cuda(v, True) for k, v in s.p.items()}, [_cuda(g, True) for g in s.grids], _cuda(s.sky, True), s.target.cuda())


def _view_results(out, cam, p, grids, sky):
    info = out["info"]
    r = dict(rgb=out["rgb"].detach(), depth=out["depth"].detach(), opacity=out["opacity"].detach(), v_viewmat=cam.viewmat.grad, v_sky=sky.grad,
             absgrad=info["means2d"].absgrad, radii=info["radii"], means2d=info["means2d"].detach(), visible_ids=info["visible_ids"],
             flatten_ranks=info["flatten_ranks"], isect_offsets=info["isect_offsets"], tiles_per_gauss=info["tiles_per_gauss"])
    r.update({"v_" + k: v.grad for k, v in p.items()})
    r.update({f"v_grid{i}": g.grad for i, g in enumerate(grids)})
    return r


def _view_check(s, r, loss):
    """The bounds of ``__graft_entry__.smoke_check`` (what tests/test_gpu_03_harness.py holds the fused view to)."""
    assert torch.equal(r["radii"].cpu().reshape(1, -1), s.radii.to(torch.int32)), "fp32 / fp64 cull decisions differ for this seed"
    diff = (r["rgb"].cpu().double() - s.rgb).abs()
    assert float((diff / s.rgb.abs().clamp(min=1.0))[s.stable].max()) < 1e-4
    sizable = s.stable[..., None] & (s.rgb.abs() > 1e-2)
    assert float((diff / s.rgb.abs().clamp(min=1e-2))[sizable].max()) < 2e-4
    assert abs(loss - s.loss) < 1e-5

    def nrm(got, ref):
        return float((got.cpu().double() - ref).norm() / ref.norm().clamp(min=1e-30))
    for k, ref in s.grads.items():
        assert nrm(r["v_" + k], ref) < 2e-3, k
        big = ref.abs() > 1e-3 * ref.abs().max()
        e = ((r["v_" + k].cpu().double() - ref).abs() / ref.abs().clamp(min=1e-300))[big].flatten()
        assert float(e.kthvalue(max(1, int(0.999 * e.numel()))).values) < 2e-3, k
    assert max(nrm(r[f"v_grid{i}"], g) for i, g in enumerate(s.grid_grads)) < 2e-3
    assert nrm(r["v_viewmat"], s.vm_grad) < 2e-3 and nrm(r["v_sky"], s.sky_grad) < 2e-3
    assert nrm(r["absgrad"].reshape(-1, 2), s.absgrad) < 2e-3
    # the lists: ascending visible ids; culled rows hold zeros
    vis = (r["radii"].reshape(-1) > 0).nonzero().squeeze(1)
    assert torch.equal(r["visible_ids"].long(), vis)
    cull = r["radii"].reshape(-1) == 0
    assert float(r["means2d"].reshape(-1, 2)[cull].abs().max()) == 0.0 and int(r["tiles_per_gauss"].reshape(-1)[cull].abs().max()) == 0


@case("fused_view_render_view", deterministic=VIEW_FORWARD)
def _render_view_case():
    from bilateral_driving_amd import harness as Hn
    s = _view_setup()
    box = {}

    def run():
        cam, p, grids, sky, target = _view_inputs(s)
        out = Hn.render_view(p, cam, grids, 1, sky)
        out["info"]["means2d"].retain_grad()
        loss = Hn.training_loss(out, target, grids)
        loss.backward()
        box["loss"] = float(loss.detach())
        r = _view_results(out, cam, p, grids, sky)
        r.update(rgb_gaussians=out["rgb_gaussians"].detach(), v_means2d=out["info"]["means2d"].grad)
        return r

    def check(r):
        _view_check(s, r, box["loss"])
        assert float((r["opacity"].cpu().double() - s.alpha).abs()[s.stable].max()) < 1e-4      # (test_gpu_01's bound on the alphas)
    return SimpleNamespace(run=run, check=check)


@case("fused_view_train_view", deterministic=VIEW_FORWARD)
def _train_view_case():
    from bilateral_driving_amd import harness as Hn
    s = _view_setup()
    box = {}

    def run():
        cam, p, grids, sky, target = _view_inputs(s)
        out = Hn.train_view(p, cam, grids, 1, sky, target)
        box["loss"] = float(out["loss"])
        r = _view_results(out, cam, p, grids, sky)
        r["loss"] = out["loss"].detach().reshape(1)
        return r
    return SimpleNamespace(run=run, check=lambda r: _view_check(s, r, box["loss"]))


def _train_view_caps_case(split_len):
    """The eager device-count form (``caps=``: what tests/test_gpu_09 / 21 / 22 / 28 call and graph_view captures): no host wait, the
    lists built into buffers of the given capacities, the backward's binned schedule (and the split area behind it) in one int32
    buffer from ``fused_view._empty`` that the compositor's forward fills.  ``split_len``: tiles whose list holds at least that many
    entries are composited strip by strip over refined lists from the pool behind the schedule (same image, bit for bit)."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.fused_view import ListCapacity
    s = _view_setup()
    box = {}
    cam, p, grids, sky, target = _view_inputs(s)
    with torch.no_grad():
        probe = Hn.train_view(p, cam, grids, 1, sky, target)
    torch.cuda.synchronize()
    M, nv = int(probe["info"]["n_isects"]), int(probe["info"]["n_visible"])
    assert M > 0 and nv > 0
    longest = int(torch.diff(torch.cat([probe["info"]["isect_offsets"].reshape(-1).long().cpu(), torch.tensor([M])])).max())
    assert longest >= max(split_len, 1), (longest, split_len)      # (some list tile really is "long": the split launch has strips to run)

    def run():
        cam, p, grids, sky, target = _view_inputs(s)
        caps = ListCapacity(int(M * 1.3) + 100, int(nv * 1.3) + 100)
        out = Hn.train_view(p, cam, grids, 1, sky, target, caps=caps, **({"split_len": split_len} if split_len else {}))
        torch.cuda.synchronize()
        assert caps.observed() == (M, nv) and not caps.overflowed(), (caps.observed(), (M, nv))
        box["loss"] = float(out["loss"])
        r = _view_results(out, cam, p, grids, sky)
        r["loss"] = out["loss"].detach().reshape(1)
        return r

    def check(r):
        assert r["visible_ids"].numel() == int(nv * 1.3) + 100 and r["flatten_ranks"].numel() == int(M * 1.3) + 100      # the capacities
        _view_check(s, dict(r, visible_ids=r["visible_ids"][:nv], flatten_ranks=r["flatten_ranks"][:M]), box["loss"])
        assert int(r["flatten_ranks"][:M].min()) >= 0 and int(r["flatten_ranks"][:M].max()) < nv
    # fused_view.fused_view: "``info["n_isects"]`` / ``["n_visible"]`` are then the CAPACITIES (the lists' tensors have those lengths;
    # entries beyond the counts are undefined)"
    return SimpleNamespace(run=run, check=check, masks={"visible_ids": lambda r: torch.arange(r["visible_ids"].numel(), device="cuda") >= nv,
                                                        "flatten_ranks": lambda r: torch.arange(r["flatten_ranks"].numel(), device="cuda") >= M})


case("fused_view_train_view_device_counts", deterministic=VIEW_FORWARD)(functools.partial(_train_view_caps_case, 0))
case("fused_view_train_view_device_counts_split", deterministic=VIEW_FORWARD)(functools.partial(_train_view_caps_case, 8))


@case("fused_view_render_classes", deterministic=True)      # ("forward is deterministic": tests/test_gpu_01 test_permutation_and_determinism)
def _render_classes_case():
    from bilateral_driving_amd.fused_view import render_classes
    s = _view_setup()
    N = VIEW_N

    def run():
        cam, p, _, _, _ = _view_inputs(s)
        masks = {"Nothing": torch.zeros(N, dtype=torch.bool, device="cuda"), "All": torch.ones(N, dtype=torch.bool, device="cuda"),
                 "Even": (torch.arange(N, device="cuda") % 2 == 0).float()}
        return dict(render_classes(p, cam.viewmat.detach(), cam.K, VIEW_W, VIEW_H, masks, cam_pos=cam.cam_pos))

    def check(r):      # tests/test_gpu_07_eval_rerenders.py
        for k in ("rgb", "depth", "opacity"):
            assert float(r["Nothing_" + k].abs().max()) == 0.0, k
        assert torch.equal(r["All_rgb"], r["rgb_gaussians"]) and torch.equal(r["All_opacity"], r["opacity"]) and torch.equal(r["All_depth"], r["depth"])
        np.testing.assert_allclose(r["opacity"].cpu().numpy(), s.alpha.numpy(), rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(r["rgb_gaussians"].cpu().numpy(), torch.clamp(s.rgb_g, max=1.0).numpy(), rtol=1e-4, atol=2e-5)
        covered = s.alpha.numpy()[..., 0] > 1e-3
        np.testing.assert_allclose(r["depth"].cpu().numpy()[covered], s.depth.numpy()[covered], rtol=2e-4, atol=1e-4)
        assert bool((r["Even_opacity"] <= r["opacity"] + 1e-6).all()) and float(r["Even_opacity"].max()) > 0.0
    return SimpleNamespace(run=run, check=check)


# ===================================================================================================================================
# losses
# ===================================================================================================================================
def _ssim_case(H, W):
    from oracle import loss_oracle as LO
    from bilateral_driving_amd.losses import ssim, ssim_loss
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + 0.15 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    p_ref = pred.clone().double().requires_grad_(True)
    s_ref = LO.ssim(gt.double(), p_ref)
    (1.7 * (1 - s_ref)).backward()

    def run():
        p = _cuda(pred, True)
        s = ssim(p, gt.cuda())
        (1.7 * ssim_loss(p, gt.cuda())).backward()
        return dict(ssim=s.detach().reshape(1), v_pred=p.grad)

    def check(r):      # tests/test_gpu_29_losses_random_sweep.py test_ssim_random_size
        assert abs(float(r["ssim"]) - float(s_ref.detach())) < 2e-5
        gref = p_ref.grad.float()
        assert float((r["v_pred"].cpu() - gref).abs().max()) <= 1e-4 * float(gref.abs().max()) + 1e-9
    return SimpleNamespace(run=run, check=check)


case("ssim_11x11")(functools.partial(_ssim_case, 11, 11))
case("ssim_12x27")(functools.partial(_ssim_case, 12, 27))


def _pixel_loss_case(H, W):
    """All terms, then each optional term dropped in turn (opacity / sky mask, depth / lidar, the ego-car mask)."""
    from oracle import loss_oracle as LO
    from bilateral_driving_amd.losses import pixel_loss
    g = torch.Generator().manual_seed(H * 100 + W)
    t = dict(rgb=torch.rand(H, W, 3, generator=g), pixels=torch.rand(H, W, 3, generator=g), opacity=torch.rand(H, W, 1, generator=g) * 0.98 + 0.01,
             depth=torch.rand(H, W, 1, generator=g) * 40 + 0.5, sky=(torch.rand(H, W, generator=g) > 0.7).float(),
             lidar=torch.rand(H, W, generator=g) * 60 * (torch.rand(H, W, generator=g) > 0.3).float(), ego=(torch.rand(H, W, generator=g) > 0.8).float())
    t["lidar"].reshape(-1)[0] = 12.0            # (at least one lidar hit: the depth term divides by their count)
    t["ego"].reshape(-1)[0] = 0.0
    variants = {"all": (True, True, True), "no_mask_term": (False, True, True), "no_depth_term": (True, False, True), "no_egocar": (True, True, False)}
    w = (0.8, 0.05, 0.01)
    ref = {}
    for tag, (um, ud, ue) in variants.items():
        d = {k: v.double() for k, v in t.items()}
        ref[tag] = LO.pixel_loss(d["rgb"], d["pixels"], d["opacity"], d["sky"], d["depth"], d["lidar"], d["ego"] if ue else None, w=w)

    def run():
        out = {}
        for tag, (um, ud, ue) in variants.items():
            rgb, op, dp = _cuda(t["rgb"], True), _cuda(t["opacity"], True), _cuda(t["depth"], True)
            terms = pixel_loss(rgb, op if um else None, dp if ud else None, t["pixels"].cuda(), t["sky"].cuda(), t["lidar"].cuda(),
                               t["ego"].cuda() if ue else None, *w)
            terms.sum().backward()
            out.update({f"{tag}_terms": terms.detach(), f"{tag}_v_rgb": rgb.grad, f"{tag}_v_opacity": op.grad, f"{tag}_v_depth": dp.grad})
        return out

    def check(r):      # tests/test_gpu_00_bilagrid_parity.py test_pixel_loss_matches_reference_goldens: 3e-6
        for tag, (um, ud, ue) in variants.items():
            z = ref[tag]
            for i, (k, on) in enumerate((("rgb_loss", True), ("sky_loss", um), ("depth_loss", ud))):
                want = float(z[k]) if on else 0.0
                assert abs(float(r[f"{tag}_terms"][i]) - want) <= 3e-6 * max(1.0, abs(want)), (tag, k)
            for k, on in (("v_rgb", True), ("v_opacity", um), ("v_depth", ud)):
                got = r[f"{tag}_{k}"]
                if not on:
                    assert got is None or float(got.abs().max()) == 0.0, (tag, k)
                    continue
                want = z[k]
                assert float((got.cpu().double() - want).abs().max()) / max(float(want.abs().max()), 1e-30) <= 3e-6, (tag, k)
    return SimpleNamespace(run=run, check=check)


case("pixel_loss_1px")(functools.partial(_pixel_loss_case, 1, 1))
case("pixel_loss_1000px")(functools.partial(_pixel_loss_case, 25, 40))


def _reg_losses_case(H, W):
    """Every subset of the terms the shape admits (the inverse-depth smoothness needs H, W > 1: tests/test_gpu_29 -- the 3x5 and 2x37
    cases run it in every combination), with and without the ego-car mask."""
    import itertools
    from oracle import loss_oracle as LO
    from bilateral_driving_amd import losses as Ls
    g = torch.Generator().manual_seed(12000 + W)
    pix, rgb = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g) * 1.1
    op = torch.rand(H, W, 1, generator=g)
    dep = torch.rand(H, W, 1, generator=g) * 30 + 0.2
    dyn = torch.rand(H, W, 1, generator=g)
    dyn.reshape(-1)[0] = 0.9
    ego = (torch.rand(H, W, generator=g) > 0.8).float()
    wt = torch.rand(3, generator=g) + 0.2
    subsets = [s for s in itertools.product((False, True), repeat=4) if (s[0] or s[1] or s[2]) and not (s[2] and (H == 1 or W == 1))]
    ref = {}
    for s in subsets:
        use_op, use_dyn, use_dep, use_ego = s
        o64 = {k: v.double().requires_grad_(True) for k, v in dict(op=op, dep=dep, rgb=rgb).items()}
        t_ref = LO.reg_losses(pix.double(), o64["op"] if use_op else None, o64["dep"] if use_dep else None, o64["rgb"],
                              dyn.double() if use_dyn else None, ego.double() if use_ego else None)
        if t_ref.requires_grad:
            (t_ref * wt.double()).sum().backward()
        ref[s] = (t_ref.detach(), {k: v.grad for k, v in o64.items()})

    def run():
        out = {}
        for s in subsets:
            use_op, use_dyn, use_dep, use_ego = s
            c = {k: _cuda(v, True) for k, v in dict(op=op, dep=dep, rgb=rgb).items()}
            t = Ls.reg_losses(pix.cuda(), c["op"] if use_op else None, c["dep"] if use_dep else None, c["rgb"], dyn.cuda() if use_dyn else None,
                              ego.cuda() if use_ego else None)
            if t.requires_grad:
                (t * wt.cuda()).sum().backward()
            tag = "".join("01"[int(b)] for b in s)
            out.update({f"{tag}_terms": t.detach(), f"{tag}_v_op": c["op"].grad, f"{tag}_v_dep": c["dep"].grad, f"{tag}_v_rgb": c["rgb"].grad})
        return out

    def check(r):      # tests/test_gpu_29_losses_random_sweep.py test_reg_losses_random_size_and_terms
        for s in subsets:
            tag = "".join("01"[int(b)] for b in s)
            t_ref, grads = ref[s]
            assert torch.allclose(r[f"{tag}_terms"].cpu().double(), t_ref, rtol=2e-5, atol=1e-7), (tag, r[f"{tag}_terms"], t_ref)
            for k in ("op", "dep", "rgb"):
                want, got = grads[k], r[f"{tag}_v_{k}"]
                if want is None or float(want.abs().max()) == 0.0:
                    assert got is None or float(got.abs().max()) == 0.0, (k, tag)
                    continue
                assert float((got.cpu().double() - want).norm() / want.norm()) < 2e-5, (k, tag)
    return SimpleNamespace(run=run, check=check)


case("reg_losses_1x1")(functools.partial(_reg_losses_case, 1, 1))
case("reg_losses_1x37")(functools.partial(_reg_losses_case, 1, 37))
case("reg_losses_3x5")(functools.partial(_reg_losses_case, 3, 5))      # (H, W > 1: the subsets with the inverse-depth smoothness term)
case("reg_losses_2x37")(functools.partial(_reg_losses_case, 2, 37))


def _photometric_case(n_grids):
    """photometric_tv_loss (the autograd node) and photometric_tv_train (one launch) against the framework expression over the
    per-level TV op, as tests/test_gpu_00_bilagrid_parity.py compares them."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.bilagrid import total_variation_loss
    from bilateral_driving_amd.losses import photometric_tv_loss, photometric_tv_train
    H, W = 9, 13
    g = torch.Generator().manual_seed(11)
    rgb0, target = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g)
    target[0, 0] = rgb0[0, 0]
    grids0 = Hn.make_grids(3, seed=3)[:n_grids]
    wts = [0.01 * 0.5 * math.sqrt(x.shape[4] * x.shape[3] * x.shape[2]) for x in grids0]
    pre0 = [torch.randn(x.shape, generator=g) for x in grids0]
    rgb, grids = _cuda(rgb0, True), [_cuda(x, True) for x in grids0]
    loss = (rgb - target.cuda()).abs().mean()
    for x, w in zip(grids, wts):
        loss = loss + total_variation_loss(x, w)
    loss.backward()
    ref = (loss.detach().clone(), rgb.grad.clone(), [x.grad.clone() for x in grids])

    def run():
        rgb, grids = _cuda(rgb0, True), [_cuda(x, True) for x in grids0]
        loss = photometric_tv_loss(rgb, target.cuda(), grids, wts)
        loss.backward()
        acc = [a.cuda() for a in pre0]
        got, v_rgb = photometric_tv_train(rgb.detach(), target.cuda(), [x.detach() for x in grids], wts, acc)
        out = dict(loss=loss.detach().reshape(1), v_rgb=rgb.grad, train_loss=got.reshape(1), train_v_rgb=v_rgb)
        out.update({f"v_grid{i}": x.grad for i, x in enumerate(grids)})
        out.update({f"train_acc{i}": a for i, a in enumerate(acc)})
        return out

    def check(r):
        assert abs(float(r["loss"] - ref[0])) <= 1e-6 * abs(float(ref[0]))
        assert torch.allclose(r["v_rgb"], ref[1], rtol=1e-6, atol=0) and float(r["v_rgb"][0, 0].abs().max()) == 0.0
        assert abs(float(r["train_loss"] - r["loss"])) <= 2e-6 * abs(float(r["loss"])) and torch.equal(r["train_v_rgb"], r["v_rgb"])
        for i, b in enumerate(ref[2]):
            assert torch.allclose(r[f"v_grid{i}"], b, rtol=1e-5, atol=1e-9)
            assert torch.allclose(r[f"train_acc{i}"] - pre0[i].cuda(), r[f"v_grid{i}"], rtol=1e-4, atol=5e-7)
    return SimpleNamespace(run=run, check=check)


case("photometric_tv_no_grid")(functools.partial(_photometric_case, 0))
case("photometric_tv_two_grids")(functools.partial(_photometric_case, 2))


# ===================================================================================================================================
# pvg.time_transform, nodes.pose_transform, deform.deform
# ===================================================================================================================================
def _np_results(prefix, d):
    return {f"{prefix}_{k}": torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


def _pvg_case(N, what):
    from oracle import gs_oracle
    from bilateral_driving_amd import pvg as P
    from tests import pvg_ref64 as PR
    from tests.test_gpu_37_pvg import compare, fused
    d = PR.random_rows(N, 100 + N, spread={"mixed": (0.03, 0.4), "all": (5.0, 6.0), "none": (1e-4, 2e-4)}[what])
    if what == "none":
        d["taus"] += 10.0
    setting = PR.SETTINGS[1]
    PR.settle_clamp(d, setting, 3)
    ref = PR.run_framework(d, setting, 3, sh=gs_oracle.spherical_harmonics)
    bound, _ = PR.measured_bound(d, setting, 3, ref)
    kept = int(ref[1].sum())
    assert kept == {"all": N, "none": 0}.get(what, kept)

    def run():
        o, m, g = fused(P, d, setting, 3)
        return dict(_np_results("out", o), mask=torch.from_numpy(m), **_np_results("grad", g))

    def check(r):      # tests/test_gpu_37_pvg.py compare(): the measured float32 bound of tests/pvg_ref64.py
        got = ({k: r["out_" + k].numpy() for k in PR.OUTS}, r["mask"].numpy(), {k: r["grad_" + k].numpy() for k in PR.RAW})
        compare(got, ref, bound)
    return SimpleNamespace(run=run, check=check)


for _n in (1, 257):
    case(f"pvg_time_transform_N{_n}", deterministic=True)(functools.partial(_pvg_case, _n, "mixed"))      # (test_two_runs_are_bit_identical)
case("pvg_time_transform_every_row_kept", deterministic=True)(functools.partial(_pvg_case, 257, "all"))
case("pvg_time_transform_every_row_dropped", deterministic=True)(functools.partial(_pvg_case, 257, "none"))


def _node_pose_case(N):
    from bilateral_driving_amd import nodes as Nd
    from tests.node_pose_ref64 import INPUTS, grads64, rel
    from tests.test_gpu_36_node_pose import fused, on, random_case
    d = random_case(N, 7)
    f = 3
    r_outs, r_g = grads64(on(d, "cpu", torch.float64), f)

    def run():
        outs, g = fused(Nd, on(d), f)
        return dict(wm=outs[0].detach(), wq=outs[1].detach(), op=outs[2].detach(), **{"grad_" + k: v for k, v in g.items()})

    def check(r):      # tests/test_gpu_36_node_pose.py test_fused_matches_float64
        for k, want in zip(("wm", "wq", "op"), r_outs):
            np.testing.assert_allclose(r[k].cpu().numpy(), want, rtol=1e-5, atol=1e-5)
        for k in INPUTS:
            gk = r["grad_" + k].cpu().numpy()
            assert gk.shape == r_g[k].shape and rel(r_g[k], gk) < (1e-4 if k.startswith("instances") else 1e-5), k
    return SimpleNamespace(run=run, check=check)


for _n in (1, 257):
    case(f"node_pose_transform_N{_n}", deterministic=True)(functools.partial(_node_pose_case, _n))      # (test_instance_gradients_are_deterministic)


def _deform_case(N):
    from bilateral_driving_amd import deform as D
    from tests import test_gpu_35_deform_network as T35
    m = T35.make(D, "cond", True, True).cuda()
    sd = T35.seeded_state(m, 11)
    m.load_state_dict(sd, strict=True)
    x, t, c = T35.inputs(N, 16, seed=N)
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(N, k, generator=g).cuda() for k in (3, 4, 3)]
    ref_outs, ref = T35.grads64({k: v.double().cuda() for k, v in sd.items()}, x, t, c, ws)

    def run():
        outs, got = T35.run(m, x, t, c, (True, True, True), ws)
        return dict({f"out{i}": o.detach() for i, o in enumerate(outs)}, **{"grad_" + k: v.detach().clone() for k, v in got.items()})

    def check(r):      # tests/test_gpu_35_deform_network.py test_against_float64 (up to 33 points: everything at 1e-4)
        for i, want in enumerate(ref_outs):
            torch.testing.assert_close(r[f"out{i}"].double(), want, rtol=1e-4, atol=2e-5)
        for k, v in r.items():
            if k.startswith("grad_"):
                want = ref[k[5:]]
                if float(want.norm()) == 0.0:
                    assert float(v.abs().max()) == 0.0, k
                else:
                    assert T35.rel(v, want) < (1e-4 if N < 1000 else (T35.PARAM_TOL if k[5:] in sd else T35.DATA_TOL)), k
    return SimpleNamespace(run=run, check=check)


for _n in (1, 257):
    case(f"deform_N{_n}", deterministic=True)(functools.partial(_deform_case, _n))      # (tests/test_gpu_35 test_deterministic)


# ===================================================================================================================================
# metrics.image_metrics, geometry
# ===================================================================================================================================
def _image_metrics_case(H, W):
    """Four mask slots: the inverted sky mask, the dynamic mask, an EMPTY mask and a FULL one."""
    from bilateral_driving_amd import metrics as M
    from tests import metrics_ref64 as R
    pred, gt = R.make_images(H, W, "noise")
    m = R.make_masks(H, W)
    score = {"occupied": ~m["sky_masks"], "masked": m["dynamic_masks"], "full": np.ones((H, W), bool)}
    r64, r32 = R.frame(pred, gt, score, np.float64), R.frame(pred, gt, score, np.float32)
    dev = lambda a: torch.as_tensor(a).cuda()

    def run():
        named = {"occupied": dev(m["sky_masks"]), "masked": dev(m["dynamic_masks"]), "none": dev(np.zeros((H, W), bool)), "full": dev(np.ones((H, W), bool))}
        return dict(M.image_metrics(dev(pred), dev(gt), named, return_map=True, invert=("occupied",)))

    def check(r):      # tests/test_gpu_39_image_metrics.py: twice the float32 restatement's own error + 1e-6 (metrics_ref64.bound)
        bound, _ = R.bound(r64, r32, "ssim_map")
        assert float(np.abs(r["ssim_map"].cpu().numpy().astype(np.float64) - r64["ssim_map"]).max()) <= bound
        for k in ("psnr", "ssim") + tuple(f"{p}_{q}" for p in score for q in ("psnr", "ssim")):
            bound, _ = R.bound(r64, r32, k)
            assert abs(float(r[k]) - r64[k]) <= bound, (k, float(r[k]), r64[k], bound)
        assert float(r["none_valid"]) == 0.0 and math.isnan(float(r["none_psnr"])) and math.isnan(float(r["none_ssim"]))
        assert all(float(r[f"{p}_valid"]) == 1.0 for p in score)
        assert abs(float(r["full_psnr"]) - float(r["psnr"])) <= 1e-9
    return SimpleNamespace(run=run, check=check)


case("image_metrics_11x11", deterministic=True)(functools.partial(_image_metrics_case, 11, 11))      # (test_two_calls_give_bit_equal_outputs)
case("image_metrics_33x19", deterministic=True)(functools.partial(_image_metrics_case, 33, 19))


@case("geometry_metrics_absent_class", deterministic=True)      # (tests/test_gpu_40 test_two_runs_of_a_frame_give_bit_equal_rows)
def _geometry_metrics_case():
    from bilateral_driving_amd import geometry as Gm
    from tests import geometry_ref64 as R
    from tests.test_gpu_40_geometry import run as run_frame
    inp, r64, r32 = R.case("absent_vehicle")
    n = r64["valid"]

    def run():
        return dict(run_frame(Gm, inp, return_distances=True))

    def check(r):      # tests/test_gpu_40_geometry.py test_scalars_and_distances_match_float64_within_the_float32_restatements_error
        assert float(r["valid"]) == n and all(float(r[f"{c}_valid"]) == r64[f"{c}_valid"] for c in R.CLASSES)
        vals = {k: float(r[k]) for k in R.SCALARS}
        vals["dist_pred"], vals["dist_gt"] = (r[k][:n].cpu().numpy() for k in ("dist_pred", "dist_gt"))
        for k in R.SCALARS + ("dist_pred", "dist_gt"):
            bound, _ = R.bound(r64, r32, k)
            assert R.error(vals[k], r64, k) <= bound, (k, vals[k], r64[k], bound)
        assert float(r["vehicle_valid"]) == 0 and math.isnan(float(r["chamfer_vehicle"]))
    # geometry.geometry_metrics: "``dist_pred`` / ``dist_gt``: [H*W] float32 arrays whose first n entries are the squared distance of
    # every pred point to its nearest lidar point, and the converse" -- the entries behind n are not part of the result
    behind_n = lambda r: (torch.arange(r["dist_pred"].numel(), device="cuda") >= n)
    return SimpleNamespace(run=run, check=check, masks={"dist_pred": behind_n, "dist_gt": behind_n})


@case("chamfer_distance_one_point_on_one_side")
def _chamfer_case():
    from bilateral_driving_amd import geometry as Gm
    from tests import geometry_ref64 as R
    g = np.random.default_rng(2)
    x, y = g.uniform(-20, 20, (1, 3)).astype(np.float32), g.uniform(-20, 20, (700, 3)).astype(np.float32)

    def run():
        out = {}
        for norm in (2, 1):
            out[f"x_norm{norm}"], out[f"y_norm{norm}"] = Gm.chamfer_distance(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), norm=norm)
        return out

    def check(r):      # tests/test_gpu_40_geometry.py test_chamfer_distance_between_clouds_of_different_sizes
        for norm in (2, 1):
            for got, a, b in ((r[f"x_norm{norm}"], x, y), (r[f"y_norm{norm}"], y, x)):
                w64, w32 = R.nearest(a.astype(np.float64), b.astype(np.float64), norm), R.nearest(a, b, norm)
                assert got.shape == (len(a),) and np.abs(got.cpu().numpy() - w64).max() <= 2 * np.abs(w32 - w64).max() + R.FLOOR
    return SimpleNamespace(run=run, check=check)


@case("depth_map_to_point_cloud")
def _point_cloud_case():
    from bilateral_driving_amd import geometry as Gm
    from tests import geometry_ref64 as R
    H, W = 17, 23
    K, c2w = R.camera(H, W)
    depth = np.random.default_rng(5).uniform(0.5, 79.0, (H, W)).astype(np.float32)
    mask = np.random.default_rng(6).uniform(0, 1, (H, W)) < 0.4
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()

    def run():
        return dict(all=Gm.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w)), masked=Gm.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), dev(mask)),
                    none=Gm.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), dev(np.zeros((H, W), bool))))

    def check(r):      # tests/test_gpu_40_geometry.py test_depth_map_to_point_cloud_is_row_major_and_masked
        for k, m in (("all", np.ones((H, W), bool)), ("masked", mask)):
            want = R.unproject(depth, K, c2w, m, np.float64)
            assert r[k].shape == want.shape and np.abs(r[k].cpu().numpy() - want).max() <= 4 * np.finfo(np.float32).eps * (np.abs(want).max() + 160)
        assert r["none"].shape == (0, 3)
    return SimpleNamespace(run=run, check=check)


# ===================================================================================================================================
# bilagrid
# ===================================================================================================================================
PYRAMID = [(2, 2, 1), (4, 4, 2), (8, 8, 4), (16, 16, 8)]


def _bilagrid_transform_case(form):
    """One case per dispatch form of bds_bilagrid_ms_fwd, named by the kernels ``bds_bilagrid_kernel_names`` reports; the sky blend on.
    K = 2 neighbour grids per level in the general form, the only one that takes them (csrc/bilagrid_ms.h cells_level_ok: the
    cell-aligned and the tile kernels are built for n_avg == 1, the training branch)."""
    import bilateral_driving_amd.bilagrid as B
    from bilateral_driving_amd import _lib as L
    levels, factors, H, W, cells, K, expect = {
        "tile_forward": (PYRAMID, [8, 4, 4, 2], 16, 32, 3, 1, ("ms_tile_fwd_kernel",)),                    # every factor divides the size
        "two_stage": (PYRAMID, [8, 4, 4, 2], 17, 35, 3, 1, ("cell_fwd_kernel<false", "ms_apply_fwd_kernel")),   # ... none does
        "cell_kernels": ([(1, 1, 1)], [1], 17, 35, 1, 1, ("cell_fwd_kernel<true",)),
        "general_kernels": (PYRAMID, [8, 4, 4, 2], 17, 35, 0, 2, ("ms_lowres_fwd_kernel", "ms_apply_fwd_kernel")),
    }[form]
    g = torch.Generator().manual_seed(H * 7919 + W)
    rgb = torch.rand(H, W, 3, generator=g) * 1.3 - 0.1
    alpha, sky = torch.rand(H, W, generator=g), torch.rand(H, W, 3, generator=g)
    ident = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    grids = [ident.reshape(1, 12, 1, 1, 1).repeat(K, 1, gl, gy, gx) + 0.05 * torch.randn(K, 12, gl, gy, gx, generator=g) for gx, gy, gl in levels]
    wt = torch.randn(H, W, 3, generator=g)
    r64, a64, s64 = (t.double().requires_grad_(True) for t in (rgb, alpha, sky))
    g64 = [x.double().requires_grad_(True) for x in grids]
    ref = BO.multiscale_transform(g64, BO.sky_blend(r64, a64[..., None], s64), factors, neighbours=True)
    (ref * wt.double()).sum().backward()

    def run():
        L.set_option(L.OPT_CELLS, cells)
        try:
            rg, ag, sg = _cuda(rgb, True), _cuda(alpha, True), _cuda(sky, True)
            gg = [_cuda(x, True) for x in grids]
            names = ",".join(L.bilagrid_kernel_names(B._levels_struct(gg, None, factors), H, W, False))
            assert all(e in names for e in expect), (form, names)
            out = B.bilagrid_transform(rg, gg, factors, alpha=ag, sky=sg)
            (out * wt.cuda()).sum().backward()
            torch.cuda.synchronize()
            return dict(out=out.detach(), v_rgb=rg.grad, v_alpha=ag.grad, v_sky=sg.grad, **{f"v_grid{i}": x.grad for i, x in enumerate(gg)})
        finally:
            L.set_option(L.OPT_CELLS, 3)

    def check(r):      # tests/test_gpu_16_bilagrid_cells.py test_single_scale_one_launch_vs_oracle: 1e-4 / 1e-3
        nrm = lambda got, want: float((got.cpu().double() - want).norm() / want.norm())
        assert rel_err(r["out"].cpu(), ref.detach()) < 1e-4
        assert max(nrm(r["v_rgb"], r64.grad), nrm(r["v_alpha"], a64.grad), nrm(r["v_sky"], s64.grad)) < 1e-3
        assert max(nrm(r[f"v_grid{i}"], x.grad) for i, x in enumerate(g64)) < 1e-3
    return SimpleNamespace(run=run, check=check)


for _form in ("tile_forward", "two_stage", "cell_kernels", "general_kernels"):
    case(f"bilagrid_transform_{_form}")(functools.partial(_bilagrid_transform_case, _form))


def _slice_image_case(H, W):
    """bilagrid._SliceImage (the band of the grid staged in LDS) against the point form on the same values."""
    from bilateral_driving_amd.bilagrid import _SliceImage, _SlicePoints
    nc, gx, gy, gl = 8, 16, 16, 8
    g = torch.Generator().manual_seed(H * 7 + W)
    grid0 = torch.randn(nc, gl, gy, gx, generator=g)
    rgb0 = torch.rand(H, W, 3, generator=g) * 1.3 - 0.15
    v = torch.randn(H, W, nc, generator=g).cuda()
    grid, rgb = _cuda(grid0, True), _cuda(rgb0, True)
    ys, xs = torch.meshgrid(torch.linspace(0, 1.0, H, device="cuda"), torch.linspace(0, 1.0, W, device="cuda"), indexing="ij")
    xy = torch.stack([xs, ys], dim=-1).reshape(-1, 2)
    ref = _SlicePoints.apply(grid, xy, rgb.reshape(-1, 3)).reshape(H, W, nc)
    (ref * v).sum().backward()
    want = (ref.detach().clone(), grid.grad.clone(), rgb.grad.clone())

    def run():
        grid, rgb = _cuda(grid0, True), _cuda(rgb0, True)
        out = _SliceImage.apply(grid, rgb)
        (out * v).sum().backward()
        pts = _SlicePoints.apply(_cuda(grid0), xy, _cuda(rgb0).reshape(-1, 3))
        return dict(out=out.detach(), v_grid=grid.grad, v_rgb=rgb.grad, points_out=pts.reshape(H, W, nc))

    def check(r):      # tests/test_gpu_12_neural_modules.py test_image_slice_equals_point_slice
        assert torch.equal(r["out"], want[0]) and torch.equal(r["points_out"], want[0])
        torch.testing.assert_close(r["v_rgb"], want[2], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(r["v_grid"], want[1], rtol=0, atol=2e-5 * float(want[1].abs().max()))
    return SimpleNamespace(run=run, check=check)


case("bilagrid_slice_image_1x300")(functools.partial(_slice_image_case, 1, 300))
case("bilagrid_slice_image_33x65")(functools.partial(_slice_image_case, 33, 65))


def _slice_points_case(P):
    """bilagrid.slice (12-channel grids -> affine maps + colours) and slice_feature (feature grids) at P points, against the oracle's
    slice in float64."""
    from bilateral_driving_amd.bilagrid import BilateralGrid, NeuralBilateralGrid, slice, slice_feature
    g = torch.Generator().manual_seed(P)
    xy0, rgb0 = torch.rand(P, 2, generator=g), torch.rand(P, 3, generator=g) * 1.2 - 0.1
    idx = torch.full((P, 1), 1, dtype=torch.long)
    bg, ng = BilateralGrid(3, 5, 7, 3).cuda(), NeuralBilateralGrid(3, 5, 7, 3, feature_dim=8).cuda()
    with torch.no_grad():
        bg.grids.add_((0.05 * torch.randn(bg.grids.shape, generator=g)).cuda())
        ng.grids.copy_(torch.randn(ng.grids.shape, generator=g).cuda())
    wa, wf = torch.randn(P, 3, generator=g), torch.randn(P, 8, generator=g)
    r64, rf64 = rgb0.double().requires_grad_(True), rgb0.double().requires_grad_(True)
    gb64, gn64 = bg.grids.detach().cpu().double().requires_grad_(True), ng.grids.detach().cpu().double().requires_grad_(True)
    aff = BO.slice_grid(gb64[1], xy0[:, 0].double(), xy0[:, 1].double(), BO.rgb2gray(r64))
    out64 = BO.apply_affine(aff, r64)
    feat64 = BO.slice_grid(gn64[1], xy0[:, 0].double(), xy0[:, 1].double(), BO.rgb2gray(rf64))
    ((out64 * wa.double()).sum() + (feat64 * wf.double()).sum()).backward()

    def run():
        bg.zero_grad(set_to_none=True); ng.zero_grad(set_to_none=True)
        rgb, rgb_f = _cuda(rgb0, True), _cuda(rgb0, True)      # (one leaf per op: each op's colour gradient at its own test's bound)
        a = slice(bg, xy0.cuda(), rgb, idx.cuda())
        f = slice_feature(ng, xy0.cuda(), rgb_f, idx.cuda())["affine_features"]
        ((a["rgb"] * wa.cuda()).sum() + (f.reshape(P, 8) * wf.cuda()).sum()).backward()
        return dict(rgb=a["rgb"].detach(), mats=a["rgb_affine_mats"].detach(), feats=f.detach().reshape(P, 8), v_rgb=rgb.grad, v_rgb_feature=rgb_f.grad,
                    v_grids=bg.grids.grad.clone(), v_feature_grids=ng.grids.grad.clone())

    def check(r):
        # tests/test_gpu_00_bilagrid_parity.py test_slice_api_vs_reference_golden: TOL on the maps and colours, v_rgb rtol 2e-3 / atol 2e-4,
        # the grids' gradient 2e-4 of max(1, largest entry); test_feature_grid_slice_matches_reference_goldens: 2e-5 / 5e-5 (rel_err)
        cpu = lambda t: t.detach().cpu().double().numpy()
        np.testing.assert_allclose(cpu(r["mats"]).reshape(P, 12), aff.detach().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(cpu(r["rgb"]), out64.detach().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(cpu(r["v_rgb"]), r64.grad.numpy(), rtol=2e-3, atol=2e-4)
        want = gb64.grad.numpy()
        assert np.abs(cpu(r["v_grids"]) - want).max() < 2e-4 * max(1.0, np.abs(want).max())
        assert rel_err(r["feats"].cpu(), feat64.detach()) < 2e-5
        assert rel_err(r["v_feature_grids"].cpu(), gn64.grad) < 5e-5 and rel_err(r["v_rgb_feature"].cpu(), rf64.grad) < 5e-5
        assert float(r["v_grids"][0].abs().max()) == 0.0 and float(r["v_feature_grids"][2].abs().max()) == 0.0      # only image 1's grid
    return SimpleNamespace(run=run, check=check)


case("bilagrid_slice_P1")(functools.partial(_slice_points_case, 1))
case("bilagrid_slice_P65")(functools.partial(_slice_points_case, 65))


@case("bilagrid_total_variation_loss")
def _tv_case():
    from bilateral_driving_amd.bilagrid import total_variation_loss
    g = torch.Generator().manual_seed(4)
    grids = [torch.randn(3, 12, gl, gy, gx, generator=g) for gx, gy, gl in PYRAMID + [(1, 1, 1)]]
    g64 = [x.double().requires_grad_(True) for x in grids]
    ref = [BO.total_variation_loss(x) for x in g64]
    sum(ref).backward()

    def run():
        gg = [_cuda(x, True) for x in grids]
        tv = [total_variation_loss(x) for x in gg]
        sum(tv).backward()
        return dict(**{f"tv{i}": t.detach().reshape(1) for i, t in enumerate(tv)}, **{f"v_grid{i}": x.grad for i, x in enumerate(gg)})

    def check(r):      # tests/test_gpu_00_bilagrid_parity.py test_tv_vs_reference_golden: value rtol 1e-4, gradient rtol 1e-3 / atol 1e-6
        for i, (t, x) in enumerate(zip(ref, g64)):
            np.testing.assert_allclose(float(r[f"tv{i}"]), float(torch.as_tensor(t).detach()), rtol=1e-4)
            if x.grad is not None and float(x.grad.abs().max()) > 0:
                np.testing.assert_allclose(r[f"v_grid{i}"].cpu().numpy(), x.grad.numpy(), rtol=1e-3, atol=1e-6)
            else:
                assert float(r[f"v_grid{i}"].abs().max()) == 0.0, i
    return SimpleNamespace(run=run, check=check, zero_filled_only=True)      # (_TotalVariation: torch.zeros for the value and the gradient)


# ===================================================================================================================================
# mlp_head
# ===================================================================================================================================
def _mlp_head_case(P, F, maps_only=False):
    from bilateral_driving_amd import mlp_head
    from tests.test_gpu_12_neural_modules import _head_inputs, _rel, _torch_head
    residual = P % 2 == 1
    base = [t.detach().cpu() for t in _head_inputs(P, F, seed=P + F)]
    ref_in = [t.double().requires_grad_(True) for t in base[:5]]
    r_out, r_aff = _torch_head(*ref_in, residual)
    ((0 if maps_only else (r_out * base[5].double()).sum()) + (r_aff * base[6].double()).sum()).backward()

    def run():
        feats, rgb, w1, w2, w3 = (_cuda(t, True) for t in base[:5])
        v_out, v_aff = base[5].cuda(), base[6].cuda()
        if maps_only:
            out, aff = None, mlp_head.affine_maps(feats, w1, w2, w3)
            (aff * v_aff).sum().backward()
        else:
            out, aff = mlp_head.transform_and_maps(feats, rgb, w1, w2, w3, residual=residual)
            ((out * v_out).sum() + (aff * v_aff).sum()).backward()
        return dict(out=None if out is None else out.detach(), aff=aff.detach(), v_feats=feats.grad, v_rgb=rgb.grad, v_w1=w1.grad, v_w2=w2.grad, v_w3=w3.grad)

    def check(r):      # tests/test_gpu_12_neural_modules.py test_fused_head_equals_framework_modules / _single_outputs_and_saturation
        if not maps_only:
            assert _rel(r["out"].cpu().double(), r_out.detach()) < 2e-6
            torch.testing.assert_close(r["out"].cpu().double(), r_out.detach(), rtol=1e-4, atol=2e-5)
        assert _rel(r["aff"].cpu().double(), r_aff.detach()) < 2e-6
        torch.testing.assert_close(r["aff"].cpu().double(), r_aff.detach(), rtol=1e-4, atol=2e-5)
        for name, want in zip(("feats", "rgb", "w1", "w2", "w3"), ref_in):
            got = r["v_" + name]
            if maps_only and name == "rgb":
                assert got is None      # the maps alone do not depend on the colour
                continue
            tol = 3e-5 if (name.startswith("w") or maps_only) else 3e-6
            assert _rel(got.cpu().double(), want.grad) < tol, (name, _rel(got.cpu().double(), want.grad))
    return SimpleNamespace(run=run, check=check)


for _p in (1, 31, 33, 2049):
    for _f in (8, 32):
        case(f"mlp_head_transform_and_maps_P{_p}_F{_f}", deterministic=True)(functools.partial(_mlp_head_case, _p, _f))      # ("no atomics anywhere")
case("mlp_head_affine_maps_P33_F8", deterministic=True)(functools.partial(_mlp_head_case, 33, 8, True))


def _image_transform_case(kind, H, W):
    """mlp_head.image_transform through the modules' ``transform`` against the two-step path (feature slice, then the head)."""
    from bilateral_driving_amd import mlp_head
    from bilateral_driving_amd.modules import MultiScaleNeuralBilateralAffineTransform, NeuralBilateralAffineTransform
    from tests.test_gpu_12_neural_modules import _randomise, _two_step
    if kind == "ms":
        mod = MultiScaleNeuralBilateralAffineTransform("Affine", 3, [[1, 1, 1], [16, 16, 8]], feature_dim=8, hidden_dim=64)
        levels = [mod.bil_grids0, mod.bil_grids1]
    else:
        mod = NeuralBilateralAffineTransform("Affine", 3, 16, 16, 8, feature_dim=24, hidden_dim=64)
        levels = [mod.bil_grids]
    _randomise(mod, H + W)
    assert mlp_head.image_supported(H, W, [g.grids[0] for g in levels], 64)
    g = torch.Generator().manual_seed(W)
    rgb0 = torch.rand(H, W, 3, generator=g) * 1.2 - 0.1
    v = torch.randn(H, W, 3, generator=g).cuda()
    infos = {"img_idx": 1}
    rgb = _cuda(rgb0, True)
    ref = _two_step(mod, rgb, infos)
    (ref * v).sum().backward()
    want = {n: p.grad.clone() for n, p in mod.named_parameters()}
    want["rgb"] = rgb.grad.clone()
    ref = ref.detach().clone()

    def run():
        mod.zero_grad(set_to_none=True)
        rgb = _cuda(rgb0, True)
        out = mod.transform(rgb, infos)
        (out * v).sum().backward()
        return dict(out=out.detach(), v_rgb=rgb.grad, **{"v_" + n: p.grad.clone() for n, p in mod.named_parameters()})

    def check(r):      # tests/test_gpu_12_neural_modules.py test_fused_image_transform_equals_two_step_path
        torch.testing.assert_close(r["out"], ref, rtol=1e-4, atol=5e-5)
        for n, w in want.items():
            torch.testing.assert_close(r["v_" + n], w, rtol=0, atol=2e-4 * float(w.abs().max()) + 1e-7, msg=lambda m, n=n: f"{n}: {m}")
            if "grids" in n:
                assert float(r["v_" + n][0].abs().max()) == 0.0 and float(r["v_" + n][2].abs().max()) == 0.0
    return SimpleNamespace(run=run, check=check)


case("mlp_head_image_transform_1x20")(functools.partial(_image_transform_case, "single24", 1, 20))
case("mlp_head_image_transform_5x7")(functools.partial(_image_transform_case, "single24", 5, 7))
case("mlp_head_image_transform_two_level_75x130")(functools.partial(_image_transform_case, "ms", 75, 130))


# ===================================================================================================================================
# colorcorrect, densify, optim.DensifyStats, init
# ===================================================================================================================================
@case("color_correct_smallest_golden")
def _color_correct_case():
    import glob
    from bilateral_driving_amd.colorcorrect import color_correct
    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "color_correct_*.npz")), key=lambda f: np.load(f)["img"].size)
    z = np.load(files[0])

    def run():
        return dict(out=color_correct(torch.from_numpy(z["img"]).float().cuda(), torch.from_numpy(z["ref"]).float().cuda(), int(z["num_iters"])))

    def check(r):      # tests/test_gpu_14_color_correct.py test_equals_reference_golden
        np.testing.assert_allclose(r["out"].cpu().numpy(), z["out_f64"], atol=2e-5)
        np.testing.assert_allclose(r["out"].cpu().numpy(), z["out_f32"], atol=2e-5)
    return SimpleNamespace(run=run, check=check)


def _refine_inputs(N, quiet):
    """tests/test_gpu_11_refine.py synthetic(); ``quiet``: a step at which nothing splits, duplicates or is pruned."""
    from tests.test_gpu_11_refine import synthetic
    P, M, V, stats = synthetic(N, seed=N + 3300)
    if quiet:
        P["_scales"] = np.full_like(P["_scales"], math.log(0.01))
        P["_opacities"] = np.full_like(P["_opacities"], 2.0)
        stats["xys_grad_norm"] = np.zeros_like(stats["xys_grad_norm"])
        stats["max_2Dsize"] = np.zeros_like(stats["max_2Dsize"])
    return P, M, V, stats


def _refinement_case(N, quiet):
    from oracle import refine_oracle as RO
    from bilateral_driving_amd.densify import plan, refinement_after
    from tests.test_gpu_11_refine import CTRL, build_model, check as check_model
    step = 3300
    P, M, V, stats = _refine_inputs(N, quiet)
    sch = RO.schedule(step, CTRL, 30.0, 150)
    n_split = int(RO.plan(sch, CTRL, P["_scales"], P["_opacities"], stats["xys_grad_norm"], stats["vis_counts"], stats["max_2Dsize"])[0].sum())
    samples = np.random.default_rng(1).standard_normal((2 * n_split, 3)).astype(np.float32)
    eP, eM, eV, ns = RO.refine(step, CTRL, 30.0, 150, P, M, V, stats["xys_grad_norm"], stats["vis_counts"], stats["max_2Dsize"], samples)
    assert ns == n_split and (not quiet or (n_split == 0 and eP["_means"].shape[0] == N))
    box = {}

    def run():
        t = lambda a: torch.from_numpy(a).cuda()
        flags, ranks, totals = plan(t(P["_scales"]), t(P["_opacities"]), t(stats["xys_grad_norm"]), t(stats["vis_counts"]), t(stats["max_2Dsize"]),
                                    do_densify=True, grad_thresh=0.0003, size_thresh=0.06, split_by_screen=True, split_screen_size=0.05,
                                    do_cull=True, cull_alpha_thresh=0.005, cull_by_scale=True, cull_scale_thresh=15.0, cull_by_screen=True,
                                    cull_screen_size=0.15)
        model, opt = build_model(P, M, V, dict(stats), CTRL, 30.0, 150, step, torch.optim.Adam)
        refinement_after(model, step, opt, samples=torch.from_numpy(samples), verbose=False)
        box["model"], box["opt"] = model, opt
        out = dict(flags=flags, ranks=ranks, totals=totals)
        for a in RO.PARAMS:
            prm = getattr(model, a)
            out["new" + a], out["m" + a], out["v" + a] = prm.detach(), opt.state[prm]["exp_avg"], opt.state[prm]["exp_avg_sq"]
        return out

    def check(r):      # tests/test_gpu_11_refine.py: test_plan_counts_and_ranks_are_exclusive_scans, test_refinement_equals_oracle_at_scale
        f = r["flags"].cpu().numpy(); rk = r["ranks"].cpu().numpy().astype(np.int64); tot = r["totals"].cpu().numpy()
        for k, bit in enumerate((0, 2, 3, 4)):
            m = (f >> bit) & 1
            np.testing.assert_array_equal(rk[:, k], np.cumsum(m) - m)
        np.testing.assert_array_equal(tot, [int(((f >> b) & 1).sum()) for b in range(5)])
        check_model(box["model"], box["opt"], eP, eM, eV, means_atol=5e-5)
    return SimpleNamespace(run=run, check=check)


for _n in (1, 300):
    case(f"densify_plan_and_refinement_N{_n}")(functools.partial(_refinement_case, _n, False))
case("densify_plan_and_refinement_quiet_step")(functools.partial(_refinement_case, 300, True))


@case("densify_out_of_bound_mask_and_stats")
def _oob_and_stats_case():
    """densify.out_of_bound_mask against the reference's expression, optim.DensifyStats.update against the golden of the reference's
    own method (tests/golden/densify_stats.npz)."""
    from bilateral_driving_amd.densify import out_of_bound_mask
    from bilateral_driving_amd.optim import DensifyStats
    g = torch.Generator().manual_seed(3)
    N, I = 300, 11
    means = (torch.rand(N, 3, generator=g) - 0.5) * 40
    ids = torch.randint(0, I, (N, 1), generator=g)
    sizes = torch.rand(I, 3, generator=g) * 30 + 8
    ref = (means.abs() > sizes[ids[..., 0]] / 2).any(dim=-1)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "densify_stats.npz"))
    Ng, W, H = int(z["N"]), int(z["W"]), int(z["H"])

    def run():
        out = dict(mask=out_of_bound_mask(means.cuda(), ids.cuda(), sizes.cuda()))
        st = DensifyStats(Ng, "cuda", batch_size=int(z["batch"]))
        for call in range(3):
            m2 = torch.zeros(1, Ng, 2, device="cuda")
            m2.absgrad = torch.from_numpy(z[f"absgrad{call}"]).cuda()
            st.update({"means2d": m2, "radii": torch.from_numpy(z[f"radii{call}"]).cuda()[None], "width": W, "height": H})
            for name in ("xys_grad_norm", "vis_counts", "max_2Dsize"):
                out[f"{name}{call}"] = getattr(st, name).clone()
        return out

    def check(r):      # tests/test_gpu_11_refine.py test_out_of_bound_mask_matches_reference_expression; tests/test_gpu_10_optim.py (rtol 2e-7)
        assert r["mask"].dtype == torch.uint8 and torch.equal(r["mask"].bool().cpu(), ref) and 0 < int(ref.sum()) < N
        for call in range(3):
            for name in ("xys_grad_norm", "vis_counts", "max_2Dsize"):
                assert torch.allclose(r[f"{name}{call}"].cpu(), torch.from_numpy(z[f"{name}{call}"]), rtol=2e-7, atol=0), (call, name)
    return SimpleNamespace(run=run, check=check)


def _knn_case(n):
    from bilateral_driving_amd import init as I
    from tests import knn_ref64 as R
    from tests.test_gpu_41_knn_init import DIST_RTOL, SCALE_FLOOR, pair_f32
    k = 3
    x = np.random.default_rng(n).uniform(0.0, 100.0, (n, 3)).astype(np.float32)
    d64, _ = R.knn(x, k)

    def run():
        dist, idx = I.k_nearest(torch.as_tensor(x).cuda(), k)
        return dict(dist=dist, idx=idx, scales=I.init_scales(torch.as_tensor(x).cuda(), k, 3), rigid_scales=I.rigid_init_scales(torch.as_tensor(x).cuda()))

    def check(r):      # tests/test_gpu_41_knn_init.py: test_every_case_matches_float64_at_every_point, test_init_scales_is_the_log_of_the_mean_distance
        d, i = r["dist"].cpu().numpy(), r["idx"].cpu().numpy()
        assert R.distance_error(d, d64) <= DIST_RTOL and np.all(np.diff(d, axis=1) >= 0)
        assert np.all(i != np.arange(n)[:, None]) and i.min() >= 0 and i.max() < n and all(len(set(row)) == k for row in i.tolist())
        assert np.array_equal(pair_f32(x, i).view(np.int32), d.view(np.int32))
        for key, clamp in (("scales", None), ("rigid_scales", (0.002, 100.0))):
            mean64 = d.astype(np.float64).mean(1)
            if clamp is not None:
                mean64 = np.clip(mean64, np.float64(np.float32(clamp[0])), np.float64(np.float32(clamp[1])))
            got = r[key].cpu().numpy()
            assert got.shape == (n, 3) and np.abs(got[:, 0].astype(np.float64) - np.log(mean64)).max() <= SCALE_FLOOR
            assert np.array_equal(got[:, 1], got[:, 0]) and np.array_equal(got[:, 2], got[:, 0])
    return SimpleNamespace(run=run, check=check)


case("init_k_nearest_n_equals_k_plus_1", deterministic=True)(functools.partial(_knn_case, 4))      # (test_result_does_not_depend_on_the_order)
case("init_k_nearest_n300", deterministic=True)(functools.partial(_knn_case, 300))


# ===================================================================================================================================
# lidar, pseudo_lidar (the golden shapes of tests/test_gpu_42_lidar_prep.py / tests/test_gpu_45_pseudo_lidar.py: their smallest)
# ===================================================================================================================================
@case("lidar_project_points", deterministic=True)      # (tests/test_gpu_42 test_projection_is_bit_identical_run_to_run_...)
def _lidar_project_case():
    from bilateral_driving_amd import lidar as LD
    from tests import lidar_ref64 as R
    from tests.test_gpu_42_lidar_prep import gpu_launch
    name = "sparse"
    case = R.golden_projection_case(name)
    box = {}

    def run():
        keep = []
        box["res"] = R.run_projection(case, gpu_launch(LD, keep))
        out = {}
        for i, (depth, winner, pix, vis, col) in enumerate(keep):
            out.update({f"depth{i}": depth, f"winner{i}": winner, f"pix{i}": pix, f"visible{i}": vis, f"colors{i}": col})
        T = len(case["sweep_times"])
        out["perm"], out["offsets"] = LD.group_by_timestep(torch.as_tensor(case["timesteps"]).cuda(), T)
        return out

    def check(r):      # tests/test_gpu_42_lidar_prep.py test_projection_equals_the_reference, test_group_by_timestep_...
        R.compare_projection_golden(name, box["res"])
        want_perm, want_off = R.grouped(case)
        assert np.array_equal(r["perm"].cpu().numpy(), want_perm) and np.array_equal(r["offsets"].cpu().numpy(), want_off)
    return SimpleNamespace(run=run, check=check)


@case("lidar_points_in_boxes_and_downsample", deterministic=True)      # (tests/test_gpu_42 test_boxes_equal_the_reference: ``again`` bit-equal)
def _lidar_boxes_case():
    from bilateral_driving_amd import lidar as LD
    from tests import lidar_ref64 as R
    from tests.test_gpu_42_lidar_prep import ulps
    z, case = R.golden(), R.golden_box_case()
    F = case["active"].shape[0]
    poses, sizes = torch.from_numpy(case["poses"]), torch.from_numpy(case["sizes"])
    fr = R.frame_ranges(case["timesteps"], F)
    eligible = R.eligible_of(case, "RigidNodes")
    inst = [int(i) for i in z["box_filter_instances"]]
    k, (Hd, Wd, factor) = 0, R.DEPTH_CASES[0]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()

    def run():
        x = dev(case["points"])
        rec = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(eligible), torch.from_numpy(fr), emit=True, chunk=3)
        inside = LD.points_in_boxes(x, poses, sizes, torch.from_numpy(case["active"]), instances=inst, chunk=3)
        none = LD.points_in_boxes(x, poses, sizes, torch.zeros_like(torch.from_numpy(case["active"])), emit=True, chunk=3)
        return dict(instance=rec["instance"], frame=rec["frame"], row=rec["row"], xyz=rec["xyz"], inside=inside, none_row=none["row"], none_xyz=none["xyz"],
                    down=LD.downsample_sparse_depth(dev(z[f"depth{k}_map"]), factor))

    def check(r):      # tests/test_gpu_42_lidar_prep.py test_boxes_equal_the_reference, test_downsampler_equals_the_reference
        ids = torch.stack([r["instance"], r["frame"], r["row"]], 1).cpu().numpy()
        R.compare_records(case, eligible, ids, r["xyz"].cpu().numpy(), exact=True)
        assert np.array_equal(r["inside"].cpu().numpy(), z["box_filter_inside"])
        assert r["none_row"].numel() == 0 and r["none_xyz"].shape == (0, 3)
        got, gold = r["down"].cpu().numpy(), z[f"depth{k}_out"]
        assert np.array_equal(got == 0, gold == 0) and ulps(got, gold).max() <= 4.0
        exact, n = R.downsample(z[f"depth{k}_map"], factor)
        assert np.all(np.abs(got - exact) <= (n + 4) * R.U * np.abs(exact) * 1.01)
    return SimpleNamespace(run=run, check=check)


@case("pseudo_lidar_depth_to_lidar_with_an_empty_camera")
def _pseudo_depth_case():
    from bilateral_driving_amd import pseudo_lidar as P
    from tests import pseudo_lidar_ref64 as R
    from tests.test_gpu_45_pseudo_lidar import golden_ref, run as run_batch
    z = R.golden()
    case, ref = golden_ref("front")
    empty = dict(case, depth=np.zeros_like(case["depth"]))      # a camera without a valid pixel, between two that have them

    def run():
        points, counts, source = run_batch(P, [case, empty, case])
        return dict(points=points, counts=counts, source=source)

    def check(r):      # tests/test_gpu_45_pseudo_lidar.py test_depth_cases_equal_the_reference
        assert r["counts"].tolist()[1] == 0
        for c in (0, 2):
            pts, n, src = r["points"][c].cpu().numpy(), int(r["counts"][c]), r["source"][c].cpu().numpy()
            assert n == len(z["front_source"]) and np.array_equal(src[:n], z["front_source"])
            R.compare(ref, pts, n, src, label="front")
            err = np.abs(pts[:n].astype(np.float64) - z["front_points"])
            assert np.all(err <= ref["e_dev"][src[:n]] + ref["e_ref"][src[:n]])
    # pseudo_lidar.depth_to_lidar: "rows [0, counts[c]) of camera c are its occupied beams in beam order, the rows behind them are not
    # written" (points and, with return_source, source alike: both are [C,cap,...] with the same rows)
    def behind(r):
        cap = r["source"].shape[1]
        return torch.arange(cap, device="cuda")[None, :] >= r["counts"][:, None].long()
    return SimpleNamespace(run=run, check=check, masks={"points": lambda r: behind(r)[..., None].expand_as(r["points"]), "source": behind})


@case("pseudo_lidar_cloud_to_lidar")
def _pseudo_cloud_case():
    from bilateral_driving_amd import pseudo_lidar as P
    from tests import pseudo_lidar_ref64 as R
    z, case = R.golden(), R.golden_cloud_case()

    def run():
        points, counts, source = P.cloud_to_lidar(torch.as_tensor(case["cloud"]).cuda(), case["H"], case["W"], case["slice"], "classic", crop=R.SPARSE_CROP,
                                                  return_source=True)
        return dict(points=points, counts=counts, source=source)

    def check(r):      # tests/test_gpu_45_pseudo_lidar.py test_cloud_case_equals_the_reference
        n = int(r["counts"][0])
        assert tuple(r["points"].shape) == (case["H"] * case["W"], 4) and n == len(z["cloud_source"])
        assert np.array_equal(r["source"][:n].cpu().numpy(), z["cloud_source"])
        assert np.array_equal(r["points"][:n].cpu().numpy().view(np.int32), z["cloud_out"].view(np.int32))
    # pseudo_lidar.cloud_to_lidar: "rows [0, counts[0]) are the occupied beams in beam order, the rows behind them are not written"
    behind = lambda r: torch.arange(r["source"].numel(), device="cuda") >= r["counts"][0].long()
    return SimpleNamespace(run=run, check=check, masks={"points": lambda r: behind(r)[:, None].expand_as(r["points"]), "source": behind})
