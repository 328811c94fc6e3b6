"""-m gpu: the 12-value wave64 transpose-reduce (csrc/bds_common.h butterfly_sum12) and its three callers.

* the helper itself on one wave (bds_reduce12_probe) against the 16-value form and the lane-by-lane model of tests/reduce12_model.py;
* the compositor's backward -- one-wave-per-tile, strip and deferred-epilogue kernels -- FIELD BY FIELD of the gradient record
  (colours per channel, conic a / b / c, mean x / y, absgrad x / y, opacity; depth = the last colour channel of the depth modes)
  against the float64 oracle at tests/test_gpu_01's gradient tolerance (1e-3 norm-relative), every reference column non-zero, so that
  a dropped or swapped slot cannot pass; the record's floats that no lane commits keep the value they held;
* the camera-pose gradient of the view backward (project.hip pose_grad_reduce): all 12 entries;
* the colour pyramid's general low-resolution backward (bilagrid.hip slice_grid_scatter): all 12 channels of the grid gradients;
* the resource report of the three backward compositors."""
import math

import numpy as np
import pytest
import torch

from oracle import bilagrid_oracle as BO
from oracle import gs_oracle as G
from tests import reduce12_model as M
from tests.util import kernel_resources, make_scene

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3          # tests/test_gpu_01_gs_parity.py: gradients 1e-3 norm-relative
POISON = 12345.0         # what the record floats no lane may write hold before the launch
FIELDS = {0: "colour 0", 1: "colour 1", 2: "colour 2", 3: "colour 3", 4: "conic a", 5: "conic b", 6: "conic c", 7: "mean x", 8: "mean y",
          9: "absgrad x", 10: "absgrad y", 11: "opacity"}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import bilateral_driving_amd.gs_ops as ops
    from bilateral_driving_amd import _lib as L
    L.lib()
    return ops, L


def _nrm(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())


# ---- the helper on one wave ---------------------------------------------------------------------------------------------------
def test_probe_equals_the_model_and_the_16_value_form(env):
    ops, L = env
    cases = M.inputs()
    v = torch.from_numpy(np.stack([c[1] for c in cases])).cuda()              # [n, 64, 12]
    out16, out12 = torch.full((len(cases), 64), POISON, device="cuda"), torch.full((len(cases), 64), POISON, device="cuda")
    lib, st = L.lib(), L.stream()
    for i in range(len(cases)):
        L.check(lib.bds_reduce12_probe(v[i].data_ptr(), out16[i].data_ptr(), out12[i].data_ptr(), st), "bds_reduce12_probe")
    torch.cuda.synchronize()
    got16, got12 = out16.cpu().numpy(), out12.cpu().numpy()
    for i, (name, vi) in enumerate(cases):
        M.check(vi, got16[i], got12[i])                                          # bit-equal totals in the documented lanes
        assert np.array_equal(got12[i].view(np.uint32), M.butterfly_sum12(vi).view(np.uint32)), name      # ... and the model's
        assert np.array_equal(got16[i].view(np.uint32), M.butterfly_sum16(M.pad16(vi)).view(np.uint32)), name
        if name.startswith("onehot"):
            k = int(name.split("_k")[1])
            assert np.array_equal(got12[i] != 0, M.SLOT12 == k), name            # the slot map
    committed = sorted(M.SLOT12[l] for l in M.COMMIT12_LANES)
    assert committed == list(range(12))


# ---- compositor backward, record by record ------------------------------------------------------------------------------------
_ORACLE = {}


def _scene_inputs(ops, N, W, H, CH, seed):
    sc = make_scene(N, W, H, seed=seed)
    with torch.no_grad():
        radii, m2, d, con, _ = ops.fully_fused_projection(sc["means"].cuda(), sc["quats"].cuda(), sc["scales"].cuda(), sc["viewmats"].cuda(),
                                                          sc["Ks"].cuda(), W, H)
    rgb = sc["colors"].cuda()
    col = {1: d[0][:, None], 3: rgb, 4: torch.cat([rgb, d[0][:, None]], -1)}[CH][None].contiguous()
    op = sc["opacities"].cuda()[None].contiguous()
    assert int((radii > 0).sum()) >= min(N, 4)
    return radii, m2.contiguous(), d.contiguous(), con.contiguous(), col, op


def _oracle_records(key, m2, con, col, op, W, H, lt, offs, fids, seed):
    """float64 oracle on the kernels' own inputs and lists -> (render, alphas, stable, weights, reference record [N,16]); computed once
    per scene and list form, shared by the absgrad on / off runs."""
    if key in _ORACLE:
        return _ORACLE[key]
    N, CH = m2.shape[1], col.shape[-1]
    lv = {k: t[0].detach().cpu().double().requires_grad_(True) for k, t in dict(m2=m2, con=con, col=col, op=op).items()}
    probe = []
    r, a, _, unstable = G.rasterize_to_pixels(lv["m2"], lv["con"], lv["col"], lv["op"], W, H, lt, offs[0].cpu(), fids.cpu().long(), None,
                                              return_unstable=True, absgrad_probe=probe)
    g = torch.Generator().manual_seed(100 + seed)
    wt = torch.randn(r.shape, generator=g) * (~unstable)[..., None]
    wa = torch.randn(a.shape, generator=g) * (~unstable)[..., None]
    ((r * wt.double()).sum() + (a * wa.double()).sum()).backward()
    ref = torch.zeros(N, 16, dtype=torch.float64)
    ref[:, 0:CH], ref[:, 4:7], ref[:, 7:9], ref[:, 11] = lv["col"].grad, lv["con"].grad, lv["m2"].grad, lv["op"].grad
    ref[:, 9:11] = G.absgrad_from_probe(probe, N)
    out = (r.detach(), a.detach(), ~unstable, wt, wa, ref)
    _ORACLE[key] = out
    return out


def _check_record(v_rec, ref, CH, absgrad, tag):
    got = v_rec.detach().cpu().double()
    written = list(range(CH)) + [4, 5, 6, 7, 8, 11] + ([9, 10] if absgrad else [])
    for k in range(16):
        if k in written:
            assert float(ref[:, k].norm()) > 0, (tag, FIELDS[k], "reference column is zero")
            e = _nrm(got[:, k], ref[:, k])
            print(f"[reduce12] {tag} absgrad={int(absgrad)} {FIELDS[k]}: norm-rel error {e:.2e}")
            assert e < GRAD_TOL, (tag, FIELDS[k], e)
        else:      # no lane commits this float: it keeps what it held
            assert bool((got[:, k] == POISON).all()), (tag, k, "a float of the record that no lane commits was written")


def _records_buffer(n, CH, absgrad):
    v_rec = torch.full((n, 16), POISON, device="cuda")
    v_rec[:, :CH] = 0.0
    v_rec[:, 4:9] = 0.0
    v_rec[:, 11] = 0.0
    if absgrad:
        v_rec[:, 9:11] = 0.0
    return v_rec


@pytest.mark.parametrize("lt", [16, 64], ids=["fine16", "coarse64"])
@pytest.mark.parametrize("CH", [1, 3, 4])
@pytest.mark.parametrize("W,H,N,seed", [(16, 16, 8, 0), (40, 24, 64, 1)])
def test_compositor_backward_record_fields_against_oracle(env, W, H, N, seed, CH, lt):
    ops, L = env
    lib, st = L.lib(), L.stream()
    radii, m2, d, con, col, op = _scene_inputs(ops, N, W, H, CH, seed)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, _, fids, offs = ops.isect_tiles(m2, radii, d, lt, math.ceil(W / lt), math.ceil(H / lt), want_isect_ids=False, conics=con, opacities=op)
    Mn = fids.numel()
    assert Mn > 0
    r64, a64, stable, wt, wa, ref = _oracle_records((W, H, N, seed, CH, lt), m2, con, col, op, W, H, lt, offs, fids, seed)
    rec = torch.empty(N, L.SPLAT_RECORD_FLOATS, device="cuda")
    render = torch.empty(1, H, W, CH, device="cuda")
    a2 = torch.empty(2, 1, H, W, 1, device="cuda")
    alphas, t_final = a2[0], a2[1]
    last = torch.empty(1, H, W, dtype=torch.int32, device="cuda")
    L.check(lib.bds_splat_pack(N, None, CH, None, L.ptr(m2), L.ptr(con), L.ptr(col), L.ptr(op), None, L.ptr(rec), None, None, 0, None, st), "pack")
    L.check(lib.bds_rasterize_fwd(1, N, Mn, None, CH, L.ptr(rec), None, W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids), L.ptr(render), L.ptr(alphas),
                                  L.ptr(t_final), L.ptr(last), None, 0, 0, 0, st), "fwd")
    err = ((render[0].cpu().double() - r64).abs() / r64.abs().clamp(min=1.0))[stable]
    assert float(err.max()) < 1e-4 and float((alphas[0].cpu().double() - a64).abs()[stable].max()) < 1e-4
    order = ops.bwd_schedule(1, W, H, lt, offs, last)
    v_render, v_alphas = wt[None].contiguous().cuda(), wa[None].contiguous().cuda()
    for absgrad in (True, False):
        v_rec = _records_buffer(N, CH, absgrad)
        L.check(lib.bds_rasterize_bwd(1, N, Mn, None, CH, L.ptr(rec), None, W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids), L.ptr(alphas),
                                      L.ptr(t_final), L.ptr(last), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_rec), int(absgrad), L.ptr(order),
                                      0, 0, 0, st), "bwd")
        torch.cuda.synchronize()
        _check_record(v_rec, ref, CH, absgrad, f"{W}x{H} N={N} CH={CH} list tile {lt}")


@pytest.mark.parametrize("pool_per_tile", [0, 4096], ids=["list_tile_list", "refined_lists"])
def test_strip_form_record_fields_against_oracle(env, pool_per_tile):
    """split_len = 1 on a 32 x 32 image with one 32-px list tile: every non-empty 16 x 16 tile is composited, forward and backward,
    by four strip waves of one pixel per lane (rasterize_bwd_split_kernel, NQ = 1) -- over the list tile's list, or over the tile's own
    refined list from the pool."""
    ops, L = env
    lib, st = L.lib(), L.stream()
    W = H = 32
    N, CH, lt, seed = 64, 4, 32, 2
    radii, m2, d, con, col, op = _scene_inputs(ops, N, W, H, CH, seed)
    tw = th = 2
    _, _, fids, offs = ops.isect_tiles(m2, radii, d, lt, 1, 1, want_isect_ids=False, conics=con, opacities=op)
    Mn = fids.numel()
    assert Mn > 0
    r64, a64, stable, wt, wa, ref = _oracle_records((W, H, N, seed, CH, lt), m2, con, col, op, W, H, lt, offs, fids, seed)
    split = (1, tw * th, pool_per_tile * tw * th)
    n_ints = int(lib.bds_rasterize_schedule_ints(1, tw, th)) + int(lib.bds_rasterize_split_pool_ints(1, tw, th, split[1], split[2], Mn))
    order = torch.zeros(n_ints, dtype=torch.int32, device="cuda")             # (binned form: a clear header)
    m_dev = torch.tensor([Mn], dtype=torch.int64, device="cuda")
    rec = torch.empty(N, L.SPLAT_RECORD_FLOATS, device="cuda")
    render = torch.empty(1, H, W, CH, device="cuda")
    a2 = torch.empty(2, 1, H, W, 1, device="cuda")
    alphas, t_final = a2[0], a2[1]
    last = torch.empty(1, H, W, dtype=torch.int32, device="cuda")
    L.check(lib.bds_splat_pack(N, None, CH, None, L.ptr(m2), L.ptr(con), L.ptr(col), L.ptr(op), None, L.ptr(rec), None, None, 0, None, st), "pack")
    L.check(lib.bds_rasterize_fwd(1, N, Mn, m_dev.data_ptr(), CH, L.ptr(rec), None, W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids), L.ptr(render),
                                  L.ptr(alphas), L.ptr(t_final), L.ptr(last), L.ptr(order), *split, st), "fwd, strips")
    err = ((render[0].cpu().double() - r64).abs() / r64.abs().clamp(min=1.0))[stable]
    assert float(err.max()) < 1e-4 and float((alphas[0].cpu().double() - a64).abs()[stable].max()) < 1e-4
    v_render, v_alphas = wt[None].contiguous().cuda(), wa[None].contiguous().cuda()
    for absgrad in (True, False):
        v_rec = _records_buffer(N, CH, absgrad)
        L.check(lib.bds_rasterize_bwd(1, N, Mn, m_dev.data_ptr(), CH, L.ptr(rec), None, W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids),
                                      L.ptr(alphas), L.ptr(t_final), L.ptr(last), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_rec), int(absgrad),
                                      L.ptr(order), *split, st), "bwd, strips")
        torch.cuda.synchronize()
        _check_record(v_rec, ref, CH, absgrad, f"strips, pool {pool_per_tile}")


# ---- the deferred-epilogue kernel and the camera-pose gradient, through one view ---------------------------------------------------
@pytest.mark.parametrize("list_tile", [16, 64], ids=["fine16", "coarse64"])
def test_view_epilogue_kernel_records_and_pose_gradient_against_oracle(env, monkeypatch, list_tile):
    """One eager view (one stream: the colour transform's backward leaves its last stage to the compositor's backward,
    rasterize_bwd_epi_kernel) of 600 Gaussians (some 70 of them visible) with a learnable pose, a loss that reaches colour, depth and opacity: the gradient
    record the compositor's backward returns, field by field, and all 12 entries of the pose gradient that the projection's backward
    reduces (pose_grad_reduce) against the float64 oracle of the whole view."""
    ops, L = env
    from bilateral_driving_amd import fused_view as FV
    from bilateral_driving_amd import harness as Hn
    W, H, N, img = 64, 48, 600, 1
    cam = Hn.ring_cameras(W, H, yaws_deg=(20.0,), device="cuda")[0]
    cam.viewmat = cam.viewmat.clone().requires_grad_(True)
    p = Hn.synthetic_scene(N, seed=7, device="cuda")
    p["means"] = p["means"] * torch.tensor([0.3, 0.3, 1.0], device="cuda")
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(2, device="cuda")]
    gen = torch.Generator().manual_seed(11)
    sky = torch.rand(H, W, 3, generator=gen).cuda()
    # oracle, float64 on the CPU, stage by stage so that the compositor's inputs keep their gradients
    q = {k: v.detach().cpu().double().requires_grad_(True) for k, v in p.items()}
    vm = cam.viewmat.detach().cpu().double().requires_grad_(True)
    K = cam.K.cpu().double()
    radii, m2, dep, con, _ = G.project(q["means"], q["quats"] / q["quats"].norm(dim=-1, keepdim=True), torch.exp(q["log_scales"]), vm, K, W, H,
                                       near_plane=0.1)
    dirs = q["means"].detach() - torch.linalg.inv(vm.detach())[:3, 3]
    col = torch.cat([torch.clamp(G.spherical_harmonics(3, dirs, q["sh"]) + 0.5, 0.0, 1.0), dep[:, None]], -1)
    opac = torch.sigmoid(q["opacity_logits"])
    for t in (m2, con, col, opac):
        t.retain_grad()
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    _, iids, fids = G.isect_tiles(m2, radii, dep, 16, tw, th)
    probe = []
    r, a, _, unstable = G.rasterize_to_pixels(m2, con, col, opac, W, H, 16, G.isect_offset_encode(iids, tw, th), fids, None,
                                              return_unstable=True, absgrad_probe=probe)
    stable = (~unstable)[..., None]
    wr, wd, wo = (torch.randn(H, W, c, generator=gen) * stable for c in (3, 1, 1))
    depth = r[..., 3:4] / a.clamp(min=1e-10)
    rgb = BO.multiscale_transform([g.detach().cpu().double()[img] for g in grids], BO.sky_blend(r[..., :3], a, sky.cpu().double()),
                                  list(Hn.FACTORS_3))
    ((rgb * wr.double()).sum() + 0.05 * (depth * wd.double()).sum() + (a * wo.double()).sum()).backward()
    ref = torch.zeros(N, 16, dtype=torch.float64)
    ref[:, 0:4], ref[:, 4:7], ref[:, 7:9], ref[:, 11] = col.grad, con.grad, m2.grad, opac.grad
    ref[:, 9:11] = G.absgrad_from_probe(probe, N)
    # the view, with the compositor's backward observed
    seen = {}
    inner = FV._composite_backward

    def observed(cfg, saved, vis_ids, *args, **kw):
        v_rec_all, v_rec = inner(cfg, saved, vis_ids, *args, **kw)
        seen.update(epilogue=kw.get("ms") is not None, vis_ids=vis_ids.clone(), v_rec=v_rec.clone())
        return v_rec_all, v_rec
    monkeypatch.setattr(FV, "_composite_backward", observed)
    out = Hn.render_view(p, cam, grids, img, sky, list_tile=list_tile)
    assert torch.equal(out["info"]["radii"].cpu().reshape(-1).long(), radii.long()), "fp32 / fp64 cull decisions differ for this seed"
    ((out["rgb"] * wr.cuda()).sum() + 0.05 * (out["depth"] * wd.cuda()).sum() + (out["opacity"] * wo.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert seen["epilogue"], "this view did not take the deferred-epilogue kernel"
    vis = seen["vis_ids"].long().cpu()
    assert vis.numel() >= 50 and float(ref[radii == 0].abs().sum()) == 0.0
    got = seen["v_rec"][:vis.numel()].cpu().double()
    for k in range(12):
        assert float(ref[:, k].norm()) > 0, (FIELDS[k], "reference column is zero")
        e = _nrm(got[:, k], ref[vis, k])
        print(f"[reduce12] view, list tile {list_tile}, epilogue kernel, {FIELDS[k]}: norm-rel error {e:.2e}")
        assert e < GRAD_TOL, (FIELDS[k], e)
    assert float(got[:, 12:].abs().max()) == 0.0          # (zero-filled by the caller, committed by no lane)
    # camera-pose gradient: 9 rotation + 3 translation sums
    pose, pose_ref = cam.viewmat.grad.cpu().double()[:3, :4], vm.grad[:3, :4]
    assert bool((pose_ref != 0).all()), pose_ref
    e = float((pose - pose_ref).norm() / pose_ref.norm())
    print(f"[reduce12] view, list tile {list_tile}: pose gradient norm-rel error {e:.2e}, entries\n{pose}\n{pose_ref}")
    assert e < GRAD_TOL, e
    assert bool(((pose - pose_ref).abs() <= GRAD_TOL * pose_ref.norm()).all())      # entry by entry: no slot dropped or swapped
    assert float(cam.viewmat.grad[3].abs().max()) == 0.0


# ---- colour pyramid, general low-resolution backward ----------------------------------------------------------------------------
@pytest.mark.parametrize("cells,K", [(0, 1), (3, 2)], ids=["general_kernels_by_option", "two_neighbour_grids"])
def test_pyramid_general_path_grid_gradient_channels_against_oracle(env, cells, K):
    """75 x 130 with factor 4 (it divides neither side), grids of 2 x 2 x 1 and 8 x 8 x 4.  The levels' low-resolution backward is
    ms_lowres_bwd_kernel, whose slice vjp goes through slice_grid_scatter, where the general kernels run: with bds_set_option(7, 0)
    (under the default options the cell-aligned kernels take even this size), and, under the default options, for levels averaged over
    K = 2 neighbour grids.  Each of the 12 affine channels of every grid gradient against the float64 oracle (tests/test_gpu_26's
    tolerance: 1e-3, or 3x the float32 oracle)."""
    ops, L = env
    import bilateral_driving_amd.bilagrid as B
    H, W, factors, levels = 75, 130, [4, 4], [(2, 2, 1), (8, 8, 4)]
    g = torch.Generator().manual_seed(26)
    rgb = torch.rand(H, W, 3, generator=g) * 1.2 - 0.1
    wt = torch.randn(H, W, 3, generator=g)
    grids = []
    for (gx, gy, gl) in levels:
        ident = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).reshape(12, 1, 1, 1).repeat(1, gl, gy, gx)
        x = ident[None] + 0.1 * torch.randn(K, 12, gl, gy, gx, generator=g)
        grids.append(x if K > 1 else x[0])

    def oracle(dt):
        gs = [x.clone().to(dt).requires_grad_(True) for x in grids]
        (BO.multiscale_transform(gs, rgb.to(dt), factors, neighbours=True if K > 1 else None) * wt.to(dt)).sum().backward()
        return [x.grad for x in gs]
    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    L.set_option(L.OPT_CELLS, cells)
    try:
        gg = [x.cuda().requires_grad_(True) for x in grids]
        names = L.bilagrid_kernel_names(B._levels_struct([x if K > 1 else x[None] for x in gg], None, factors), H, W, True)
        assert any("ms_lowres_bwd_kernel" in n for n in names), names
        (B.bilagrid_transform(rgb.cuda(), gg, factors) * wt.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        L.set_option(L.OPT_CELLS, 3)
    for lvl, (got, r64, r32) in enumerate(zip(gg, g64, g32)):
        for ch in range(12):
            sel = (slice(None), ch) if K > 1 else (ch,)
            assert float(r64[sel].norm()) > 0, (lvl, ch)
            e, e32 = _nrm(got.grad[sel], r64[sel]), _nrm(r32[sel], r64[sel])
            print(f"[reduce12] pyramid cells={cells} K={K} level {lvl} channel {ch}: norm-rel error {e:.2e} (float32 oracle {e32:.2e})")
            assert e < max(1e-3, 3.0 * e32), (lvl, ch, e, e32)


# ---- resource report -------------------------------------------------------------------------------------------------------------
def test_backward_compositors_keep_their_registers():
    from tests import test_kernel_resources as R
    rep = kernel_resources("rasterize.hip")
    pins = {k: v for k, v in R.MIN_OCCUPANCY.items() if k.startswith("rasterize_bwd")}
    assert len(pins) == 2
    pins["rasterize_fwd_wave_kernelILi4ELb1ELb1E"] = R.MIN_OCCUPANCY["rasterize_fwd_wave_kernelILi4ELb1ELb1E"]
    for prefix, occ in pins.items():
        hits = [(n, r) for n, r in rep.items() if n.startswith(prefix)]
        assert hits, prefix
        for n, r in hits:
            assert r["ScratchSize"] == 0 and r["Occupancy"] >= occ, (n, r)
    for n, r in rep.items():
        if n.startswith("rasterize_bwd"):
            assert r["ScratchSize"] == 0, (n, r)
