"""-m gpu: the compositors' per-pixel decisions and what they do with finished pixels and strips (csrc/rasterize.hip
rasterize_fwd_wave_body / rasterize_bwd_wave_body).

The forward decides `blend` without asking for T > 0 (a finished pixel carries T < 0, so T (1 - alpha) is below the transmittance floor
by itself: it keeps its T, a live pixel that stops gets -T); the backward takes -1 / opacity once per staged candidate (it rides in the
record's radius slot behind the candidate filter) and multiplies the moment sum with it.  A per-strip early exit (lane pixel q of the 64
lanes is one 16 x 4 strip) was built on these cases too and not kept (profiles/NOTES.md).  Scenes built in pixel space so that every
place where finished pixels and strips matter is hit:

* 40 x 24 (tile row 1 has two strips entirely outside the image: finished from the start) and 32 x 32, 64 Gaussians;
* eight opaque, wide, flat Gaussians in front that cover rows 0..5 only: every pixel of strip 0 of every tile of tile row 0 is
  finished within those eight entries while the strips below go on through the tile's list -- the strips of one tile terminate at
  different depths, and the finished pixels see the rest of the list;
* a tile (1, 0) whose strip 2 (rows 8..11) blends nothing while its neighbours do (last_ids stays 0 there);
* a tile with an empty list (the bottom-right one).

Checks: the one-wave-per-tile kernels' image, alphas, t_final and last_ids bit-equal to the four-strip form (split_len = 1: one pixel
per lane, four waves per tile -- no strip is ever skipped there), 1 / 3 channels and 16-px lists bit-equal to the 4-channel / 64-px
ones, everything within tests/test_gpu_01's bounds of the float64 oracle (image 1e-4, gradients 1e-3 norm-relative), the gradient record
field by field with every reference column non-zero (the opacity field is the one -1 / opacity feeds), and the deferred-epilogue kernel
through one eager view with all 12 pose entries.

Measured on MI355X: image 3.3e-7, alphas 1.2e-7, t_final 1.3e-7 (bound 1e-4); record fields 3e-8 ... 6e-7, the opacity field
1.3e-7 ... 2.3e-7, through the view 7e-7 ... 1.9e-5, pose gradient 3.5e-6 (bound 1e-3)."""
import math

import pytest
import torch

from oracle import bilagrid_oracle as BO
from oracle import gs_oracle as G
from tests import reduce12_model as M12

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4           # tests/test_gpu_01_gs_parity.py: image 1e-4 (relative to max(|ref|, 1)), alphas 1e-4
GRAD_TOL = 1e-3          # ... gradients 1e-3 norm-relative (tests/test_gpu_48_reduce12.py's bound)
POISON = 12345.0
FIELDS = {0: "colour 0", 1: "colour 1", 2: "colour 2", 3: "colour 3", 4: "conic a", 5: "conic b", 6: "conic c", 7: "mean x", 8: "mean y",
          9: "absgrad x", 10: "absgrad y", 11: "opacity"}
SIZES = [(40, 24), (32, 32)]
N = 64


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


def _scene(W, H):
    """64 Gaussians in pixel space (float32, CPU): means2d [1,N,2], conics [1,N,3], depths [1,N], radii [1,N] i32, opacities [1,N],
    colours [1,N,4] (r, g, b, depth)."""
    g = torch.Generator().manual_seed(49 + W)
    mx, my, sx, sy, rho, op, dep = [], [], [], [], [], [], []

    def add(x, y, a, b, r, o, d):
        mx.append(x); my.append(y); sx.append(a); sy.append(b); rho.append(r); op.append(o); dep.append(d)
    # eight opaque, wide, flat ones in front: rows 0..5 of every tile of tile row 0 (alpha >= 1/255 up to 3.33 sigma_y = 2.8 px).
    # Two of them sit on every row of strip 0 with alpha >= 0.99: the second one takes the pixel below the floor of 1e-4
    for i, y0 in enumerate((0.5, 1.5, 2.5, 3.5, 0.6, 1.6, 2.6, 3.4)):
        add(8.0 + 1.3 * i, y0, 400.0, 0.85, 0.0, 1.0, 0.5 + 0.01 * i)
    # tile (1, 0): eight small ones in rows 12..15 (strip 3); rows 8..11 (strip 2) are reached by nothing
    for i in range(8):
        add(17.5 + 1.6 * i, 13.2 + 0.075 * i, 0.6, 0.45, 0.0, 0.5 + 0.05 * i, 2.0 + 0.3 * i)
    # the rest: mid-size ones over tile column 0, none of which reaches x >= 16
    while len(mx) < N:
        a, b = (1.0 + 1.5 * torch.rand(2, generator=g)).tolist()
        x = 1.0 + float(torch.rand(1, generator=g)) * (15.5 - 3.4 * a - 1.0)
        y = 1.0 + float(torch.rand(1, generator=g)) * (H - 2.0)
        add(x, y, a, b, float(torch.rand(1, generator=g)) * 1.2 - 0.6, 0.2 + 0.7 * float(torch.rand(1, generator=g)),
            1.0 + 9.0 * float(torch.rand(1, generator=g)))
    mx, my, sx, sy, rho, op, dep = (torch.tensor(v, dtype=torch.float64) for v in (mx, my, sx, sy, rho, op, dep))
    det = (sx * sy) ** 2 * (1 - rho ** 2)                      # covariance [[sx^2, rho sx sy], [., sy^2]] -> its inverse
    con = torch.stack([sy ** 2 / det, -rho * sx * sy / det, sx ** 2 / det], -1)
    radii = torch.ceil(3.0 * torch.maximum(sx, sy)).to(torch.int32)
    rgb = torch.rand(N, 3, generator=g, dtype=torch.float64)
    col = torch.cat([rgb, dep[:, None]], -1)
    f = lambda t: t.float()[None].contiguous()
    return dict(m2=f(torch.stack([mx, my], -1)), con=f(con), dep=f(dep), radii=radii[None].contiguous(), op=f(op), col=f(col))


def _colours(sc, CH):
    c = sc["col"]
    return {1: c[..., 3:4], 3: c[..., :3], 4: c}[CH].contiguous()


_CACHE = {}


def _lists(ops, sc, W, H, lt):
    key = ("lists", W, H, lt)
    if key not in _CACHE:
        d = {k: v.cuda() for k, v in sc.items()}
        _, _, fids, offs = ops.isect_tiles(d["m2"], d["radii"], d["dep"], lt, math.ceil(W / lt), math.ceil(H / lt), want_isect_ids=False,
                                           conics=d["con"], opacities=d["op"])
        assert fids.numel() > 0
        _CACHE[key] = (fids, offs)
    return _CACHE[key]


def _oracle(ops, sc, W, H, CH, bg):
    """float64 oracle over the 16-px lists (the records carry the radii: lists of 64-px tiles give the same image and gradients) ->
    render, alphas, last_ids, stable, v_render, v_alphas, reference record [N,16]; computed once per (size, channels, background)."""
    key = ("oracle", W, H, CH, bg is not None)
    if key in _CACHE:
        return _CACHE[key]
    fids, offs = _lists(ops, sc, W, H, 16)
    lv = {k: t[0].double().requires_grad_(True) for k, t in dict(m2=sc["m2"], con=sc["con"], col=_colours(sc, CH), op=sc["op"]).items()}
    probe = []
    r, a, last, unstable = G.rasterize_to_pixels(lv["m2"], lv["con"], lv["col"], lv["op"], W, H, 16, offs[0].cpu(), fids.cpu().long(),
                                                 None if bg is None else bg.double(), return_unstable=True, absgrad_probe=probe)
    gen = torch.Generator().manual_seed(7 * W + CH)
    wt = torch.randn(r.shape, generator=gen) * (~unstable)[..., None]
    wa = torch.randn(a.shape, generator=gen) * (~unstable)[..., None]
    ((r * wt.double()).sum() + (a * wa.double()).sum()).backward()
    ref = torch.zeros(N, 16, dtype=torch.float64)
    ref[:, 0:CH], ref[:, 4:7], ref[:, 7:9], ref[:, 11] = lv["col"].grad, lv["con"].grad, lv["m2"].grad, lv["op"].grad
    ref[:, 9:11] = G.absgrad_from_probe(probe, N)
    out = (r.detach(), a.detach(), last, ~unstable, wt, wa, ref)
    _CACHE[key] = out
    return out


def _forward(ops, L, sc, W, H, CH, lt, bg, split=False):
    """-> rec, render, alphas, t_final, last_ids, schedule (None unless split), m_dev"""
    lib, st = L.lib(), L.stream()
    key = ("fwd", W, H, CH, lt, bg is not None, split)
    if key in _CACHE:
        return _CACHE[key]
    fids, offs = _lists(ops, sc, W, H, lt)
    d = {k: v.cuda() for k, v in sc.items()}
    col = _colours(sc, CH).cuda()
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    Mn = fids.numel()
    rec = torch.empty(N, L.SPLAT_RECORD_FLOATS, device="cuda")
    render = torch.full((1, H, W, CH), POISON, device="cuda")
    a2 = torch.full((2, 1, H, W, 1), POISON, device="cuda")
    last = torch.full((1, H, W), -7, dtype=torch.int32, device="cuda")
    bgp = None if bg is None else bg[None].contiguous().cuda()
    L.check(lib.bds_splat_pack(N, None, CH, None, L.ptr(d["m2"]), L.ptr(d["con"]), L.ptr(col), L.ptr(d["op"]), L.ptr(d["radii"]), L.ptr(rec),
                               None, None, 0, None, st), "pack")
    order, m_dev, sp = None, None, (0, 0, 0)
    if split:      # every tile strip by strip over its list tile's list (no refined lists: last_ids stay list positions)
        sp = (1, tw * th, 0)
        order = torch.zeros(int(lib.bds_rasterize_schedule_ints(1, tw, th)), dtype=torch.int32, device="cuda")
        m_dev = torch.tensor([Mn], dtype=torch.int64, device="cuda")
    L.check(lib.bds_rasterize_fwd(1, N, Mn, None if m_dev is None else m_dev.data_ptr(), CH, L.ptr(rec), L.ptr(bgp), W, H, 16, lt, tw, th,
                                  L.ptr(offs), L.ptr(fids), L.ptr(render), L.ptr(a2[0]), L.ptr(a2[1]), L.ptr(last), L.ptr(order), *sp, st), "fwd")
    torch.cuda.synchronize()
    out = (rec, render, a2[0], a2[1], last, order, m_dev, bgp)
    _CACHE[key] = out
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _bg(CH, on):
    return torch.tensor([0.3, 0.7, 0.1, 2.5])[:CH] if on else None


# ---- the scene has the places the changes can go wrong ------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
def test_scene_has_early_strips_a_gap_strip_and_an_empty_tile(env, W, H):
    ops, L = env
    sc = _scene(W, H)
    fids, offs = _lists(ops, sc, W, H, 16)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    o = offs.reshape(-1).cpu().tolist() + [fids.numel()]
    assert o[tw * th] == o[tw * th - 1], "the bottom-right tile's list is not empty"
    _, _, alphas, t_final, last, *_ = _forward(ops, L, sc, W, H, 4, 16, None)
    last, alphas, t_final = last[0].cpu(), alphas[0, ..., 0].cpu(), t_final[0, ..., 0].cpu()
    # tile (0, 0): strip 0 finished (below the transmittance floor times the last blend) long before the tile's deepest entry
    s0, rest = last[0:4, 0:16], last[4:16, 0:16]
    assert float(t_final[0:4, 0:16].max()) < 2e-2 and int(s0.max()) < 8 and int(rest.max()) > 12, (s0.max(), rest.max())
    # tile (1, 0): strips 0, 1, 3 blend, strip 2 nothing (last_ids 0, alpha 0)
    assert int(last[8:12, 16:32].max()) == 0 and float(alphas[8:12, 16:32].max()) == 0.0
    assert int(last[0:4, 16:32].min()) > 0 and int(last[12:16, 16:32].max()) > 0 and float(alphas[4:8, 16:32].max()) > 0
    # the empty tile
    y0, x0 = (th - 1) * 16, (tw - 1) * 16
    assert float(alphas[y0:, x0:].max()) == 0.0 and int(last[y0:, x0:].max()) == 0
    if H % 16:
        assert H - (th - 1) * 16 <= 8, "tile row 1 should have two strips outside the image"


# ---- image: the four-strip form, the other channel counts and list forms, the oracle ---------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True], ids=["no_background", "background"])
@pytest.mark.parametrize("W,H", SIZES)
def test_forward_bit_equal_to_the_strip_form_and_within_oracle_bounds(env, W, H, with_bg):
    ops, L = env
    sc = _scene(W, H)
    bg4 = _bg(4, with_bg)
    _, r4, a4, t4, l4, *_ = _forward(ops, L, sc, W, H, 4, 64, bg4)
    # 1. the four-strip form of the same scene: one pixel per lane, nothing skipped
    _, rs, as_, ts, ls, *_ = _forward(ops, L, sc, W, H, 4, 64, bg4, split=True)
    for name, x, y in (("render", r4, rs), ("alphas", a4, as_), ("t_final", t4, ts), ("last_ids", l4, ls)):
        assert torch.equal(_bits(x), _bits(y)), (name, "one wave per tile differs from the four-strip form")
    # the 16-px lists, and 1 / 3 channels over both list forms: the same pixels through the other instantiations
    for lt in (16, 64):
        for CH in (1, 3, 4):
            if (lt, CH) == (64, 4):
                continue
            _, r, a, t, l, *_ = _forward(ops, L, sc, W, H, CH, lt, _bg(CH, with_bg))
            want = {1: r4[..., 3:4], 3: r4[..., :3], 4: r4}[CH]
            if with_bg and CH == 1:      # (the 1-channel background is the 4-channel one's first entry, not its depth entry)
                want = None
            tag = (lt, CH)
            if want is not None:
                assert torch.equal(_bits(r), _bits(want)), (tag, "render")
            assert torch.equal(_bits(a), _bits(a4)) and torch.equal(_bits(t), _bits(t4)), (tag, "alphas / t_final")
            if lt == 64:
                assert torch.equal(l, l4), (tag, "last_ids")
    # 2. the float64 oracle, tests/test_gpu_01's bounds on the stable pixels
    for CH in (1, 3, 4):
        bg = _bg(CH, with_bg)
        r64, a64, last64, stable, *_ = _oracle(ops, sc, W, H, CH, bg)
        assert float(stable.float().mean()) > 0.8
        for lt in (16, 64):
            _, r, a, t, l, *_ = _forward(ops, L, sc, W, H, CH, lt, bg)
            err = ((r[0].cpu().double() - r64).abs() / r64.abs().clamp(min=1.0))[stable]
            ea = (a[0].cpu().double() - a64).abs()[stable]
            et = (t[0].cpu().double() - (1.0 - a64)).abs()[stable]
            print(f"[diet] {W}x{H} CH={CH} list tile {lt} bg={int(with_bg)}: image {float(err.max()):.2e} alphas {float(ea.max()):.2e} "
                  f"t_final {float(et.max()):.2e}")
            assert float(err.max()) < IMG_TOL and float(ea.max()) < IMG_TOL and float(et.max()) < IMG_TOL
            if lt == 16:
                assert torch.equal(l[0].cpu()[stable], last64[stable]), "last_ids differ from the oracle's on stable pixels"


# ---- gradient records ------------------------------------------------------------------------------------------------------------------
def _records_buffer(CH, absgrad):
    v_rec = torch.full((N, 16), POISON, device="cuda")
    v_rec[:, :CH] = 0.0
    v_rec[:, 4:9] = 0.0
    v_rec[:, 11] = 0.0
    if absgrad:
        v_rec[:, 9:11] = 0.0
    return v_rec


def _check_record(v_rec, ref, CH, absgrad, tag):
    got = v_rec.detach().cpu().double()
    written = list(range(CH)) + [4, 5, 6, 7, 8, 11] + ([9, 10] if absgrad else [])
    for k in range(16):
        if k in written:
            assert float(ref[:, k].norm()) > 0, (tag, FIELDS[k], "reference column is zero")
            e = _nrm(got[:, k], ref[:, k])
            print(f"[diet] {tag} absgrad={int(absgrad)} {FIELDS[k]}: norm-rel error {e:.2e}")
            assert e < GRAD_TOL, (tag, FIELDS[k], e)
        else:
            assert bool((got[:, k] == POISON).all()), (tag, k, "a float of the record that no lane commits was written")


@pytest.mark.parametrize("with_bg", [False, True], ids=["no_background", "background"])
@pytest.mark.parametrize("lt", [16, 64], ids=["fine16", "coarse64"])
@pytest.mark.parametrize("CH", [1, 3, 4])
@pytest.mark.parametrize("W,H", SIZES)
def test_backward_record_fields_against_oracle(env, W, H, CH, lt, with_bg):
    ops, L = env
    lib, st = L.lib(), L.stream()
    sc = _scene(W, H)
    bg = _bg(CH, with_bg)
    _, _, _, stable, wt, wa, ref = _oracle(ops, sc, W, H, CH, bg)
    rec, render, alphas, t_final, last, _, _, bgp = _forward(ops, L, sc, W, H, CH, lt, bg)
    fids, offs = _lists(ops, sc, W, H, lt)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    order = ops.bwd_schedule(1, W, H, lt, offs, last)
    v_render, v_alphas = wt[None].contiguous().cuda(), wa[None].contiguous().cuda()
    for absgrad in (True, False):
        v_rec = _records_buffer(CH, absgrad)
        L.check(lib.bds_rasterize_bwd(1, N, fids.numel(), None, CH, L.ptr(rec), L.ptr(bgp), W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids),
                                      L.ptr(alphas), L.ptr(t_final), L.ptr(last), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_rec), int(absgrad),
                                      L.ptr(order), 0, 0, 0, st), "bwd")
        torch.cuda.synchronize()
        _check_record(v_rec, ref, CH, absgrad, f"{W}x{H} CH={CH} list tile {lt} bg={int(with_bg)}")


@pytest.mark.parametrize("W,H", SIZES)
def test_strip_form_backward_record_fields_against_oracle(env, W, H):
    """The four-strip form's backward (rasterize_bwd_split_kernel, one pixel per lane) shares the body: same records."""
    ops, L = env
    lib, st = L.lib(), L.stream()
    sc = _scene(W, H)
    CH, lt = 4, 64
    _, _, _, stable, wt, wa, ref = _oracle(ops, sc, W, H, CH, None)
    rec, render, alphas, t_final, last, order, m_dev, _ = _forward(ops, L, sc, W, H, CH, lt, None, split=True)
    fids, offs = _lists(ops, sc, W, H, lt)
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    v_render, v_alphas = wt[None].contiguous().cuda(), wa[None].contiguous().cuda()
    for absgrad in (True, False):
        v_rec = _records_buffer(CH, absgrad)
        L.check(lib.bds_rasterize_bwd(1, N, fids.numel(), m_dev.data_ptr(), CH, L.ptr(rec), None, W, H, 16, lt, tw, th, L.ptr(offs), L.ptr(fids),
                                      L.ptr(alphas), L.ptr(t_final), L.ptr(last), L.ptr(v_render), L.ptr(v_alphas), L.ptr(v_rec), int(absgrad),
                                      L.ptr(order), 1, tw * th, 0, st), "bwd, strips")
        torch.cuda.synchronize()
        _check_record(v_rec, ref, CH, absgrad, f"{W}x{H} strips")


def test_reduce_model_is_what_the_records_go_through():
    """tests/reduce12_model.py is unchanged: the 12 committed slots are the record's 12 floats, opacity last."""
    assert sorted(M12.SLOT12[l] for l in M12.COMMIT12_LANES) == list(range(12)) and max(FIELDS) == 11


# ---- the deferred-epilogue kernel through one eager view ---------------------------------------------------------------------------
@pytest.mark.parametrize("list_tile", [16, 64], ids=["fine16", "coarse64"])
def test_view_epilogue_kernel_records_and_pose_gradient_against_oracle(env, monkeypatch, list_tile):
    """One eager view (rasterize_bwd_epi_kernel shares the body) of 600 Gaussians with a learnable pose, as tests/test_gpu_48_reduce12.py
    runs it: the gradient record field by field and all 12 entries of the pose gradient against the float64 oracle of the whole view."""
    ops, L = env
    from bilateral_driving_amd import fused_view as FV
    from bilateral_driving_amd import harness as Hn
    W, H, n, img = 64, 48, 600, 1
    cam = Hn.ring_cameras(W, H, yaws_deg=(20.0,), device="cuda")[0]
    cam.viewmat = cam.viewmat.clone().requires_grad_(True)
    p = Hn.synthetic_scene(n, seed=7, device="cuda")
    p["means"] = p["means"] * torch.tensor([0.3, 0.3, 1.0], device="cuda")
    p = {k: v.requires_grad_(True) for k, v in p.items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(2, device="cuda")]
    gen = torch.Generator().manual_seed(11)
    sky = torch.rand(H, W, 3, generator=gen).cuda()
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
    ref = torch.zeros(n, 16, dtype=torch.float64)
    ref[:, 0:4], ref[:, 4:7], ref[:, 7:9], ref[:, 11] = col.grad, con.grad, m2.grad, opac.grad
    ref[:, 9:11] = G.absgrad_from_probe(probe, n)
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
    assert vis.numel() >= 50
    got = seen["v_rec"][:vis.numel()].cpu().double()
    for k in range(12):
        assert float(ref[:, k].norm()) > 0, (FIELDS[k], "reference column is zero")
        e = _nrm(got[:, k], ref[vis, k])
        print(f"[diet] view, list tile {list_tile}, epilogue kernel, {FIELDS[k]}: norm-rel error {e:.2e}")
        assert e < GRAD_TOL, (FIELDS[k], e)
    pose, pose_ref = cam.viewmat.grad.cpu().double()[:3, :4], vm.grad[:3, :4]
    assert bool((pose_ref != 0).all()), pose_ref
    e = float((pose - pose_ref).norm() / pose_ref.norm())
    print(f"[diet] view, list tile {list_tile}: pose gradient norm-rel error {e:.2e}")
    assert e < GRAD_TOL, e
    assert bool(((pose - pose_ref).abs() <= GRAD_TOL * pose_ref.norm()).all())
