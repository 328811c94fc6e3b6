"""-m gpu: a scene of SEVERAL Gaussian classes through the reference's call sequence (``marshalling.collect_gaussians`` ->
``render_gaussians``, models/trainers/base.py:342-432) with ``marshalling.install(cls, scene=True)`` -- the placeholders survive the
concatenation and ``rendering._RasterizeSceneView`` runs: deferred activations and visible-only SH for the raw classes, the other
classes' rows as they are -- against the SAME sequence with ``scene=False``: every placeholder materialises at the ``torch.cat`` and
the activated-input node ``rendering._RasterizeView`` runs, which tests/test_gpu_03 / 06 tie to the oracle.

The scene is A + B + C = 8 277 rows, no boundary a multiple of 64:
    A raw    K = 16, 6 000 rows, step 10^6 (degree 3)
    B dense  1 500 rows: a test-local class that returns the eager mirror's activated tensors, every seventh opacity times exactly 0
             (the node classes' ``instances_fv`` mask)
    C raw    K = 4, 777 rows, step 0: degree 0 of a degree-1 class (the ramp of vanilla.py:387)
Bounds: those of tests/test_gpu_23_lazy_gaussians.py for the same arithmetic (image 2e-5 max(1, max|ref|), loss 1e-5, gradients 1e-4 of
the reference's largest entry).  Visible rows (float64 oracle projection, checked on the CPU and again here): A 984, B 248, C 136."""
import ctypes
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 256, 192
SEEDS = dict(A=5, B=6, C=7)
ROWS = dict(A=6000, B=1500, C=777)
NAMES = ("_means", "_quats", "_scales", "_opacities", "_features_dc", "_features_rest")


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd import marshalling as M
    from bilateral_driving_amd import rendering as R
    return Hn, M, R


def scene_params(Hn, name, device):
    """Raw parameters of class ``name`` (shared with the CPU check of the visible counts)."""
    p = Hn.synthetic_scene(ROWS[name], seed=SEEDS[name], device=device)
    if name == "C":
        p = dict(p, sh=p["sh"][:, :4].contiguous())
    return p


def visible_rows(Hn, name, cam):
    """radii > 0 of class ``name`` under oracle/gs_oracle.py's float64 projection (CPU)."""
    from oracle import gs_oracle as G
    p = scene_params(Hn, name, "cpu")
    q = p["quats"].double()
    radii = G.project(p["means"].double(), q / q.norm(dim=-1, keepdim=True), p["log_scales"].double().exp(), cam.viewmat.detach().double().cpu(),
                      cam.K.double().cpu(), W, H, near_plane=0.1)[0]
    return radii > 0


def _dense_class(Hn, M):
    class NodeLike(Hn.VanillaModel):
        """A class that hands over ACTIVATED tensors, as the node classes do: the eager mirror's, every seventh opacity times 0."""

        def get_gaussians(self, cam):
            gs = M.get_gaussians(self, cam)
            n = gs["_opacities"].shape[0]
            keep = (torch.arange(n, device=gs["_opacities"].device) % 7 != 0).float()[:, None]
            return dict(gs, _opacities=gs["_opacities"] * keep)
    return NodeLike


@pytest.fixture(scope="module")
def world(mods):
    Hn, M, R = mods
    dev = "cuda"
    cam = Hn.ring_cameras(W, H, yaws_deg=(20.0,), device=dev)[0]
    cam.viewmat.requires_grad_(True)
    NodeLike = _dense_class(Hn, M)
    models = dict(A=Hn.VanillaModel(scene_params(Hn, "A", dev), sh_degree=3, step=10 ** 6),
                  B=NodeLike(scene_params(Hn, "B", dev), sh_degree=3, step=10 ** 6),
                  C=Hn.VanillaModel(scene_params(Hn, "C", dev), sh_degree=1, step=0),
                  Z=NodeLike({k: v[:0] for k, v in scene_params(Hn, "B", dev).items()}, sh_degree=3, step=10 ** 6))
    assert models["C"]._features_rest.shape[1] == 3
    grids = [g.requires_grad_(True) for g in Hn.make_grids(1, device=dev)]
    gen = torch.Generator().manual_seed(5)
    sky = torch.rand(H, W, 3, generator=gen).to(dev)
    target = torch.rand(H, W, 3, generator=gen).to(dev)
    vis = {k: visible_rows(Hn, k, cam) for k in "ABC"}
    return types.SimpleNamespace(cam=cam, models=models, grids=grids, sky=sky, target=target, vis=vis, cache={})


def _leaves(w, order):
    return [p for k in order for p in w.models[k].parameters()] + [w.cam.viewmat] + w.grids


def _run(mods, w, order, scene, antialiased=False, backward=True, mask=None):
    """The reference's sequence over the classes ``order``; returns (outputs, loss, gradients, info, labels)."""
    Hn, M, R = mods
    for t in _leaves(w, order):
        t.grad = None
    cam = w.cam
    camera = M.process_camera({"camera_to_world": torch.linalg.inv(cam.viewmat), "intrinsics": cam.K, "height": H, "width": W}, torch.tensor([0]))
    classes = {k: i for i, k in enumerate(order)}
    M.install(Hn.VanillaModel, scene=scene)
    try:
        gs, labels = M.collect_gaussians({k: w.models[k] for k in order}, classes, camera)
        res, render_fn, info = M.render_gaussians(gs, camera, antialiased=antialiased, training=backward, near_plane=0.1, far_plane=1e10,
                                                  render_mode="RGB+ED", radius_clip=0.0)
        masked = render_fn(mask) if mask is not None else None
    finally:
        M.uninstall(Hn.VanillaModel)
    from bilateral_driving_amd.bilagrid import bilagrid_transform
    rgb = bilagrid_transform(res["rgb_gaussians"], [g[0:1] for g in w.grids], Hn.FACTORS_3, alpha=res["opacity"], sky=w.sky)
    out = dict(rgb=rgb, depth=res["depth"], opacity=res["opacity"], rgb_gaussians=res["rgb_gaussians"], masked=masked)
    if not backward:
        return out, None, None, info, labels
    loss = Hn.training_loss(out, w.target, w.grids) + 0.1 * out["depth"].mean() + 0.1 * out["opacity"].mean()
    loss.backward()
    grads = [t.grad.detach().clone() if t.grad is not None else torch.zeros_like(t) for t in _leaves(w, order)]
    return out, float(loss.detach()), grads, info, labels


def _reference(mods, w, order, antialiased):
    """The comparator (scene=False), computed once per case and left unchanged."""
    key = (order, antialiased)
    if key not in w.cache:
        out, loss, grads, info, labels = _run(mods, w, order, scene=False, antialiased=antialiased)
        w.cache[key] = (({k: v.detach().clone() for k, v in out.items() if v is not None}), loss, grads, info["radii"].clone(),
                        info["means2d"].absgrad.clone(), info["means2d"].grad.clone())
    return w.cache[key]


ORDERS = [pytest.param(("A", "B", "C"), False, id="ABC"), pytest.param(("B", "A"), False, id="BA"), pytest.param(("C", "B", "A"), False, id="CBA"),
          pytest.param(("A", "Z", "B", "C"), False, id="A0BC"), pytest.param(("A", "B", "C"), True, id="ABC-antialiased")]


@pytest.mark.parametrize("order,antialiased", ORDERS)
def test_scene_node_equals_the_materialising_sequence(mods, world, order, antialiased):
    w = world
    out_e, loss_e, g_e, radii_e, absgrad_e, grad_e = _reference(mods, w, order, antialiased)
    out_l, loss_l, g_l, info, labels = _run(mods, w, order, scene=True, antialiased=antialiased)
    radii = info["radii"]
    N = sum(w.models[k]._means.shape[0] for k in order)
    assert radii.shape == (1, N) and labels.shape == (N,)
    a = 0
    for i, k in enumerate(order):      # every segment is seen, as the oracle's projection says
        n = w.models[k]._means.shape[0]
        if n:
            got = (radii[0, a:a + n] > 0).cpu()
            assert int(got.sum()) >= 100 and int(w.vis[k].sum()) >= 100, (k, int(got.sum()), int(w.vis[k].sum()))
        a += n
    assert int((radii > 0).sum()) >= 1000
    assert torch.equal(radii, radii_e)
    for k in ("rgb", "depth", "opacity"):
        err = float((out_l[k] - out_e[k]).abs().max())
        print(f"{k}: err {err:.3e} ref max {float(out_e[k].abs().max()):.3e}")
        assert err <= 2e-5 * max(1.0, float(out_e[k].abs().max())), (k, err)
    print(f"loss {loss_l:.8f} vs {loss_e:.8f}")
    assert abs(loss_l - loss_e) <= 1e-5
    names = [f"{k}.{n}" for k in order for n in NAMES] + ["viewmat", "grid0", "grid1", "grid2"]
    assert len(names) == len(g_l) == len(g_e)
    for n, x, y in zip(names, g_l, g_e):
        assert x.shape == y.shape, n
        ref = float(y.abs().max()) if y.numel() else 0.0
        err = float((x - y).abs().max()) if y.numel() else 0.0
        print(f"{n}: err {err:.3e} ref max {ref:.3e}")
        assert err <= 1e-4 * ref + 1e-9, (n, err, ref)
    for x, y, n in ((info["means2d"].absgrad, absgrad_e, "absgrad"), (info["means2d"].grad, grad_e, "grad")):
        assert x.shape == (1, N, 2) and float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-12, n


def test_the_scene_node_is_what_runs(mods, world):
    Hn, M, R = mods
    w = world
    seen = []
    applies = R._RasterizeSceneView.apply, R._RasterizeRawView.apply, R._RasterizeView.apply
    try:
        R._RasterizeSceneView.apply = staticmethod(lambda *a: (seen.append("scene"), applies[0](*a))[1])
        R._RasterizeRawView.apply = staticmethod(lambda *a: (seen.append("raw"), applies[1](*a))[1])
        R._RasterizeView.apply = staticmethod(lambda *a: (seen.append("one"), applies[2](*a))[1])
        with torch.no_grad():
            out, _, _, _, labels = _run(mods, w, ("A", "B", "C"), scene=True, backward=False)
            assert seen == ["scene"]
            del seen[:]
            # an opacity mask (the evaluation renders, scene_graph.py:296-313): the placeholders materialise, the activated-input node runs
            out2, _, _, _, _ = _run(mods, w, ("A", "B", "C"), scene=True, backward=False, mask=torch.ones(labels.shape[0], device="cuda"))
            assert seen == ["scene", "one"]
            assert float((out2["masked"][0] - out["rgb_gaussians"]).abs().max()) <= 2e-5
            del seen[:]
            _run(mods, w, ("A",), scene=True, backward=False)          # one class: the raw one-view node, as without the flag
            assert seen == ["raw"]
            del seen[:]
            _run(mods, w, ("A", "B", "C"), scene=False, backward=False)
            assert seen == ["one"]
    finally:
        R._RasterizeSceneView.apply, R._RasterizeRawView.apply, R._RasterizeView.apply = applies


def test_culled_rows_cost_nothing_and_get_nothing(mods, world):
    Hn, M, R = mods
    w = world
    order = ("A", "B", "C")
    out, loss, grads, info, _ = _run(mods, w, order, scene=True)
    radii = info["radii"][0]
    a = 0
    per = {}
    for i, k in enumerate(order):
        n = w.models[k]._means.shape[0]
        per[k] = (radii[a:a + n] == 0, grads[6 * i:6 * i + 6])
        a += n
    for k in ("A", "C"):      # the raw classes: a culled row has exactly zero gradient in every raw parameter
        culled, gs = per[k]
        assert int(culled.sum()) > 100
        for n, g in zip(NAMES, gs):
            assert float(g[culled].abs().max()) == 0.0, (k, n)
            if (k, n) != ("C", "_features_rest"):      # (C runs at degree 0: its higher bands get zeros in every row)
                assert float(g[~culled].abs().max()) > 0.0, (k, n)
    # a NaN in the SH coefficients of a culled row of A is never read (the check off: it would see it)
    culled_both = torch.nonzero(~w.vis["A"] & per["A"][0].cpu()).flatten()      # culled for the float64 oracle and on the device
    assert culled_both.numel() > 4000
    row = int(culled_both[culled_both.numel() // 2])
    A = w.models["A"]
    keep, check = A._features_rest.detach()[row].clone(), R._CHECK_FINITE
    try:
        R._CHECK_FINITE = False
        with torch.no_grad():
            A._features_rest[row, 7, 1] = float("nan")
            out2, _, _, _, _ = _run(mods, w, order, scene=True, backward=False)
        for k in ("rgb", "depth", "opacity"):
            assert torch.equal(out2[k], out[k].detach()), k
    finally:
        R._CHECK_FINITE = check
        with torch.no_grad():
            A._features_rest[row] = keep


def test_nonfinite_raw_parameters_raise_per_class(mods, world):
    Hn, M, R = mods
    w = world
    order = ("A", "B", "C")
    A, C = w.models["A"], w.models["C"]

    def run():
        with torch.no_grad():
            return _run(mods, w, order, scene=True, backward=False)

    def poke(t, idx, val):
        keep = t.detach()[idx].clone()
        with torch.no_grad():
            t[idx] = val
        return lambda: t.detach().__setitem__(idx, keep)

    run()      # clean: no raise
    for t, idx, val, field, step in ((C._scales, (17, 2), 90.0, "scales", 0), (A._quats, 99, 0.0, "quats", 10 ** 6),
                                     (A._means, (4321, 1), float("nan"), "means", 10 ** 6)):
        undo = poke(t, idx, val)
        try:
            with pytest.raises(ValueError, match=rf"NaN / Inf detected in gaussian {field} at step {step}$"):
                run()
        finally:
            undo()
    undo1, undo2 = poke(C._scales, (17, 2), -float("inf")), poke(A._opacities, (5, 0), float("inf"))
    try:
        run()      # exp(-Inf) = 0, sigmoid(Inf) = 1: the reference does not raise
    finally:
        undo1()
        undo2()
    run()


def _table(rows, kinds, Ks, degs, p0, p1):
    n = len(rows)
    ptr = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    return (n, (ctypes.c_int64 * n)(*rows), (ctypes.c_int * n)(*kinds), (ctypes.c_int * n)(*Ks), (ctypes.c_int * n)(*degs), ptr(p0), ptr(p1))


def test_device_count_form_leaves_the_rows_past_the_count_alone(mods):
    """The two entries called directly with ``n_dev`` holding fewer entries than the capacity: the rows of the records, of sh_rgb and
    of the gradient arrays behind the count keep their poison, the rows in front equal the host-count call's bit for bit, the raw
    rows' records equal bds_splat_pack_sh's over that class alone, and no guard band is written."""
    from bilateral_driving_amd import _lib as L
    from tests.poison import holds_poison, poisoned_allocations
    lib, st, dev = L.lib(), L.stream(), "cuda"
    g = torch.Generator().manual_seed(11)
    rows, kinds, Ks, degs = [300, 0, 100, 77], [1, 0, 0, 1], [16, 1, 1, 4], [3, 0, 0, 1]
    N = sum(rows)
    starts = [0, 300, 300, 400]
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    means, cam_pos = r(N, 3) * 5, r(3)
    dc = [r(300, 3), None, torch.rand(100, 3, generator=g).to(dev), r(77, 3)]
    rest = [r(300, 15, 3) * 0.3, None, None, r(77, 3, 3) * 0.3]
    means2d, conics, depths, opac = r(N, 2), r(N, 3), r(N), torch.rand(N, generator=g).to(dev)
    radii = torch.randint(1, 50, (N,), generator=g).to(dev).int()
    cap, cnt = 400, 333
    ids = torch.randperm(N, generator=g)[:cap].int().to(dev)
    n_dev = torch.tensor([cnt], dtype=torch.int64, device=dev)
    scales, o_act = torch.rand(N, 3, generator=g).to(dev), torch.rand(N, generator=g).to(dev)
    v_rec = r(cap, L.GRAD_RECORD_FLOATS)
    fwd = _table(rows, kinds, Ks, degs, dc, rest)

    def pack(n, nd, rec, sh_rgb):
        L.check(lib.bds_scene_pack(n, nd, L.ptr(ids), *fwd, L.ptr(means), L.ptr(cam_pos), L.ptr(means2d), L.ptr(conics), L.ptr(depths), L.ptr(opac),
                                   L.ptr(radii), L.ptr(rec), L.ptr(sh_rgb), None, None, 0, None, st), "bds_scene_pack")

    def sh_bwd(n, nd, sh_rgb, v_dc, v_rest, v_scales, v_opac):
        L.check(lib.bds_scene_sh_bwd(n, nd, L.ptr(ids), *_table(rows, kinds, Ks, degs, v_dc, v_rest), L.ptr(means), L.ptr(cam_pos), L.ptr(sh_rgb),
                                     L.ptr(v_rec), L.ptr(scales), L.ptr(o_act), L.ptr(v_scales), L.ptr(v_opac), st), "bds_scene_sh_bwd")

    def grads():
        v_dc = [torch.empty(300, 3, device=dev), None, None, torch.empty(77, 3, device=dev)]
        v_rest = [torch.empty(300, 15, 3, device=dev), None, None, torch.empty(77, 3, 3, device=dev)]
        return v_dc, v_rest

    with poisoned_allocations(True, name="scene entries, device count"):
        rec_d, rgb_d = torch.empty(cap, L.SPLAT_RECORD_FLOATS, device=dev), torch.empty(cap, 3, device=dev)
        rec_h, rgb_h = torch.empty(cnt, L.SPLAT_RECORD_FLOATS, device=dev), torch.empty(cnt, 3, device=dev)
        pack(cap, n_dev.data_ptr(), rec_d, rgb_d)
        pack(cnt, None, rec_h, rgb_h)
        assert bool(holds_poison(rec_d[cnt:]).all()) and bool(holds_poison(rgb_d[cnt:]).all())
        assert not bool(holds_poison(rec_d[:cnt]).any()) and not bool(holds_poison(rgb_d[:cnt]).any())
        assert torch.equal(rec_d[:cnt], rec_h) and torch.equal(rgb_d[:cnt], rgb_h)
        # the raw rows against the one-class pack over that class alone; the dense rows against their colours
        idl = ids[:cnt].long()
        for s in (0, 3):
            mine = (idl >= starts[s]) & (idl < starts[s] + rows[s])
            loc = (idl[mine] - starts[s]).int().contiguous()
            sl = slice(starts[s], starts[s] + rows[s])
            rec1, rgb1 = torch.empty(loc.numel(), L.SPLAT_RECORD_FLOATS, device=dev), torch.empty(loc.numel(), 3, device=dev)
            L.check(lib.bds_splat_pack_sh(loc.numel(), None, L.ptr(loc), Ks[s], degs[s], L.ptr(means[sl].contiguous()), L.ptr(cam_pos), L.ptr(dc[s]),
                                          L.ptr(rest[s]), L.ptr(means2d[sl].contiguous()), L.ptr(conics[sl].contiguous()), L.ptr(depths[sl].contiguous()),
                                          L.ptr(opac[sl].contiguous()), L.ptr(radii[sl].contiguous()), L.ptr(rec1), L.ptr(rgb1), None, None, 0, None, st),
                    "bds_splat_pack_sh")
            assert int(mine.sum()) > 20
            # (the same sums of at most 16 products of magnitude < 4: a few ulp of a value below 8)
            assert float((rec_d[:cnt][mine] - rec1).abs().max()) <= 4e-6 and float((rgb_d[:cnt][mine] - rgb1).abs().max()) <= 4e-6, s
        mine = (idl >= 300) & (idl < 400)
        assert torch.equal(rec_d[:cnt][mine][:, 6:9], dc[2][idl[mine] - 300]) and float(rgb_d[:cnt][mine].abs().max()) == 0.0

        # the backward entry: rows of the lists' entries behind the count keep their poison, in every gradient array
        v_dc_d, v_rest_d = grads()
        v_dc_h, v_rest_h = grads()
        vs_d, vo_d = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
        vs_h, vo_h = torch.empty(N, 3, device=dev), torch.empty(N, device=dev)
        vs0, vo0 = r(N, 3), r(N)
        seen = torch.zeros(N, dtype=torch.bool, device=dev)
        seen[idl] = True
        raw_row = torch.zeros(N, dtype=torch.bool, device=dev)
        raw_row[0:300] = True
        raw_row[400:477] = True
        for vs, vo in ((vs_d, vo_d), (vs_h, vo_h)):      # (what the ACTIVATED projection backward left: the listed rows only)
            vs[seen] = vs0[seen]
            vo[seen] = vo0[seen]
        sh_bwd(cap, n_dev.data_ptr(), rgb_d, v_dc_d, v_rest_d, vs_d, vo_d)
        sh_bwd(cnt, None, rgb_h, v_dc_h, v_rest_h, vs_h, vo_h)
        for s in (0, 3):
            listed = torch.zeros(rows[s], dtype=torch.bool, device=dev)
            m = (idl >= starts[s]) & (idl < starts[s] + rows[s])
            listed[idl[m] - starts[s]] = True
            for d, h in ((v_dc_d[s], v_dc_h[s]), (v_rest_d[s], v_rest_h[s])):
                assert bool(holds_poison(d[~listed]).all()) and not bool(holds_poison(d[listed]).any())
                assert torch.equal(d[listed], h[listed])
        assert bool(holds_poison(vs_d[~seen]).all()) and bool(holds_poison(vo_d[~seen]).all())
        assert torch.equal(vs_d[seen], vs_h[seen]) and torch.equal(vo_d[seen], vo_h[seen])
        chained = seen & raw_row
        assert torch.equal(vs_d[seen & ~raw_row], vs0[seen & ~raw_row]) and torch.equal(vo_d[seen & ~raw_row], vo0[seen & ~raw_row])
        assert torch.equal(vs_d[chained], vs0[chained] * scales[chained])
        assert torch.equal(vo_d[chained], vo0[chained] * o_act[chained] * (1 - o_act[chained]))
        # ... and against the one-class SH backward over class 0 alone
        m = (idl >= 0) & (idl < 300)
        ranks = torch.nonzero(m).flatten()
        loc = idl[m].int().contiguous()
        v1 = torch.zeros(300, 3, device=dev), torch.zeros(300, 15, 3, device=dev)
        L.check(lib.bds_sh_view_bwd_list(loc.numel(), None, L.ptr(loc), 16, 3, L.ptr(means[:300].contiguous()), L.ptr(cam_pos),
                                         L.ptr(rgb_d[ranks].contiguous()), 1, L.ptr(v_rec[ranks].contiguous()), L.ptr(v1[0]), L.ptr(v1[1]), None, 0, st),
                "bds_sh_view_bwd_list")
        listed = torch.zeros(300, dtype=torch.bool, device=dev)
        listed[idl[m]] = True
        assert torch.equal(v_dc_d[0][listed], v1[0][listed]) and torch.equal(v_rest_d[0][listed], v1[1][listed])


def test_scene_node_on_poisoned_memory_leaves_nothing_unwritten(mods, world):
    """The whole [A, B, C] step with every ``torch.empty`` poisoned and guard-banded (tests/poison.py): no output or gradient element
    holds the poison (a NaN: it would also break the bounds), the results are those of the clean run within the bounds of the first
    test (the backward's atomic sums are not ordered), and no guard is written."""
    from tests.poison import holds_poison, poisoned_allocations
    w, order = world, ("A", "B", "C")
    out, loss, grads, info, _ = _run(mods, w, order, scene=True)
    with poisoned_allocations(True, name="scene view"):
        out_p, loss_p, grads_p, info_p, _ = _run(mods, w, order, scene=True)
        for k in ("rgb", "depth", "opacity"):
            assert not bool(holds_poison(out_p[k]).any()), k
            assert float((out_p[k] - out[k]).abs().max()) <= 2e-5 * max(1.0, float(out[k].abs().max())), k
        assert abs(loss_p - loss) <= 1e-5
        for x, y in zip(grads_p, grads):
            assert not bool(holds_poison(x).any())
            assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-9
        for k in ("radii", "depths", "conics", "opacities", "means2d"):
            assert not bool(holds_poison(info_p[k]).any()), k
            assert torch.equal(info_p[k].detach(), info[k].detach()), k
