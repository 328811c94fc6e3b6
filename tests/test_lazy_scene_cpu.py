"""Host logic of the lazy scene (``lazy_gaussians.LazyCat`` / ``lazy_scene`` / ``marshalling.install(cls, scene=True)``): with scene
sources the placeholders of a class survive the concatenation with other classes' tensors that the reference's trainer does
(the reference's models/trainers/base.py:355-366) and ``gs.opacities.squeeze()`` (:397); any other use gives exactly
``torch.cat`` of the reference's expressions.  Without the flag nothing changes (tests/test_lazy_gaussians.py).  The segment lookup
of csrc/scene_math.h runs on the host through tests/hostmath_scene_shim.hip.  CPU: no kernel runs."""
import ctypes

import numpy as np
import pytest
import torch

from bilateral_driving_amd import harness as Hn
from bilateral_driving_amd import marshalling as M
from bilateral_driving_amd.lazy_gaussians import LazyCat, LazyField, RawGaussians, lazy_scene, lazy_source, materialised
from tests.util import build_shim

SHAPES = {"_means": 3, "_opacities": 1, "_scales": 3, "_quats": 4, "_rgbs": 3}
CAM = torch.zeros(3)


def _src(N=12, seed=3, scene=True, K=16, deg=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
    return RawGaussians(r(N, 3), r(N, 4), r(N, 3), r(N, 1), r(N, 3), r(N, K - 1, 3), deg, CAM, step=7, scene=scene)


def _lazy(src):
    N = src.means.shape[0]
    return {k: LazyField(src, k, (N, w)) for k, w in SHAPES.items()}


def _dense(n, seed=9):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(n, w, generator=g).requires_grad_(True) for k, w in SHAPES.items()}


def _cat(classes):
    return {k: torch.cat([c[k] for c in classes], dim=0) for k in SHAPES}          # base.py:365-366


def _args(cat, **swap):
    cat = dict(cat, **swap)
    return cat["_means"], cat["_quats"], cat["_scales"], cat["_opacities"].squeeze(), cat["_rgbs"]


def test_the_concatenation_of_scene_sources_stays_lazy_and_lazy_scene_describes_it():
    a, c = _src(12, 3), _src(5, 4, K=4, deg=0)
    A, B, C = _lazy(a), _dense(7), _lazy(c)
    cat = _cat([A, B, C])
    for k, w in SHAPES.items():
        assert isinstance(cat[k], LazyCat) and cat[k].shape == (24, w) and cat[k].dtype == torch.float32 and len(cat[k]._parts) == 3
        assert torch.cat([cat[k]], 0) is cat[k]
    op = cat["_opacities"].squeeze()                                                  # base.py:397
    assert isinstance(op, LazyCat) and op.shape == (24,)
    assert isinstance(cat["_scales"].reshape(-1, 3), LazyCat) and type(cat["_quats"].reshape(-1, 4)) is torch.Tensor
    segs = lazy_scene(*_args(cat))
    assert [(s.start, s.n, s.raw) for s in segs] == [(0, 12, True), (12, 7, False), (19, 5, True)]
    assert segs[0].src is a and segs[2].src is c and segs[1].dense[0] is B["_means"] and segs[1].dense[4] is B["_rgbs"]
    assert lazy_source(*_args(cat)) is None
    # a zero-row part is legal
    z = _cat([A, _dense(0), B])
    assert [(s.start, s.n, s.raw) for s in lazy_scene(*_args(z))] == [(0, 12, True), (12, 0, False), (12, 7, False)]


def test_lazy_scene_refuses_what_the_node_does_not_serve():
    a, c = _src(12, 3), _src(5, 4)
    A, B, C = _lazy(a), _dense(7), _lazy(c)
    cat = _cat([A, B, C])
    assert lazy_scene(*_args(cat)) is not None
    # a missing field: one argument an ordinary tensor
    assert lazy_scene(*_args(cat, _quats=materialised(cat["_quats"]))) is None
    assert lazy_scene(*_args(cat, _means=torch.zeros(24, 3))) is None
    # a permuted partition: the same parts in another order in one field
    assert lazy_scene(*_args(cat, _scales=torch.cat([C["_scales"], B["_scales"], A["_scales"]], 0))) is None
    assert lazy_scene(*_args(cat, _scales=torch.cat([A["_scales"], B["_scales"][:6], torch.cat([B["_scales"][6:], torch.ones(0, 3)]), C["_scales"]], 0))) is None
    # a part whose five placeholders come from two sources
    other = _src(12, 5)
    mixed = dict(A, _quats=LazyField(other, "_quats", (12, 4)))
    assert lazy_scene(*_args(_cat([mixed, B, C]))) is None
    # a part that is half placeholders, half tensors
    half = dict(A, _scales=torch.ones(12, 3))
    assert lazy_scene(*_args(_cat([half, B, C]))) is None
    # 9 parts
    nine = _cat([A] + [_dense(2, s) for s in range(8)])
    assert all(isinstance(v, LazyCat) for v in nine.values()) and lazy_scene(*_args(nine)) is None
    eight = _cat([A] + [_dense(2, s) for s in range(7)])
    assert len(lazy_scene(*_args(eight))) == 8
    # no raw part: plain tensors only never make a LazyCat
    plain = _cat([B, _dense(3)])
    assert all(type(v) is torch.Tensor for v in plain.values()) and lazy_scene(*_args(plain)) is None
    # another camera behind one of the sources
    far = RawGaussians(c.means, c.quats, c.log_scales, c.logits, c.features_dc, c.features_rest, 3, torch.ones(3), step=7, scene=True)
    assert lazy_scene(*_args(_cat([A, B, _lazy(far)]))) is None


def test_any_other_use_is_the_cat_of_the_references_expressions():
    a, c = _src(12, 3), _src(5, 4)
    B = _dense(7)
    cat = _cat([_lazy(a), B, _lazy(c)])
    want = {"_means": torch.cat([a.means, B["_means"], c.means]),
            "_opacities": torch.cat([torch.sigmoid(a.logits), B["_opacities"], torch.sigmoid(c.logits)]),
            "_scales": torch.cat([torch.exp(a.log_scales), B["_scales"], torch.exp(c.log_scales)]),
            "_quats": torch.cat([a.quats / a.quats.norm(dim=-1, keepdim=True), B["_quats"], c.quats / c.quats.norm(dim=-1, keepdim=True)])}
    for k, w in want.items():
        got = cat[k] * 1.0
        assert type(got) is torch.Tensor and got.requires_grad and torch.equal(got, w * 1.0), k
        assert materialised(cat[k]) is materialised(cat[k])                             # cached
    m = cat["_opacities"].squeeze() * torch.ones(24)                                    # an opacity mask (scene_graph.py:296-313)
    assert type(m) is torch.Tensor and m.shape == (24,) and torch.equal(m, want["_opacities"].squeeze())
    assert materialised(cat["_opacities"].squeeze()).data_ptr() == materialised(cat["_opacities"]).data_ptr()      # one concatenation per field
    assert torch.equal(cat["_quats"].detach(), want["_quats"].detach())
    (cat["_scales"] * 1.0).sum().backward()
    (cat["_opacities"].squeeze() * 2.0).sum().backward()
    for s in (a, c):
        assert torch.equal(s.log_scales.grad, torch.exp(s.log_scales).detach())
        assert torch.allclose(s.logits.grad, 2.0 * (torch.sigmoid(s.logits) * (1 - torch.sigmoid(s.logits))).detach())
    assert torch.equal(B["_scales"].grad, torch.ones(7, 3)) and torch.equal(B["_opacities"].grad, torch.full((7, 1), 2.0))


def test_materialising_raises_the_references_message_per_raw_part():
    a, c = _src(12, 3), _src(5, 4)
    with torch.no_grad():
        c.log_scales[3, 1] = 90.0
        a.log_scales[0, 0] = -float("inf")
        a.logits[2] = float("inf")
    cat = _cat([_lazy(a), _dense(7), _lazy(c)])
    assert isinstance(cat["_scales"], LazyCat)                                          # lazy: nothing has been looked at
    with pytest.raises(ValueError, match="Inf detected in gaussian _scales at step 7"):
        cat["_scales"] * 1.0
    assert bool(torch.isfinite(cat["_opacities"].squeeze() * torch.ones(24)).all())
    with torch.no_grad():
        a.quats[5] = 0.0
    with pytest.raises(ValueError, match="NaN detected in gaussian _quats at step 7"):
        cat["_quats"] + 0.0


def test_without_the_flag_a_second_tensor_materialises_at_the_cat():
    src = _src(scene=False)
    assert RawGaussians(*[torch.zeros(1, 3)] * 6, 3, CAM).scene is False
    q = LazyField(src, "_quats", (12, 4))
    both = torch.cat([q, torch.ones(2, 4)], dim=0)
    assert type(both) is torch.Tensor and both.shape == (14, 4)
    with torch.no_grad():
        src.log_scales[3, 1] = 90.0
    with pytest.raises(ValueError, match="Inf detected in gaussian _scales at step 7"):
        torch.cat([LazyField(src, "_scales", (12, 3)), torch.ones(2, 3)], dim=0)
    # mixed: one scene source next to a source without the flag materialises too
    mixed = torch.cat([LazyField(_src(4, 1), "_quats", (4, 4)), q], dim=0)
    assert type(mixed) is torch.Tensor and mixed.shape == (16, 4)
    # another dtype / trailing shape next to a scene placeholder: the eager concatenation, with torch's own result or error
    s = _src(4, 1)
    assert type(torch.cat([LazyField(s, "_quats", (4, 4)), torch.ones(2, 4, dtype=torch.float64)], 0)) is torch.Tensor
    with pytest.raises(RuntimeError):
        torch.cat([LazyField(s, "_quats", (4, 4)), torch.ones(2, 3)], 0)


def test_install_scene_is_opt_in():
    p = Hn.synthetic_scene(50, seed=1)
    p2 = Hn.synthetic_scene(20, seed=2)
    model, second = Hn.VanillaModel(p), Hn.VanillaModel(dict(p2, sh=p2["sh"][:, :4].contiguous()), sh_degree=1, step=0)
    flat = Hn.VanillaModel(Hn.synthetic_scene(9, seed=3), sh_degree=0)
    cam = M.dataclass_camera(camtoworlds=torch.eye(4), camtoworlds_gt=torch.eye(4), Ks=torch.eye(3), H=8, W=8)
    eager = Hn.VanillaModel.__dict__["get_gaussians"]
    M.install(Hn.VanillaModel)
    try:
        assert Hn.VanillaModel.get_gaussians is M.get_gaussians_lazy
        gs = model.get_gaussians(cam)
        assert gs["_quats"]._src.scene is False
        assert type(torch.cat([gs["_quats"], torch.ones(2, 4)], 0)) is torch.Tensor
    finally:
        M.uninstall(Hn.VanillaModel)
    M.install(Hn.VanillaModel, scene=True)
    try:
        gs = model.get_gaussians(cam)
        assert all(isinstance(v, LazyField) and v._src.scene for v in gs.values())
        models = {"Background": model, "Second": second, "Flat": flat}
        g, labels = M.collect_gaussians(models, {"Background": 0, "Second": 1, "Flat": 2}, cam)
        assert labels.shape == (79,) and isinstance(g.opacities.squeeze(), LazyCat) and g.means.shape == (79, 3)
        segs = lazy_scene(g.means, g.quats, g.scales, g.opacities.squeeze(), g.rgbs)
        # (a class without SH bands takes the eager mirror: a dense part)
        assert [(s.start, s.n, s.raw) for s in segs] == [(0, 50, True), (50, 20, True), (70, 9, False)]
        assert segs[0].src.sh_degree == 3 and segs[1].src.sh_degree == 0 and segs[1].src.features_rest.shape[1] == 3
        # one class alone: the placeholder itself, as without the flag
        one, _ = M.collect_gaussians({"Background": model}, {"Background": 0}, cam)
        assert isinstance(one.quats, LazyField) and lazy_source(one.means, one.quats, one.scales, one.opacities.squeeze(), one.rgbs) is not None
    finally:
        M.uninstall(Hn.VanillaModel)
    assert Hn.VanillaModel.__dict__["get_gaussians"] is eager


def test_segment_lookup_equals_searchsorted_for_every_id():
    lib = build_shim("scene")
    lib.hm_scene_segments.restype = ctypes.c_int
    sizes = [0, 1, 63, 64, 65, 1000]
    rows = np.asarray(sizes, dtype=np.int64)
    N = int(rows.sum())
    ids = np.arange(N, dtype=np.int32)
    starts, seg, total = np.zeros(8, np.int32), np.full(N, -1, np.int32), np.zeros(1, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.hm_scene_segments(len(sizes), p(rows), ctypes.c_int64(N), p(ids), p(starts), p(seg), p(total)) == 0
    want_starts = np.concatenate([[0], np.cumsum(rows)[:-1]])
    assert int(total[0]) == N and np.array_equal(starts[:6], want_starts) and (starts[6:] == np.iinfo(np.int32).max).all()
    want = np.searchsorted(want_starts, ids, side="right") - 1
    assert np.array_equal(seg, want)
    assert (seg != 0).all() and seg.max() == 5                                      # the zero-row segment is never selected
    local = ids - want_starts[seg]
    assert (local >= 0).all() and (local < rows[seg]).all()                         # every id inside its own segment's [0, n)
    # a trailing and a middle zero-row segment, a single segment, the refusals of the set-up
    for sz in ([5, 0, 0, 7, 0], [3], [0, 0, 4], [1] * 8):
        rows = np.asarray(sz, dtype=np.int64)
        n = int(rows.sum())
        ids = np.arange(n, dtype=np.int32)
        seg = np.full(n, -1, np.int32)
        assert lib.hm_scene_segments(len(sz), p(rows), ctypes.c_int64(n), p(ids), p(starts), p(seg), p(total)) == 0
        st = np.concatenate([[0], np.cumsum(rows)[:-1]])
        assert np.array_equal(seg, np.searchsorted(st, ids, side="right") - 1) and (rows[seg] > 0).all(), sz
    # ids outside [0, N): still an answer inside the table (the kernels bound the local row by the segment's count)
    odd = np.asarray([-1, -2 ** 31, 2 ** 31 - 2], dtype=np.int32)
    seg = np.full(3, -1, np.int32)
    rows = np.asarray([4, 4], dtype=np.int64)
    assert lib.hm_scene_segments(2, p(rows), ctypes.c_int64(3), p(odd), p(starts), p(seg), p(total)) == 0
    assert seg.tolist() == [0, 0, 1]
    for bad in ([1] * 9, [3, -1], [2 ** 31 - 1, 1]):
        rows = np.asarray(bad, dtype=np.int64)
        assert lib.hm_scene_segments(len(bad), p(rows), ctypes.c_int64(0), p(ids), p(starts), p(seg), p(total)) == -1
