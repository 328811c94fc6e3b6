"""The pytorch3d drop-in on the MI355X (csrc/knn_cross.hip through bilateral_driving_amd/p3d.py and skinning_field.py) against the
numpy restatement (tests/knn_cross_ref64.py, pinned by tests/test_knn_points_cpu.py, where every bound used here is derived).

``dists`` and ``idx`` are held to the float32 restatement with no tolerance: the value's operations are not fused and the (value,
row) order is total, so that restatement is the specification.  Against float64 the relative 2e-6 of the CPU file holds, and a value
is exactly 0 where the float64 one is.  The blend and the skinning field are held to ``blend_bound`` of the CPU file against the
float64 restatement.

Shapes: T = p3d.TARGET_TILE candidates per LDS tile, Q = p3d.QUERY_BLOCK queries per workgroup; P2 in {1, K-1, K, K+1, T-1, T, T+1,
2T+1} x P1 in {1, Q-1, Q+1} x K on both sides of every list capacity (4, 8, 16, 32) x both norms, each as a batch of three clouds
with lengths (P1, 1, 0) and (P2, K-1, 0): a full cloud, one whose list is never full, and an empty one.

Measured on the MI355X after the bounds were fixed (the tests print each figure): ``dists`` at most 2.05e-7 from float64 (bound
2e-6), 0 on the lattice and the far-offset cloud; the blend at most 5.96e-7 (K = 30, J = 1, bound 3.93e-6); the skinning field on the
golden 5.4e-8 from float64 through ``knn_points`` and 8.1e-8 through the fused blend (bound 3.91e-6), 8.9e-8 from the reference's
recorded float32."""
import numpy as np
import pytest
import torch

from tests import knn_cross_ref64 as R
from tests import poison
from tests.test_knn_points_cpu import BLEND_FLOOR, DIST_RTOL, GOLDEN, KS, blend_bound, same_bits

pytestmark = pytest.mark.gpu

CLAMP = (0.0001, 1.0)


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import p3d
    return p3d


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def lens(n):
    return None if n is None else torch.tensor(n, dtype=torch.int64).cuda()


def run(P, p1, p2, K, norm=2, len1=None, len2=None):
    got = P.knn_points(dev(p1), dev(p2), lens(len1), lens(len2), norm=norm, K=K)
    assert got.dists.is_cuda and got.dists.dtype == torch.float32 and got.idx.dtype == torch.int64 and got.knn is None
    assert got.dists.shape == got.idx.shape == (p1.shape[0], p1.shape[1], K)
    return got.dists.cpu().numpy(), got.idx.cpu().numpy()


def check(P, p1, p2, K, norm, len1=None, len2=None, what=""):
    """The device's result against the float32 restatement (bits) and the float64 one (2e-6); returns the latter error."""
    d, i = run(P, p1, p2, K, norm, len1, len2)
    d32, i32 = R.search_fast(p1, p2, K, norm, len1, len2, np.float32)
    assert same_bits(d, d32), (what, "dists differ from the float32 restatement", int((d.view(np.uint32) != d32.view(np.uint32)).sum()))
    assert np.array_equal(i, i32), (what, "idx differs from the float32 restatement", int((i != i32).sum()))
    d64, _ = R.search_fast(p1, p2, K, norm, len1, len2, np.float64)
    err, zeros, ok = R.within(d, d64, DIST_RTOL)
    assert ok and zeros, (what, err)
    return err


@pytest.mark.parametrize("K", KS)
def test_every_shape_on_both_sides_of_every_edge(P, K):
    T, Q = P.TARGET_TILE, P.QUERY_BLOCK
    worst = 0.0
    for P2 in (1, K - 1, K, K + 1, T - 1, T, T + 1, 2 * T + 1):
        for P1 in (1, Q - 1, Q + 1):
            p1, p2 = R.batch("uniform", 3, P1, P2, seed=K)
            len1, len2 = (P1, min(1, P1), 0), (P2, min(K - 1, P2), 0)
            for norm in (2, 1):
                err = check(P, p1, p2, K, norm, len1, len2, what=(K, P1, P2, norm))
                worst = max(worst, err)
                if P1 == Q + 1 and P2 == 2 * T + 1:      # the same clouds without lengths: every cloud full
                    worst = max(worst, check(P, p1, p2, K, norm, what=(K, P1, P2, norm, "full")))
    print(f"\nknn_points K={K}: worst relative difference from float64 over 48 shapes x 3 clouds {worst:.3e}, bound {DIST_RTOL:.0e}")


@pytest.mark.parametrize("name", ["uniform", "lattice", "duplicates", "self", "planar", "far_offset"])
def test_named_clouds(P, name):
    T, Q = P.TARGET_TILE, P.QUERY_BLOCK
    worst = 0.0
    for K in KS:
        for norm in (2, 1):
            if name == "self":
                p1 = p2 = R.batch("distinct", 1, T + 1, T + 1)[1]
            else:
                p1, p2 = R.batch(name, 1, Q + 1, 2 * T + 1)
            worst = max(worst, check(P, p1, p2, K, norm, what=(name, K, norm)))
            if name == "self":      # the query is its own first neighbour, at 0
                d, i = run(P, p1, p2, K, norm)
                assert np.array_equal(i[..., 0], np.broadcast_to(np.arange(p1.shape[1]), i.shape[:2])) and not d[..., 0].any()
    print(f"\nknn_points {name}: worst relative difference from float64 over {len(KS)} K x 2 norms {worst:.3e}, bound {DIST_RTOL:.0e}")
    if name == "lattice":
        assert worst == 0.0      # every value is exact in float32 there: the row rule alone decides


def test_same_bits_run_to_run_and_under_a_permutation_of_the_queries(P):
    p1, p2 = R.batch("duplicates", 2, P.QUERY_BLOCK + 1, 2 * P.TARGET_TILE + 1)
    perm = np.random.default_rng(0).permutation(p1.shape[1])
    for K, norm in ((3, 2), (30, 2), (32, 1)):
        d, i = run(P, p1, p2, K, norm)
        for _ in range(2):
            d2, i2 = run(P, p1, p2, K, norm)
            assert same_bits(d, d2) and np.array_equal(i, i2)
        dp, ip = run(P, p1[:, perm], p2, K, norm)
        assert same_bits(dp, d[:, perm]) and np.array_equal(ip, i[:, perm])


def test_return_nn_and_gradients_on_the_device(P):
    p1, p2 = R.batch("uniform", 2, 40, 90)
    a, b = dev(p1).requires_grad_(True), dev(p2).requires_grad_(True)
    got = P.knn_points(a, b, K=5, return_nn=True)
    d32, i32 = R.search(p1, p2, 5)
    assert same_bits(got.dists.detach().cpu().numpy(), d32) and np.array_equal(got.idx.cpu().numpy(), i32)
    assert np.array_equal(got.knn.detach().cpu().numpy(), np.stack([p2[k][i32[k]] for k in range(2)]))
    got.dists.sum().backward()
    diff = p1[:, :, None, :].astype(np.float64) - np.stack([p2[k][i32[k]] for k in range(2)])
    assert np.allclose(a.grad.cpu().numpy(), (2 * diff).sum(2), rtol=1e-5, atol=1e-6)
    want_b = np.zeros(p2.shape)
    for k in range(2):
        np.add.at(want_b[k], i32[k].reshape(-1), (-2 * diff[k]).reshape(-1, 3))
    assert np.allclose(b.grad.cpu().numpy(), want_b, rtol=1e-5, atol=1e-6)


# ---- the blend epilogue ------------------------------------------------------------------------------------------------------------------
def check_blend(P, p1, p2, feat, K, len1=None, len2=None, what=""):
    got = P.knn_blend(dev(p1), dev(p2), dev(feat), K, CLAMP, lens(len1), lens(len2))
    assert got.shape == (p1.shape[0], p1.shape[1], feat.shape[2]) and got.dtype == torch.float32
    _, idx = R.search(p1, p2, K, 2, len1, len2, np.float32)
    valid = R.slots(p1.shape[0], p1.shape[1], p2.shape[1], K, len1, len2)
    want = R.blend(p1, p2, feat, idx, valid, CLAMP)
    err, bound = float(np.abs(got.cpu().numpy() - want).max()), blend_bound(K, np.abs(feat).max(initial=0.0))
    print(f"\nblend {what}: K={K} J={feat.shape[2]}: {err:.3e} from float64, bound {bound:.3e}")
    assert err <= bound, (what, K, feat.shape[2], err, bound)
    return got.cpu().numpy(), want


@pytest.mark.parametrize("J", (1, 5, 24, 64))
def test_blend_against_float64(P, J):
    rng = np.random.default_rng(J)
    Q, T = P.QUERY_BLOCK, P.TARGET_TILE
    for K in (3, 30, 32):
        p1, p2 = R.batch("uniform", 2, Q + 1, T + 1, seed=J)
        p1 = p1.copy()
        p1[:, :7] = p2[:, 10:17]                       # queries that coincide with a vertex: distance 0, the lower clamp
        p1[:, 7:12] = p2[:, 20:25] + np.float32(3e-5)  # and within the lower clamp of one
        feat = rng.random((2, T + 1, J), dtype=np.float32)
        feat /= feat.sum(-1, keepdims=True)            # rows that sum to 1, as skinning weights
        got, want = check_blend(P, p1, p2, feat, K, what="coinciding queries")
        assert np.abs(got.sum(-1) - 1).max() <= blend_bound(K, 1.0) * J
        far = p1 + np.float32(5.0)                     # every distance above 1: the upper clamp makes the blend a plain mean
        got, want = check_blend(P, far, p2, rng.standard_normal((2, T + 1, J)).astype(np.float32), K, what="all beyond the upper clamp")
        short = (T + 1, K - 1)                         # fewer candidates than slots: only the valid ones count
        got, want = check_blend(P, p1, p2, feat, K, (Q + 1, 3), short, what="len2 < K")
        assert not got[1, 3:].any() and np.abs(got[1, :3].sum(-1) - 1).max() <= blend_bound(K, 1.0) * J
        none = P.knn_blend(dev(p1), dev(p2), dev(feat), K, CLAMP, None, lens((0, 0))).cpu().numpy()
        assert none.shape == (2, Q + 1, J) and not none.any()      # no candidate at all: zeros


def test_skinning_field_on_the_golden_installed_and_not(P):
    from bilateral_driving_amd import skinning_field as SF
    g = np.load(GOLDEN)
    dhw, K = tuple(int(v) for v in g["resolution_dhw"]), int(g["K"])
    x, verts, weights = dev(g["x"]), dev(g["verts"]), dev(g["weights"])
    blend64, field64 = R.field(g["x"], g["verts"], g["weights"], dhw, K)
    bound = blend_bound(K, np.abs(g["weights"]).max())

    class VoxelDeformer:      # a stand-in with the reference's expression, restated: modules.py:1199-1211 through knn_points, then :1212-1226
        resolution_dhw = dhw

        def _query_weights_smpl(self, x, smpl_verts, smpl_weights):
            dist, idx, _ = P.knn_points(x, smpl_verts.detach(), K=30)
            dist = dist.sqrt().clamp_(0.0001, 1.0)
            near = smpl_weights.unsqueeze(2).expand(-1, -1, idx.shape[2], -1).gather(1, idx.unsqueeze(-1).expand(-1, -1, -1, smpl_weights.shape[-1]))
            ws = 1.0 / dist
            ws = ws / ws.sum(-1, keepdim=True)
            blend = (ws[..., None] * near).sum(-2)
            self.blend = blend.clone()      # (the relaxation works in place on a view of it, as the reference's does)
            b, c = x.shape[0], smpl_weights.shape[-1]
            return SF.relax(blend.permute(0, 2, 1).reshape(b, c, *self.resolution_dhw)).detach()

    m = VoxelDeformer()
    plain = m._query_weights_smpl(x, verts, weights)
    e_blend, e_field = float(np.abs(m.blend.cpu().numpy() - blend64).max()), float(np.abs(plain.cpu().numpy() - field64).max())
    print(f"\nskinning field through knn_points (not installed): blend {e_blend:.3e}, field {e_field:.3e} from float64; bound {bound:.3e}; "
          f"from the reference's recorded float32: blend {np.abs(m.blend.cpu().numpy() - g['blend']).max():.3e}, "
          f"field {np.abs(plain.cpu().numpy() - g['field']).max():.3e} (BLEND_FLOOR {BLEND_FLOOR:.1e})")
    assert e_blend <= bound and e_field <= bound
    SF.install(VoxelDeformer)
    try:
        fused = m._query_weights_smpl(x, verts, weights)
        assert VoxelDeformer._query_weights_smpl is SF._query_weights_smpl
    finally:
        SF.uninstall(VoxelDeformer)
    assert fused.shape == (2, 5, *dhw) and fused.dtype == torch.float32 and not fused.requires_grad
    e_fused = float(np.abs(fused.cpu().numpy() - field64).max())
    e_direct = float(np.abs(SF.query_weights(x, verts, weights, dhw).cpu().numpy() - field64).max())
    print(f"skinning field with the fused blend (installed): field {e_fused:.3e} from float64, bound {bound:.3e}")
    assert e_fused <= bound and e_direct == e_fused
    assert "_query_weights_smpl_torch" not in VoxelDeformer.__dict__


# ---- recycled, poisoned memory ----------------------------------------------------------------------------------------------------------
def test_every_output_element_is_written_on_poisoned_memory(P):
    Q, T = P.QUERY_BLOCK, P.TARGET_TILE
    p1, p2 = R.batch("uniform", 3, Q + 1, T + 1)
    feat = np.random.default_rng(1).random((3, T + 1, 24), dtype=np.float32)
    a, b, f = dev(p1), dev(p2), dev(feat)
    len1, len2 = lens((Q + 1, 1, 0)), lens((T + 1, 16, 0))

    def ops():
        out = {}
        for K in (3, 17, 32):
            for norm in (2, 1):
                r = P.knn_points(a, b, len1, len2, norm=norm, K=K, return_nn=True)
                out[f"dists{K}_{norm}"], out[f"idx{K}_{norm}"], out[f"knn{K}_{norm}"] = r.dists, r.idx, r.knn
            out[f"blend{K}"] = P.knn_blend(a, b, f, K, CLAMP, len1, len2)
            out[f"full{K}"] = P.knn_blend(a, b, f, K, CLAMP)
        out["few"] = P.knn_points(a, b[:, :5], K=9).dists      # P2 < K: the padding slots are written too
        out["few_idx"] = P.knn_points(a, b[:, :5].contiguous(), K=9).idx
        return out
    plain = ops()
    torch.cuda.synchronize()
    with poison.poisoned_allocations(True, name="knn_points") as pz:      # (guards are compared on exit)
        got = ops()
        torch.cuda.synchronize()
        assert len(pz.records) >= 18
    for k, t in got.items():
        assert not bool(poison.holds_poison(t).any()), (k, int(poison.holds_poison(t).sum()))
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, plain[k].view(torch.int32) if t.dtype == torch.float32 else plain[k]), k
    assert not got["few"][..., 5:].any() and not got["few_idx"][..., 5:].any()


# ---- errors, before any launch ------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch(P):
    from bilateral_driving_amd import _lib as L
    p1, p2 = R.batch("uniform", 2, 9, 20)
    a, b = dev(p1), dev(p2)
    with pytest.raises(ValueError):
        P.knn_points(a, torch.from_numpy(p2))              # a CPU / GPU mix
    with pytest.raises(ValueError):
        P.knn_points(torch.from_numpy(p1), b)
    with pytest.raises(ValueError, match="1..32"):
        P.knn_points(a, b, K=33)
    with pytest.raises(ValueError, match="D = 3"):
        P.knn_points(a[..., :2].contiguous(), b[..., :2].contiguous())
    with pytest.raises(ValueError, match="batch"):
        P.knn_points(a[:1], b)
    with pytest.raises(L.BdsError):
        P.knn_blend(a, b, torch.zeros(2, 20, 4), 3, CLAMP)      # features on the CPU
    with pytest.raises(ValueError):
        P.knn_blend(a, b, torch.zeros(2, 20, 4).cuda(), 3, (0.0, 1.0))
    empty = P.knn_points(a[:, :0], b, K=3)                 # valid: nothing to launch
    assert empty.dists.shape == (2, 0, 3)
    nothing = P.knn_points(a, b[:, :0], K=3)               # valid: everything is padding
    assert nothing.dists.shape == (2, 9, 3) and not nothing.dists.any() and not nothing.idx.any()
    torch.cuda.synchronize()
