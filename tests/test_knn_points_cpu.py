"""The pytorch3d drop-in on the CPU (bilateral_driving_amd/p3d.py, skinning_field.py, dropin/pytorch3d): the chunked torch formulation
of ``knn_points`` against the numpy restatement (tests/knn_cross_ref64.py), the device math on the host
(tests/hostmath_knn_cross_shim.hip), the golden that pins the restatement, the rotation conversions, the import surface and the seam.

Bounds, all fixed here before anything ran on a GPU; tests/test_gpu_53_knn_points.py imports them.

DIST_RTOL = 2e-6, relative, on ``dists`` against the float64 restatement (exactly 0 where that is 0).  tests/test_knn_cpu.py derives
1e-6 for the distance (three float32 differences, three squares, two sums and a root within about 3 ulp, 1e-6 being about 8 ulp); the
value here is the distance's SQUARE, whose relative error is twice the distance's, hence twice the figure.  The K-th smallest of values
that are each within a relative eps of their exact ones is within eps of the exact K-th smallest, so the bound carries over to the
sorted lists whatever the neighbour chosen at a near-tie.  Against the float32 restatement there is no tolerance at all: no operation
of the value is fused and the (value, row) order is total, so that restatement is the specification, bit for bit.

BLEND_FLOOR = 7.8e-8: how far the float64 restatement of the skinning field (blend plus relaxation, from the float32 search's rows)
stands from the REFERENCE's float32 result on tests/golden/knn_points/voxel_weights_f32.npz -- 7.77e-8 on the blend before the
relaxation, 6.70e-8 on the field after it (test_golden_pins_the_restatement prints both; measured on the CPU, from the reference's own
code, before any device run).

blend_bound(K, fmax) = max(4 * BLEND_FLOOR, (K + 3) * 2^-23 * fmax), absolute, on the device's blend and field against the float64
restatement, fmax the largest |feature|.  Derivation: a blend is a convex sum of K features, sum_k wn_k f_k with wn_k >= 0 and
sum wn = 1, so an error of relative size e in every weight moves it by at most e * fmax.  A weight takes K + 3 float32 roundings:
the root, the reciprocal of the clamped distance, the K - 1 additions of the normaliser (common to all weights), the normaliser's
reciprocal and the product with it -- each at most 2^-24 relative.  The squared distance that enters carries about 2.5 * 2^-24 of
relative error in its root, and the K multiply-adds of the sum itself add at most 2^-24 each of a partial sum that never exceeds
fmax.  Together (K + 3) + 2.5 + K half-ulps, which (K + 3) whole ulps (2^-23 each) cover for every K >= 1.  At K = 30 and fmax = 1
the bound is 3.9e-6.  The relaxation's own float32 roundings are the reference's as well, so they are inside BLEND_FLOOR; its steps
are convex means and a division by a sum within rounding of 1, which do not amplify what enters them."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bilateral_driving_amd import p3d
from bilateral_driving_amd import skinning_field as SF
from tests import knn_cross_ref64 as R
from tests.util import build_shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_RTOL = 2e-6
BLEND_FLOOR = 7.8e-8
KS = (1, 3, 4, 5, 8, 9, 16, 17, 30, 32)
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_points", "voxel_weights_f32.npz")


def blend_bound(K, fmax):
    return max(4.0 * BLEND_FLOOR, (K + 3) * 2.0 ** -23 * float(fmax))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def cpu_search(p1, p2, K, norm=2, len1=None, len2=None, **kw):
    t = lambda n: None if n is None else torch.tensor(n, dtype=torch.int64)
    return p3d.knn_points(torch.from_numpy(p1), torch.from_numpy(p2), t(len1), t(len2), norm=norm, K=K, **kw)


# ---- knn_points' CPU formulation against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CLOUDS) + ["self"])
def test_cpu_formulation_equals_the_restatement(name):
    for K in KS:
        for norm in (2, 1):
            if name == "self":
                p1 = p2 = R.batch("distinct", 2, 150, 150)[1]
            else:
                p1, p2 = R.batch(name, 2, 70, 150)
            got = cpu_search(p1, p2, K, norm)
            d32, i32 = R.search(p1, p2, K, norm, dtype=np.float32)
            d64, _ = R.search(p1, p2, K, norm, dtype=np.float64)
            assert got.dists.dtype == torch.float32 and got.idx.dtype == torch.int64 and got.knn is None
            assert same_bits(got.dists.numpy(), d32), (name, K, norm)
            assert np.array_equal(got.idx.numpy(), i32), (name, K, norm)
            err, zeros, ok = R.within(got.dists.numpy(), d64, DIST_RTOL)
            assert ok and zeros, (name, K, norm, err)
            f32, f64 = R.search_fast(p1, p2, K, norm, dtype=np.float32), R.search_fast(p1, p2, K, norm, dtype=np.float64)
            assert same_bits(f32[0], d32) and np.array_equal(f32[1], i32) and np.array_equal(f64[0], d64)      # the GPU tests' shortcut
            if name == "self":
                assert np.array_equal(i32[..., 0], np.broadcast_to(np.arange(150), (2, 150))) and not d32[..., 0].any()
            if name == "lattice" and norm == 2:      # every value exact: the float32 and the float64 lists are the same numbers
                assert np.array_equal(d32.astype(np.float64), d64)


def test_padding_of_short_clouds_and_lengths():
    p1, p2 = R.batch("uniform", 3, 9, 6)
    for K in (1, 5, 6, 7, 32):
        for norm in (2, 1):
            len1, len2 = (9, 1, 0), (6, min(K - 1, 6), 0)
            got = cpu_search(p1, p2, K, norm, len1, len2)
            d32, i32 = R.search(p1, p2, K, norm, len1, len2)
            assert same_bits(got.dists.numpy(), d32) and np.array_equal(got.idx.numpy(), i32), (K, norm)
            valid = R.slots(3, 9, 6, K, len1, len2)
            assert not got.dists.numpy()[~valid].any() and not got.idx.numpy()[~valid].any()
            assert not valid[2].any() and not valid[1, 1:].any() and valid[0, :, :min(K, 6)].all() and not valid[0, :, 6:].any()
    empty = cpu_search(p1, np.zeros((3, 0, 3), np.float32), 3)
    assert empty.dists.shape == (3, 9, 3) and not empty.dists.any() and not empty.idx.any()
    none = cpu_search(np.zeros((3, 0, 3), np.float32), p2, 3, return_nn=True)
    assert none.dists.shape == (3, 0, 3) and none.knn.shape == (3, 0, 3, 3)
    over = cpu_search(p1, p2, 2, 2, (100, 100, 100), (100, 100, 100))      # lengths above the sizes are clamped
    assert same_bits(over.dists.numpy(), R.search(p1, p2, 2)[0])


def test_return_nn_is_the_gather_and_arguments_are_checked():
    p1, p2 = R.batch("uniform", 2, 11, 23)
    got = cpu_search(p1, p2, 4, return_nn=True, version=3, return_sorted=False)
    assert np.array_equal(got.knn.numpy(), np.stack([p2[b][got.idx.numpy()[b]] for b in range(2)]))
    a, b = torch.from_numpy(p1), torch.from_numpy(p2)
    with pytest.raises(ValueError, match="D = 3"):
        p3d.knn_points(a[..., :2], b[..., :2])
    with pytest.raises(ValueError, match="batch"):
        p3d.knn_points(a[:1], b)
    for K in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            p3d.knn_points(a, b, K=K)
    with pytest.raises(ValueError):
        p3d.knn_points(a, b, norm=3)
    with pytest.raises(ValueError):
        p3d.knn_points(a, b, lengths2=torch.tensor([1]))
    with pytest.raises(ValueError):
        p3d.knn_blend(a, b, torch.zeros(2, 23, 65), 3, (1e-4, 1.0))


def test_gradients_of_the_cpu_route_pass_gradcheck():
    g = torch.Generator().manual_seed(7)
    for norm in (2, 1):
        p1 = torch.rand(1, 5, 3, generator=g, dtype=torch.float64, requires_grad=True)
        p2 = torch.rand(1, 7, 3, generator=g, dtype=torch.float64, requires_grad=True)
        assert torch.autograd.gradcheck(lambda a, b: p3d.knn_points(a, b, K=3, norm=norm).dists.sum(), (p1, p2))
    p1, p2 = R.batch("uniform", 2, 5, 7)      # float32: the values formed again from the rows are the search's own, bit for bit
    a, b = torch.from_numpy(p1).requires_grad_(True), torch.from_numpy(p2)
    with_grad, plain = p3d.knn_points(a, b, K=3, lengths2=torch.tensor([7, 2])), cpu_search(p1, p2, 3, len2=(7, 2))
    assert with_grad.dists.requires_grad and same_bits(with_grad.dists.detach().numpy(), plain.dists.numpy())
    with_grad.dists.sum().backward()
    nn = np.stack([p2[i][plain.idx.numpy()[i]] for i in range(2)])
    want = (2.0 * (p1[:, :, None, :] - nn) * R.slots(2, 5, 7, 3, None, (7, 2))[..., None]).sum(2)
    assert np.allclose(a.grad.numpy(), want, rtol=1e-6, atol=1e-7)


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("knn_cross")
    h.hm_knn_cross_pair.restype = ctypes.c_float
    h.hm_knn_cross_weight.restype = ctypes.c_float
    h.hm_knn_cross_weight.argtypes = [ctypes.c_float] * 3
    return h


@pytest.mark.parametrize("Kc", (4, 8, 16, 32))
def test_host_math_lists_do_not_depend_on_the_order_of_arrival(shim, Kc):
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    for name in ("uniform", "lattice", "duplicates", "far_offset"):
        p2 = np.ascontiguousarray(R.cloud(name, 90, 3))
        q = np.ascontiguousarray(R.cloud(name, 4, 5)[1])
        orders = [np.arange(90), np.arange(90)[::-1].copy(), np.random.default_rng(Kc).permutation(90)]
        for norm in (2, 1):
            d32, i32 = R.search(q[None, None], p2[None], Kc, norm)
            for shift in (1, 0):
                for order in orders:
                    order = np.ascontiguousarray(order, dtype=np.int32)
                    out_d, out_i = np.zeros(Kc, np.float32), np.zeros(Kc, np.int32)
                    assert shim.hm_knn_cross_query(Kc, norm, shift, q.ctypes.data_as(fp), p2.ctypes.data_as(fp), order.ctypes.data_as(ip), 90,
                                                   out_d.ctypes.data_as(fp), out_i.ctypes.data_as(ip)) == 0
                    for K in sorted({1, Kc - 1, Kc}):      # a list longer than asked is exact in its first K
                        assert same_bits(out_d[:K], d32[0, 0, :K]) and np.array_equal(out_i[:K], i32[0, 0, :K]), (name, norm, shift, K)
    # fewer candidates than slots: the rest stays empty
    p2, q = np.ascontiguousarray(R.cloud("uniform", 90, 3)), np.ascontiguousarray(R.cloud("uniform", 4, 5)[0])
    order, out_d, out_i = np.arange(2, dtype=np.int32), np.zeros(Kc, np.float32), np.zeros(Kc, np.int32)
    shim.hm_knn_cross_query(Kc, 2, 1, q.ctypes.data_as(fp), p2.ctypes.data_as(fp), order.ctypes.data_as(ip), 2, out_d.ctypes.data_as(fp),
                            out_i.ctypes.data_as(ip))
    assert np.isinf(out_d[2:]).all() and (out_i[2:] == 0x7FFFFFFF).all() and np.isfinite(out_d[:2]).all()


def test_host_math_value_and_weight(shim):
    fp = ctypes.POINTER(ctypes.c_float)
    p = np.ascontiguousarray(R.cloud("far_offset", 40, 1))
    for norm in (2, 1):
        want = R.values(p[:1], p, norm, np.float32)[0]
        got = np.array([shim.hm_knn_cross_pair(norm, p[0].ctypes.data_as(fp), p[j].ctypes.data_as(fp)) for j in range(40)], np.float32)
        assert same_bits(got, want)
    for d2, want in ((0.0, 1e4), (1e-10, 1e4), (0.25, 2.0), (4.0, 1.0), (1e6, 1.0)):
        assert abs(shim.hm_knn_cross_weight(d2, 1e-4, 1.0) - want) <= 1e-6 * want


# ---- the golden pins the restatement ---------------------------------------------------------------------------------------------------
def test_golden_pins_the_restatement():
    g = np.load(GOLDEN)
    assert sorted(g.files) == ["K", "blend", "field", "resolution_dhw", "verts", "weights", "x"]
    dhw, K = tuple(int(v) for v in g["resolution_dhw"]), int(g["K"])
    assert g["x"].shape == (2, 256, 3) and g["verts"].shape == (2, 97, 3) and g["weights"].shape == (2, 97, 5) and K == 30
    assert np.abs(g["weights"].sum(-1) - 1).max() < 1e-6
    blend, field = R.field(g["x"], g["verts"], g["weights"], dhw, K)
    e_blend, e_field = np.abs(blend - g["blend"]).max(), np.abs(field - g["field"]).max()
    print(f"\nskinning field: float64 restatement against the reference's float32 result: blend {e_blend:.3e}, field {e_field:.3e}; "
          f"BLEND_FLOOR {BLEND_FLOOR:.1e}; the device's bound at K = 30: {blend_bound(K, np.abs(g['weights']).max()):.3e}")
    assert max(e_blend, e_field) <= BLEND_FLOOR
    # the unmodified expression through the CPU knn_points, in float32 torch: inside the bound the device must meet
    got = cpu_search(g["x"], g["verts"], K)
    w = 1.0 / got.dists.sqrt().clamp(1e-4, 1.0)
    w = w / w.sum(-1, keepdim=True)
    feats = torch.from_numpy(g["weights"])
    mine = torch.stack([(w[b][..., None] * feats[b][got.idx[b]]).sum(-2) for b in range(2)])
    assert np.abs(mine.numpy() - blend).max() <= blend_bound(K, np.abs(g["weights"]).max())
    mine = SF.relax(mine.permute(0, 2, 1).reshape(2, 5, *dhw))
    assert np.abs(mine.numpy() - field).max() <= blend_bound(K, np.abs(g["weights"]).max())


# ---- rotation conversions -----------------------------------------------------------------------------------------------------------------
def _axis_aligned():
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = signs[r]
            if np.linalg.det(m) > 0:
                out.append(m)
    return np.stack(out)


def test_matrix_to_quaternion_round_trip():
    g = torch.Generator().manual_seed(11)
    q = torch.nn.functional.normalize(torch.randn(10000, 4, generator=g, dtype=torch.float64), dim=-1)
    tiny = (torch.rand(2000, generator=g, dtype=torch.float64) * 2 - 1) * 1e-6      # real parts within 1e-6 of 0
    q[:2000] = torch.nn.functional.normalize(torch.cat([tiny[:, None], q[:2000, 1:]], -1), dim=-1)
    q[0] = torch.tensor([0.0, 1.0, 0.0, 0.0])
    R32 = torch.cat([p3d.quaternion_to_matrix(q), torch.eye(3, dtype=torch.float64)[None]]).float()
    got = p3d.matrix_to_quaternion(R32)
    assert got.dtype == torch.float32 and got.shape == (10001, 4) and bool(torch.isfinite(got).all())
    assert float((got.norm(dim=-1) - 1).abs().max()) <= 1e-6 and float(got[:, 0].min()) >= 0.0
    back = p3d.quaternion_to_matrix(got)
    err = float((back - R32).abs().max())
    print(f"\nmatrix_to_quaternion round trip over 10001 rotations: {err:.3e}")
    assert err <= 2e-6
    assert torch.equal(got[-1], torch.tensor([1.0, 0.0, 0.0, 0.0]))
    # the quaternion itself, where its sign is not within rounding of free (a real part of 0 leaves it to the matrix's last bits)
    q64 = p3d.standardize_quaternion(q)
    clear = q64[:, 0] > 1e-3
    assert int(clear.sum()) > 7000 and float((got[:-1].double() - q64)[clear].abs().max()) <= 1e-6
    assert float((p3d.quaternion_to_matrix(q64) - p3d.quaternion_to_matrix(-q64)).abs().max()) <= 1e-15


def test_axis_aligned_rotations_are_exact():
    mats = _axis_aligned()
    assert mats.shape == (24, 3, 3)
    got = p3d.matrix_to_quaternion(torch.from_numpy(mats).float())
    want64 = p3d.matrix_to_quaternion(torch.from_numpy(mats))
    assert float((got.double() - want64).abs().max()) <= 1e-7
    assert float((p3d.quaternion_to_matrix(want64) - torch.from_numpy(mats)).abs().max()) <= 1e-15
    comps = torch.tensor([0.0, 0.5, 2.0 ** -0.5, 1.0], dtype=torch.float64)      # every component of these 24 is one of these
    assert float((want64.abs()[..., None] - comps).abs().min(-1).values.max()) <= 1e-15
    assert float(got[:, 0].min()) >= 0.0


def test_half_turns_are_finite_with_finite_gradients():
    axes = torch.nn.functional.normalize(torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 0], [1.0, -2.0, 3.0]], dtype=torch.float64), dim=-1)
    mats = (2.0 * axes[:, :, None] * axes[:, None, :] - torch.eye(3, dtype=torch.float64)).float().requires_grad_(True)
    q = p3d.matrix_to_quaternion(mats)
    assert bool(torch.isfinite(q).all()) and float(q.detach()[:, 0].abs().max()) <= 1e-6
    (q * torch.tensor([1.0, 2.0, 3.0, 4.0])).sum().backward()
    assert bool(torch.isfinite(mats.grad).all())
    assert float((p3d.quaternion_to_matrix(q) - mats).detach().abs().max()) <= 2e-6


def test_axis_angle_against_the_matrix_exponential():
    g = torch.Generator().manual_seed(3)
    axes = torch.nn.functional.normalize(torch.randn(6, 3, generator=g, dtype=torch.float64), dim=-1)
    aa = torch.cat([torch.zeros(1, 3, dtype=torch.float64), axes * torch.pi, axes * 1e-9, axes * 0.7])
    skew = torch.zeros(aa.shape[0], 3, 3, dtype=torch.float64)
    skew[:, 0, 1], skew[:, 0, 2], skew[:, 1, 2] = -aa[:, 2], aa[:, 1], -aa[:, 0]
    skew = skew - skew.transpose(1, 2)
    assert float((p3d.axis_angle_to_matrix(aa) - torch.matrix_exp(skew)).abs().max()) <= 1e-12
    assert torch.equal(p3d.axis_angle_to_matrix(aa[:1])[0], torch.eye(3, dtype=torch.float64))
    assert float((p3d.axis_angle_to_matrix(aa.float()).double() - torch.matrix_exp(skew)).abs().max()) <= 2e-6


def test_standardize_quaternion():
    q = torch.tensor([[-1.0, 2.0, -3.0, 4.0], [1.0, 2.0, 3.0, 4.0], [0.0, -1.0, 0.0, 0.0]])
    assert torch.equal(p3d.standardize_quaternion(q), torch.tensor([[1.0, -2.0, 3.0, -4.0], [1.0, 2.0, 3.0, 4.0], [0.0, -1.0, 0.0, 0.0]]))


# ---- the import surface and the seam ----------------------------------------------------------------------------------------------------
def test_pytorch3d_imports_resolve_to_the_product():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bilateral_driving_amd", "dropin"), ROOT]))
    code = ("import sys\n"
            "assert not any(m == 'pytorch3d' or m.startswith('pytorch3d.') for m in sys.modules)\n"
            "from pytorch3d.ops import knn_points\n"
            "from pytorch3d.ops.knn import knn_points as knn_points_2\n"
            "from pytorch3d.transforms import matrix_to_quaternion, quaternion_to_matrix, axis_angle_to_matrix\n"
            "import pytorch3d, bilateral_driving_amd.p3d as P\n"
            "assert knn_points is P.knn_points and knn_points_2 is P.knn_points\n"
            "assert matrix_to_quaternion is P.matrix_to_quaternion and quaternion_to_matrix is P.quaternion_to_matrix\n"
            "assert axis_angle_to_matrix is P.axis_angle_to_matrix\n"
            "assert 'dropin' in pytorch3d.__file__ and (P.QUERY_BLOCK, P.TARGET_TILE, P.MAX_K, P.MAX_J) == (256, 512, 32, 64)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_constants_match_the_header():
    from tests.util import header
    import re
    got = dict(re.findall(r"#define (BDS_KNN_CROSS_\w+) (\d+)", header()))
    assert got == {"BDS_KNN_CROSS_MAX_K": str(p3d.MAX_K), "BDS_KNN_CROSS_MAX_J": str(p3d.MAX_J),
                   "BDS_KNN_CROSS_QUERY_BLOCK": str(p3d.QUERY_BLOCK), "BDS_KNN_CROSS_TARGET_TILE": str(p3d.TARGET_TILE)}


def test_entry_refuses_bad_arguments_before_any_launch():
    from bilateral_driving_amd import _lib as L
    h, p = L.lib().bds_cross_knn, 4096      # p stands for any aligned device address: nothing is launched
    ok = dict(B=1, P1=8, P2=8, p1=p, p2=p, len1=None, len2=None, K=3, norm=2, dists=p, idx=p, feat=None, J=0, lo=0.0, hi=0.0, blend=None)

    def call(**kw):
        a = dict(ok, **kw)
        return h(a["B"], a["P1"], a["P2"], a["p1"], a["p2"], a["len1"], a["len2"], a["K"], a["norm"], a["dists"], a["idx"], a["feat"], a["J"],
                 a["lo"], a["hi"], a["blend"], None)
    blend = dict(feat=p, blend=p, J=24, lo=1e-4, hi=1.0)
    for bad in (dict(K=0), dict(K=33), dict(norm=0), dict(norm=3), dict(B=-1), dict(P1=-1), dict(P2=-1), dict(p1=None), dict(p2=None),
                dict(dists=None, idx=None), dict(feat=p), dict(blend=p), dict(blend, norm=1), dict(blend, J=0), dict(blend, J=65),
                dict(blend, lo=0.0), dict(blend, lo=2.0), dict(blend, lo=float("nan")), dict(p1=p + 2), dict(dists=p + 2), dict(idx=p + 4),
                dict(len1=p + 4), dict(len2=p + 4), dict(blend, feat=p + 2), dict(P2=2 ** 31 - 1)):
        assert call(**bad) == L.BDS_EINVAL, bad
    assert call(B=0) == 0 and call(P1=0) == 0 and call(B=0, p1=None, p2=None) == 0 and call(P1=0, p1=None) == 0      # nothing to launch


class _StandIn:
    def _query_weights_smpl(self, x, smpl_verts, smpl_weights):
        return "the class's own"


class _Child(_StandIn):
    pass


def test_install_and_uninstall_put_back_exactly_what_was_there():
    own = _StandIn.__dict__["_query_weights_smpl"]
    for cls in (_StandIn, _Child):
        before = dict(cls.__dict__)
        SF.install(cls)
        SF.install(cls)      # twice: the first former is the one put back
        assert cls._query_weights_smpl is SF._query_weights_smpl and getattr(cls, SF.FORMER) is own
        assert cls()._query_weights_smpl(torch.zeros(1, 4, 3), None, None) == "the class's own"      # CPU tensors keep the class's method
        SF.uninstall(cls)
        assert dict(cls.__dict__) == before and cls._query_weights_smpl is own
    SF.install(_StandIn)
    SF.uninstall()
    assert _StandIn.__dict__["_query_weights_smpl"] is own and SF.FORMER not in _StandIn.__dict__
