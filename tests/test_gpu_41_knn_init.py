"""Scene initialisation on the MI355X (csrc/knn.hip through bilateral_driving_amd/init.py) against the float64 restatement of the
reference's neighbour search (tests/knn_ref64.py, pinned to sklearn's recorded distances by tests/test_knn_cpu.py).

Every case of knn_ref64.CASES runs with k = 3, ``uniform`` and ``duplicates`` also with k = 1 and 8.  Distances: relative 1e-6 against
float64 at every point, exactly 0 where the reference is 0 (derived in tests/test_knn_cpu.py: about 3 ulp of float32 arithmetic, the
bound is about 8).  Log-scales: 1e-6 absolute against the float64 logarithm of the float64 mean of the RETURNED distances -- two
float32 sums and a division put the mean within 3 * 2^-24 of that (1.8e-7 in the logarithm), the device's logf is specified to 1 ulp,
4.8e-7 for log-scales of magnitude 4 .. 8, which covers these clouds (the test checks the magnitude); together 6.6e-7, below the
SCALE_FLOOR = 1e-6 recorded in tests/test_knn_cpu.py -- and twice that against torch's own float32 ``log(mean)``, which stands as far
from the exact value.  Measured on the MI355X (the test prints each figure): 9.05e-7 from float64 at the worst, 9.54e-7 from
``torch.log(mean)``.  That is more than the 6.6e-7 derived above: the device's logf stands about 1.5 ulp off there, not 1.  The bound
was set before the measurement and stays; it holds with a tenth to spare."""
import math
import types

import numpy as np
import pytest
import torch

from tests import knn_ref64 as R

pytestmark = pytest.mark.gpu

DIST_RTOL = 1e-6
SCALE_FLOOR = 1e-6
CASE_KS = [(n, k) for n in R.CASES for k in R.GOLDEN_KS[n]]


@pytest.fixture(scope="module")
def I():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import init
    return init


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.view(torch.int32).cpu()


def pair_f32(x, rows):
    """The distance of every point to the given rows as the kernels form it, in numpy float32 (no fused multiply-add)."""
    d = x[:, None, :] - x[rows]
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


@pytest.mark.parametrize("name,k", CASE_KS)
def test_every_case_matches_float64_at_every_point(I, name, k):
    x = R.points(name)
    N = len(x)
    dist, idx, stats = I.k_nearest(dev(x), k, return_stats=True)
    assert dist.shape == (N, k) and dist.dtype == torch.float32 and dist.is_cuda
    assert idx.shape == (N, k) and idx.dtype == torch.int64 and idx.is_cuda
    d, i = dist.cpu().numpy(), idx.cpu().numpy()
    d64, i64 = R.reference(name, k)
    err, e32 = R.distance_error(d, d64), R.distance_error(R.reference(name, k, np.float32)[0], d64)
    print(f"\nknn {name} k={k}: float32 restatement {e32:.3e}, kernel {err:.3e}, bound {DIST_RTOL:.0e}; grid {stats['dims']} edge "
          f"{stats['cell_edge']:.4g}, unresolved {stats['unresolved']} of {N}")
    assert err <= DIST_RTOL, (name, k, err)
    assert np.all(np.diff(d, axis=1) >= 0)
    assert np.all(i != np.arange(N)[:, None]) and i.min() >= 0 and i.max() < N
    assert all(len(set(row)) == k for row in i.tolist())
    assert np.array_equal(pair_f32(x, i).view(np.int32), d.view(np.int32))      # the distance of the reported row, bit for bit
    if name == "lattice":
        assert np.array_equal(i, i64)      # d2 is exact there, so the tie rule decides
    dims = stats["dims"]
    assert min(dims) >= 1 and dims[0] * dims[1] * dims[2] == stats["cells"] <= 2 * N and 0 <= stats["unresolved"] <= N
    assert np.array_equal(np.float32(stats["cloud_lo"]), x.min(0)) and np.array_equal(np.float32(stats["cloud_hi"]), x.max(0))
    assert np.all(np.float32(stats["lo"]) >= x.min(0)) and np.all(np.float32(stats["hi"]) <= x.max(0))
    beyond = (x < np.float32(stats["lo"])).sum(0), (x > np.float32(stats["hi"])).sum(0)
    assert max(beyond[0].max(), beyond[1].max()) <= 2 * (N >> 7)      # two trimming passes of at most N / 128 points each


def test_outliers_reach_the_fallback_and_are_exact(I):
    x = R.points("clusters_outliers")
    dist, idx, stats = I.k_nearest(dev(x), 3, return_stats=True)
    d64, i64 = R.reference("clusters_outliers", 3)
    # From the reported grid alone: a point more than RING_MAX + 1 edges inside both faces of the grid's box on some axis with more
    # than 2 RING_MAX + 1 cells has a last cube whose faces on that axis are not faces of the grid, so its margin is at most
    # (RING_MAX + 1) edges; with its nearest neighbour farther than that, no ring resolves it.  By construction (knn_ref64) that
    # holds for outliers -- every one lies more than 240 m from every other point -- and for no cluster point.
    reach = (I.RING_MAX + 1) * stats["cell_edge"]
    inside = (x > np.float64(stats["lo"]) + reach) & (x < np.float64(stats["hi"]) - reach) & (np.array(stats["dims"]) > 2 * I.RING_MAX + 1)
    must = inside.any(1) & (d64[:, 0] > reach * 1.001)
    print(f"\nknn fallback: edge {stats['cell_edge']:.4g} m, grid {stats['dims']}, {int(must.sum())} points that no ring can resolve, "
          f"unresolved {stats['unresolved']}")
    assert reach < 240.0 and must[:-R.OUTLIERS].sum() == 0 and must[-R.OUTLIERS:].sum() > 0
    assert must.sum() <= stats["unresolved"] <= len(x)
    out = dist.cpu().numpy()[-R.OUTLIERS:]
    assert R.distance_error(out, d64[-R.OUTLIERS:]) <= DIST_RTOL and out.min() > 240.0
    assert np.array_equal(idx.cpu().numpy()[-R.OUTLIERS:], i64[-R.OUTLIERS:])      # (distances hundreds of metres apart: no near-tie)


@pytest.mark.parametrize("name,k", [("uniform", 3), ("duplicates", 3), ("clusters_outliers", 3), ("lattice", 3), ("uniform", 8)])
def test_result_does_not_depend_on_the_order(I, name, k):
    x = dev(R.points(name))
    d0, i0 = I.k_nearest(x, k)
    d1, i1 = I.k_nearest(x, k)
    assert torch.equal(bits(d0), bits(d1)) and torch.equal(i0, i1)      # run to run
    perm = torch.randperm(len(x), generator=torch.Generator().manual_seed(3)).cuda()
    dp, ip = I.k_nearest(x[perm].contiguous(), k)
    assert torch.equal(bits(dp), bits(d0[perm]))
    # the rows name points at the same distances (they may differ from perm^-1(i0) only where distances tie)
    xp = R.points(name)[perm.cpu().numpy()]
    assert np.array_equal(pair_f32(xp, ip.cpu().numpy()).view(np.int32), dp.cpu().numpy().view(np.int32))
    only = I.k_nearest(x, k, return_indices=False)
    assert torch.equal(bits(only), bits(d0))


@pytest.mark.parametrize("dims", [1, 2, 3])
@pytest.mark.parametrize("clamp", [None, (0.002, 100.0)])
def test_init_scales_is_the_log_of_the_mean_distance(I, dims, clamp):
    for name, k in (("uniform", 3), ("duplicates", 3), ("clusters_outliers", 3), ("flat_far", 3), ("duplicates", 8)):
        x = dev(R.points(name))
        s = I.init_scales(x, k, dims, clamp)
        assert s.shape == (len(x), dims) and s.dtype == torch.float32 and s.is_cuda
        for c in range(1, dims):
            assert torch.equal(bits(s[:, c].contiguous()), bits(s[:, 0].contiguous()))
        dist = I.k_nearest(x, k)[0]
        mean64 = dist.cpu().numpy().astype(np.float64).mean(1)
        if clamp is not None:
            mean64 = np.clip(mean64, np.float64(np.float32(clamp[0])), np.float64(np.float32(clamp[1])))
        with np.errstate(divide="ignore"):
            want = np.log(mean64)
        got = s[:, 0].cpu().numpy()
        inf = np.isneginf(want)
        assert inf.sum() == (11 if (clamp is None and name == "duplicates") else 0)      # the point present 11 times: a mean of 0
        assert np.all(np.isneginf(got[inf])) and np.all(np.isfinite(got[~inf]))
        assert np.abs(want[~inf]).max() < 8.0      # the magnitude the bound was derived for
        err = np.abs(got[~inf].astype(np.float64) - want[~inf]).max()
        mean = dist.mean(dim=-1, keepdim=True)
        framework = torch.log(mean if clamp is None else mean.clamp(*clamp))[:, 0].cpu().numpy()
        diff = np.abs(got[~inf].astype(np.float64) - framework[~inf]).max()
        print(f"\ninit_scales {name} k={k} dims={dims} clamp={clamp}: {err:.3e} from float64 (bound {SCALE_FLOOR:.0e}), {diff:.3e} from "
              f"torch.log(mean) (bound {2 * SCALE_FLOOR:.0e})")
        assert err <= SCALE_FLOOR and diff <= 2 * SCALE_FLOOR and np.all(np.isneginf(framework[inf]))
        if clamp is not None and name == "duplicates":
            low = mean64 <= np.float32(0.002)
            assert low.sum() >= 11 and np.all(np.abs(got[low] - np.float32(math.log(0.002))) <= abs(np.spacing(np.float32(math.log(0.002)))))
    assert torch.equal(bits(I.rigid_init_scales(x)), bits(I.init_scales(x, 3, 3, (0.002, 100.0))))


class _Gaussians:
    """What create_from_pcd reads of VanillaGaussians (vanilla.py:28-77)."""

    def __init__(self, sh_degree, ball=False, flat=False):
        self.device = torch.device("cuda")
        self.sh_degree = sh_degree
        self.ball_gaussians = ball
        self.gaussian_2d = flat

    @property
    def num_points(self):
        return self._means.shape[0]


@pytest.mark.parametrize("sh_degree,ball,flat,width", [(3, False, False, 3), (1, False, True, 2), (0, True, False, 1)])
def test_create_from_pcd_sets_the_references_parameters(I, sh_degree, ball, flat, width):
    x = dev(R.points("uniform"))
    N = len(x)
    colors = torch.rand(N, 3, generator=torch.Generator().manual_seed(1)).cuda()
    m = _Gaussians(sh_degree, ball, flat)
    torch.manual_seed(11)
    I.create_from_pcd(m, x, colors)
    want = {"_means": (N, 3), "_scales": (N, width), "_quats": (N, 4), "_features_dc": (N, 3),
            "_features_rest": (N, (sh_degree + 1) ** 2 - 1, 3), "_opacities": (N, 1)}
    for name, shape in want.items():
        p = getattr(m, name)
        assert isinstance(p, torch.nn.Parameter) and tuple(p.shape) == shape and p.dtype == torch.float32 and p.is_cuda and p.requires_grad, name
    assert torch.equal(m._means.data, x)
    # vanilla.py:82-92 restated in torch from the search's distances
    avg = I.k_nearest(x, 3)[0].mean(dim=-1, keepdim=True)
    assert (m._scales.data - torch.log(avg.repeat(1, width))).abs().max().item() <= 2 * SCALE_FLOOR
    # :94-105
    if sh_degree > 0:
        assert torch.equal(m._features_dc.data, (colors - 0.5) / 0.28209479177387814)
    else:
        assert torch.equal(m._features_dc.data, torch.logit(colors, eps=1e-10))
    assert torch.count_nonzero(m._features_rest.data).item() == 0
    assert torch.equal(m._opacities.data, torch.logit(0.1 * torch.ones(N, 1, device="cuda")))
    # basics.py:47-62: the same seed gives the reference's quaternions
    torch.manual_seed(11)
    u, v, w = torch.rand(N), torch.rand(N), torch.rand(N)
    ref = torch.stack([torch.sqrt(1 - u) * torch.sin(2 * math.pi * v), torch.sqrt(1 - u) * torch.cos(2 * math.pi * v),
                       torch.sqrt(u) * torch.sin(2 * math.pi * w), torch.sqrt(u) * torch.cos(2 * math.pi * w)], dim=-1)
    assert torch.equal(m._quats.data.cpu(), ref)
    assert (m._quats.data.norm(dim=1) - 1).abs().max().item() <= 1e-6
    again = _Gaussians(sh_degree, ball, flat)
    torch.manual_seed(11)
    I.create_from_pcd(again, x, colors)
    assert torch.equal(again._quats.data, m._quats.data) and torch.equal(bits(again._scales.data), bits(m._scales.data))


def test_install_gives_the_references_function(I):
    mod = types.ModuleType("vanilla")
    I.install(mod)
    try:
        x = R.points("two_tiles_plus_1")
        for cloud in (dev(x), torch.as_tensor(np.array(x))):      # the reference passes its means wherever they live
            d, i = mod.k_nearest_sklearn(cloud, 3)
            assert isinstance(d, np.ndarray) and isinstance(i, np.ndarray) and d.dtype == np.float32 and i.dtype == np.float32
            assert d.shape == (len(x), 3) and i.shape == (len(x), 3)
            assert R.distance_error(d, R.reference("two_tiles_plus_1", 3)[0]) <= DIST_RTOL
            assert np.array_equal(i.astype(np.int64), R.reference("two_tiles_plus_1", 3, np.float32)[1])
    finally:
        I.uninstall(mod)
    assert not hasattr(mod, "k_nearest_sklearn")


def test_errors(I):
    from bilateral_driving_amd import _lib as L
    x = dev(R.points("uniform"))
    with pytest.raises(ValueError):
        I.k_nearest(x[:3].contiguous(), 3)
    bad = x.clone()
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError):
        I.k_nearest(bad, 3)
    bad[17, 1] = float("inf")
    with pytest.raises(ValueError):
        I.init_scales(bad)
    with pytest.raises(L.BdsError):
        I.k_nearest(x.cpu(), 3)
    with pytest.raises(L.BdsError):
        I.init_scales(x.cpu())
    d, i = I.k_nearest(x[:4].contiguous(), 3)      # N = k + 1: every other point
    assert sorted(i[0].tolist()) == [1, 2, 3] and torch.isfinite(d).all()
    ws = torch.empty(64, dtype=torch.uint8, device="cuda")
    out = torch.empty(len(x), 3, device="cuda")
    args = (L.ptr(x), 3, L.ptr(out), None, None, 0, 0.0, math.inf, L.ptr(ws), ws.numel(), L.stream())
    assert L.lib().bds_knn_self(len(x), *args) == L.BDS_EWORKSPACE and L.lib().bds_knn_self(3, *args) == L.BDS_EINVAL
