"""Restatement of the reference's neighbour search for scene initialisation (models/gaussians/basics.py:208-224 k_nearest_sklearn:
sklearn's NearestNeighbors over k + 1 neighbours, first column dropped) for the tests of bilateral_driving_amd/init.py: a numpy brute
force in float64, and a float32 twin that rounds as the kernels do -- coordinate differences, (dx*dx + dy*dy) + dz*dz, a square root.
Candidates are ordered by (d2, row) with the query itself excluded BY ROW, so a duplicate of a point is its neighbour at distance 0.

tests/golden/knn/<case>.npz hold sklearn 1.7.2's own distances for CASES (scripts/gen_golden_knn.py), which pin this restatement on
machines without sklearn."""
import functools
import os

import numpy as np

QUERY_BLOCK = 256       # include/bds.h BDS_KNN_QUERY_BLOCK
TARGET_TILE = 512       # include/bds.h BDS_KNN_TARGET_TILE
RING_MAX = 2            # include/bds.h BDS_KNN_RING_MAX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn")
OUTLIERS = 37
CLUSTER = 700


def _uniform(seed, n, side=100.0):
    return np.random.default_rng(seed).uniform(0.0, side, (n, 3)).astype(np.float32)


def _clusters_outliers(seed):
    """Two tight clusters 300 m apart and OUTLIERS points over +-400 m: jittered slots of a 4 x 4 x 4 lattice of pitch 800 / 3 m
    without its inner eight, so every outlier lies more than 240 m from every other point (test_gpu_41 checks it against the grid)."""
    g = np.random.default_rng(seed)
    a = g.normal(0.0, 0.05, (CLUSTER, 3)) + (-150.0, 0.0, 0.0)
    b = g.normal(0.0, 0.05, (CLUSTER, 3)) + (150.0, 0.0, 0.0)
    ticks = np.array([-400.0, -400.0 / 3, 400.0 / 3, 400.0])
    slots = np.array([(x, y, z) for x in ticks for y in ticks for z in ticks if max(abs(x), abs(y), abs(z)) > 200.0])
    out = slots[g.permutation(len(slots))[:OUTLIERS]] + g.uniform(-10.0, 10.0, (OUTLIERS, 3))
    return np.concatenate([a, b, out]).astype(np.float32)      # the outliers are the last OUTLIERS rows


def _duplicates(seed):
    g = np.random.default_rng(seed)
    p = g.uniform(0.0, 10.0, (101, 3)).astype(np.float32)
    x = np.concatenate([p[:100], p[:100], np.repeat(p[100:], 11, 0)])
    return np.ascontiguousarray(x[g.permutation(len(x))])


def _flat_far(seed):
    g = np.random.default_rng(seed)
    return (g.uniform(0.0, 1.0, (1200, 3)) * (200.0, 3.0, 0.01) + (1000.0, -2000.0, 5.0)).astype(np.float32)


def _lattice(seed):
    t = np.arange(11, dtype=np.float32) * np.float32(0.25)
    x = np.stack(np.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(x[np.random.default_rng(seed).permutation(len(x))])


def _planar(seed):
    x = _uniform(seed, 800, 40.0)
    x[:, 2] = np.float32(1.5)
    return x


def _collinear(seed):
    t = np.random.default_rng(seed).uniform(-30.0, 30.0, 500)
    return (t[:, None] * (1.0, 2.0, -0.5) + (3.0, -7.0, 2.0)).astype(np.float32)


def _heavy_tail(seed):
    """1200 points in a 20 m cube and 150 at inverse-uniform distances of up to 2 km from it (the sky's stand-ins of a street scene,
    models/trainers/scene_graph.py:165-176): the cloud's box is a hundred times the box that holds nine points in ten."""
    g = np.random.default_rng(seed)
    v = g.normal(size=(150, 3))
    far = 10.0 + v / np.linalg.norm(v, axis=1, keepdims=True) * (10.0 / g.uniform(0.005, 1.0, (150, 1)))
    x = np.concatenate([g.uniform(0.0, 20.0, (1200, 3)), far])
    return np.ascontiguousarray(x[g.permutation(len(x))].astype(np.float32))


CASES = {
    "uniform": lambda: _uniform(1, 1500),
    "clusters_outliers": lambda: _clusters_outliers(2),
    "duplicates": lambda: _duplicates(3),
    "flat_far": lambda: _flat_far(4),
    "lattice": lambda: _lattice(5),
    "planar": lambda: _planar(6),
    "collinear": lambda: _collinear(7),
    "heavy_tail": lambda: _heavy_tail(12),
    "n4": lambda: _uniform(8, 4, 2.0),
    "query_block_minus_1": lambda: _uniform(9, QUERY_BLOCK - 1, 20.0),
    "query_block_plus_1": lambda: _uniform(10, QUERY_BLOCK + 1, 20.0),
    "two_tiles_plus_1": lambda: _uniform(11, 2 * TARGET_TILE + 1, 30.0),
}
# (case, k) of the goldens and of the GPU tests: k = 3 everywhere (the reference's), k = 1 and 8 where the issue asks
GOLDEN_KS = {name: (3,) for name in CASES}
GOLDEN_KS["uniform"] = GOLDEN_KS["duplicates"] = (1, 3, 8)


@functools.lru_cache(maxsize=None)
def points(name):
    x = CASES[name]()
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 3 and np.isfinite(x).all()
    x.setflags(write=False)
    return x


def knn(x, k, dtype=np.float64):
    """-> (distances [N,k] of ``dtype``, ascending; rows [N,k] int64), ordered by (d2, row), the query's own row excluded."""
    x = np.asarray(x, np.float32).astype(dtype)
    d = x[:, None, :] - x[None, :, :]
    sq = d * d
    d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
    np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]      # stable: equal d2 keep their row order
    return np.sqrt(np.take_along_axis(d2, order, 1)).astype(dtype), order


@functools.lru_cache(maxsize=None)
def reference(name, k, dtype=np.float64):
    d, i = knn(points(name), k, dtype)
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


def log_scales(dist, clamp=None, dtype=np.float64):
    """vanilla.py:85-92 (clamp None) / rigid.py:117-119 (clamp (0.002, 100)): log of the (clamped) mean distance, [N]."""
    m = np.asarray(dist).astype(dtype).mean(-1, dtype=dtype)
    if clamp is not None:
        m = np.clip(m, dtype(clamp[0]), dtype(clamp[1]))
    with np.errstate(divide="ignore"):
        return np.log(m)


def distance_error(got, want):
    """Worst relative error of the sorted distances; inf where the reference is 0 and the result is not."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    if np.any(got[zero] != 0):
        return np.inf
    return float(np.max(np.abs(got[~zero] - want[~zero]) / want[~zero], initial=0.0))


def golden(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {int(key[1:]): z[key] for key in z.files}
