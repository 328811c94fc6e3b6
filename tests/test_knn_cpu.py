"""Scene initialisation's neighbour search (bilateral_driving_amd/init.py, csrc/knn.hip) on the CPU: the restatement
(tests/knn_ref64.py) against sklearn's recorded distances (tests/golden/knn) and known answers, the device math on the host
(tests/hostmath_knn_shim.hip) against that restatement, the new kernels' resources, and the C entries' signatures and argument checks.

Distances are held to a relative 1e-6 (exactly 0 where the reference is 0).  The bound is derived: three float32 differences, three
squares, two sums and a square root stay within about 3 ulp of the exact distance of the float32 coordinates, and a neighbour chosen
differently at a near-tie moves a sorted distance by no more than that; 1e-6 is about 8 ulp.  (The float32 restatement measures 1.2e-7
over these cases.)

The scale epilogue is held to twice the float32 restatement's own error against float64 plus SCALE_FLOOR, absolute in the log-scale.
The excess over twice the restatement's error was measured here over every case, both clamp forms and k = 1, 3, 8 (the test prints
each figure): 0.0 at the worst -- the shim sums the K distances one after the other and divides, as numpy's float32 mean does, and the
host's logf agrees with numpy's float32 log on these values.  The floor is therefore not a measured excess but what the device's
logarithm may add: logf is specified to 1 ulp, one float32 ulp of a log-scale of magnitude 4 .. 8 (means of 3e-4 .. 0.02 m and
55 .. 3000 m) is 4.8e-7, and a result 1 ulp off where the restatement is exact stands that far above twice its error.  SCALE_FLOOR = 1e-6 is that ulp rounded up to the next power of ten; the GPU test uses it (and measures 9.05e-7 on the MI355X: the
device's logf is about 1.5 ulp off at its worst on these values, inside the floor)."""
import ctypes
import math
import re
import types

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from tests import knn_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources, short_name

DIST_RTOL = 1e-6
SCALE_FLOOR = 1e-6
RIGID_CLAMP = (0.002, 100.0)


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)


# ---- the restatement against sklearn and known answers --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_sklearns_recorded_distances(name):
    gold = R.golden(name)
    assert sorted(gold) == sorted(R.GOLDEN_KS[name])
    for k, want in gold.items():
        d64, _ = R.reference(name, k)
        assert want.dtype == np.float32 and want.shape == d64.shape
        zero = d64 == 0
        assert np.all(want[zero] == 0), (name, k)
        worst = ulps(d64.astype(np.float32)[~zero], want[~zero]).max(initial=0.0)
        print(f"\nknn restatement {name} k={k}: worst difference from sklearn's recorded distances {worst:.2f} ulp")
        assert worst <= 1.0, (name, k, worst)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_a_fresh_sklearn_run(name):
    pytest.importorskip("sklearn")
    from sklearn.neighbors import NearestNeighbors
    x = np.array(R.points(name))
    for k in R.GOLDEN_KS[name]:
        distances, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
        want = distances[:, 1:].astype(np.float32)
        d64, _ = R.reference(name, k)
        zero = d64 == 0
        assert np.all(want[zero] == 0) and ulps(d64.astype(np.float32)[~zero], want[~zero]).max(initial=0.0) <= 1.0, (name, k)


def test_known_answers_of_the_restatement():
    for dtype in (np.float64, np.float32):
        d, i = R.reference("lattice", 3, dtype)
        assert np.all(d == 0.25)                                        # every lattice point has at least three axis neighbours
        x = R.points("lattice")
        assert np.all(np.abs(x[i] - x[:, None, :]).sum(-1) == 0.25) and np.all(np.diff(i, axis=1) > 0)      # ties: by row
        d, i = R.reference("duplicates", 3, dtype)
        assert np.all(d[:, 0] == 0) and np.all(i != np.arange(len(i))[:, None])
        x = R.points("duplicates")
        assert np.all(np.all(x[i[:, 0]] == x, axis=1))
        assert (d[:, 2] == 0).sum() == 11 and np.all(R.reference("duplicates", 8, dtype)[0][d[:, 2] == 0] == 0)      # 11 copies: > K
    assert np.isneginf(R.log_scales(R.reference("duplicates", 3)[0])).sum() == 11
    assert np.sum(R.log_scales(R.reference("duplicates", 3)[0], RIGID_CLAMP) == math.log(0.002)) >= 11
    x = R.points("clusters_outliers")
    d1 = R.reference("clusters_outliers", 1)[0][:, 0]
    assert d1[-R.OUTLIERS:].min() > 240.0 and d1[:-R.OUTLIERS].max() < 1.0 and len(x) == 2 * R.CLUSTER + R.OUTLIERS
    assert [len(R.points(n)) for n in ("n4", "query_block_minus_1", "query_block_plus_1", "two_tiles_plus_1")] == [4, 255, 257, 1025]
    e32 = max(R.distance_error(R.reference(n, k, np.float32)[0], R.reference(n, k)[0]) for n in R.CASES for k in R.GOLDEN_KS[n])
    print(f"\nknn float32 restatement: worst relative distance error {e32:.3e}")
    assert e32 <= DIST_RTOL


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("knn")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.hm_knn_pair.argtypes = [vp, vp]
    h.hm_knn_pair.restype = cf
    h.hm_knn_ordered.argtypes = [cf]
    h.hm_knn_ordered.restype = ctypes.c_uint
    h.hm_knn_from_ordered.argtypes = [ctypes.c_uint]
    h.hm_knn_from_ordered.restype = cf
    h.hm_knn_grid.argtypes = [vp, vp, ctypes.c_longlong, vp, vp]
    h.hm_knn_insert_all.argtypes = [ci, vp, vp, ci, vp, vp]
    h.hm_knn_run.argtypes = [ctypes.c_longlong, vp, ci, ci, vp, vp, vp, vp, vp, cf, cf, vp, vp]
    return h


_RUNS = {}


def shim_run(shim, name, k, clamp=None, ring_max=R.RING_MAX):
    key = (name, k, clamp, ring_max)
    if key not in _RUNS:
        x = np.array(R.points(name))
        N = len(x)
        out = {"dist": np.zeros((N, k), np.float32), "idx": np.zeros((N, k), np.int32), "ring": np.zeros(N, np.int32),
               "cells": np.zeros((N, 3), np.int32), "scale": np.zeros(N, np.float32), "grid": np.zeros(9, np.float32),
               "dims": np.zeros(3, np.int32)}
        lo, hi = (0.0, math.inf) if clamp is None else clamp
        assert shim.hm_knn_run(N, x.ctypes.data, k, ring_max, out["dist"].ctypes.data, out["idx"].ctypes.data, out["ring"].ctypes.data,
                               out["cells"].ctypes.data, out["scale"].ctypes.data, lo, hi, out["grid"].ctypes.data,
                               out["dims"].ctypes.data) == 0
        _RUNS[key] = out
    return _RUNS[key]


def test_host_pair_rounds_every_operation_on_its_own(shim):
    a, b = np.array([1000.5, -800.25, 30.0], np.float32), np.array([1000.25, -800.0, 31.0], np.float32)
    assert shim.hm_knn_pair(a.ctypes.data, b.ctypes.data) == 0.0625 + 0.0625 + 1.0      # exact: no |x|^2 + |y|^2 - 2 x.y
    g = np.random.default_rng(0)
    for _ in range(2000):      # (dx*dx + dy*dy) + dz*dz in float32, bit for bit: no fused multiply-add
        a, b = g.uniform(-50, 50, 3).astype(np.float32), g.uniform(-50, 50, 3).astype(np.float32)
        d = a - b
        assert shim.hm_knn_pair(a.ctypes.data, b.ctypes.data) == (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def test_host_ordered_encoding_keeps_the_order_and_round_trips(shim):
    v = np.array([-3.4e38, -1000.5, -1e-30, -0.0, 0.0, 1e-30, 0.25, 1000.5, 3.4e38], np.float32)
    enc = [shim.hm_knn_ordered(float(t)) for t in v]
    assert enc == sorted(enc) and len(set(enc)) == len(enc) and 0 < enc[0] and enc[-1] < 0xffffffff
    assert [shim.hm_knn_from_ordered(e) for e in enc] == [float(t) for t in v]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_host_insertion_does_not_depend_on_the_order_of_the_candidates(shim, k):
    g = np.random.default_rng(k)
    d2 = (g.integers(0, 6, 60) * 0.5).astype(np.float32)      # many ties: the index decides
    ids = g.permutation(1000)[:60].astype(np.int32)
    want = sorted(zip(d2.tolist(), ids.tolist()))[:k]
    for _ in range(20):
        p = g.permutation(60)
        a, b = np.ascontiguousarray(d2[p]), np.ascontiguousarray(ids[p])
        od, oi = np.zeros(k, np.float32), np.zeros(k, np.int32)
        assert shim.hm_knn_insert_all(k, a.ctypes.data, b.ctypes.data, 60, od.ctypes.data, oi.ctypes.data) == 0
        assert list(zip(od.tolist(), oi.tolist())) == want
    od, oi = np.zeros(k, np.float32), np.zeros(k, np.int32)
    shim.hm_knn_insert_all(k, d2.ctypes.data, ids.ctypes.data, max(k - 1, 0), od.ctypes.data, oi.ctypes.data)      # fewer than K
    assert np.all(np.isinf(od[max(k - 1, 0):])) and list(od[:k - 1]) == sorted(d2[:k - 1].tolist())


def test_host_grid_choice_respects_the_cell_cap_and_degenerate_axes(shim):
    def grid(lo, hi, N):
        lo, hi = np.array(lo, np.float32), np.array(hi, np.float32)
        g, d = np.zeros(6, np.float32), np.zeros(3, np.int32)
        shim.hm_knn_grid(lo.ctypes.data, hi.ctypes.data, N, g.ctypes.data, d.ctypes.data)
        return float(g[0]), [int(v) for v in d]
    for lo, hi, N in (((0, 0, 0), (100, 100, 100), 1500), ((1000, -2000, 5), (1200, -1997, 5.01), 1200), ((0, 0, 1.5), (40, 40, 1.5), 800),
                      ((0, 0, 0), (1000, 1e-6, 1e-6), 10), ((-400, -400, -400), (400, 400, 400), 4), ((0, 0, 0), (1, 1, 1), 1 << 30),
                      ((0, 0, 0), (3e38, 1, 1), 100), ((-3e38, 0, 0), (3e38, 1, 1), 100), ((2, 2, 2), (2, 2, 2), 50)):
        edge, dims = grid(lo, hi, N)
        assert all(d >= 1 for d in dims) and dims[0] * dims[1] * dims[2] <= max(1, 2 * N) and edge > 0, (lo, hi, N, edge, dims)
        for a in range(3):
            if hi[a] == lo[a]:
                assert dims[a] == 1
            elif dims[a] > 1 and math.isfinite(hi[a] - lo[a]):
                assert (dims[a] - 1) * edge <= (hi[a] - lo[a]) * (1 + 1e-6)      # the cells do not run past the box by a whole cell
    assert grid((0, 0, 0), (100, 100, 100), 1500)[1] == [12, 12, 12] and grid((2, 2, 2), (2, 2, 2), 50)[1] == [1, 1, 1]
    assert grid((-3e38, 0, 0), (3e38, 1, 1), 100)[1] == [1, 1, 1]      # an extent beyond float32: one cell, every query brute force


CASE_KS = [(n, k) for n in R.CASES for k in R.GOLDEN_KS[n]]


def must_be_unresolved(x, lo, hi, edge, dims, nearest):
    """The points that no ring can resolve, from the grid alone: on some axis with more than 2 RING_MAX + 1 cells the point lies more
    than RING_MAX + 1 edges inside both faces of the grid's box, so neither face of its last cube on that axis is a face of the grid
    and the margin is at most (RING_MAX + 1) edges -- and its nearest neighbour is farther than that."""
    reach = (R.RING_MAX + 1) * np.float64(edge)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    inside = (x > lo + reach) & (x < hi - reach) & (np.asarray(dims) > 2 * R.RING_MAX + 1)
    return inside.any(1) & (nearest > reach * 1.001)


@pytest.mark.parametrize("name,k", CASE_KS)
def test_host_search_matches_float64_at_every_point(shim, name, k):
    out = shim_run(shim, name, k)
    d64, i64 = R.reference(name, k)
    err, e32 = R.distance_error(out["dist"], d64), R.distance_error(R.reference(name, k, np.float32)[0], d64)
    unresolved = int((out["ring"] < 0).sum())
    print(f"\nknn shim {name} k={k}: float32 restatement {e32:.3e}, shim {err:.3e}, bound {DIST_RTOL:.0e}; grid {out['dims'].tolist()} edge "
          f"{out['grid'][0]:.4g}; resolved at ring 0 / 1 / 2: {[int((out['ring'] == r).sum()) for r in range(3)]}, fallback {unresolved}")
    assert err <= DIST_RTOL, (name, k, err)
    assert np.all(np.diff(out["dist"], axis=1) >= 0)
    N = len(d64)
    assert np.all(out["idx"] != np.arange(N)[:, None]) and out["idx"].min() >= 0 and out["idx"].max() < N
    assert all(len(set(row)) == k for row in out["idx"].tolist())
    # the float32 twin restates the same arithmetic and the same order: equal bit for bit, rows included
    d32, i32 = R.reference(name, k, np.float32)
    assert np.array_equal(out["dist"], d32) and np.array_equal(out["idx"], i32)
    if name == "lattice":
        assert np.array_equal(out["idx"], i64)      # d2 is exact there, so the tie rule decides
    dims = out["dims"]
    assert dims.min() >= 1 and int(dims[0]) * int(dims[1]) * int(dims[2]) <= 2 * N
    if name == "clusters_outliers":
        must = must_be_unresolved(R.points(name), out["grid"][3:6], out["grid"][6:9], out["grid"][0], dims, R.reference(name, k)[0][:, 0])
        assert must[:-R.OUTLIERS].sum() == 0 and must[-R.OUTLIERS:].sum() > 0 and np.all(out["ring"][must] < 0)


@pytest.mark.parametrize("name,k", CASE_KS)
def test_host_termination_test_never_resolves_too_early(shim, name, k):
    """For every query resolved at ring r, no point outside the cube of cells within r of its cell is closer than its K-th distance
    in float64.  Also with the ring limit lifted, so that the outer rings are tested too."""
    x = R.points(name).astype(np.float64)
    kth = R.reference(name, k)[0][:, -1]
    for ring_max in (R.RING_MAX, 64):
        out = shim_run(shim, name, k, None, ring_max)
        cells, ring = out["cells"].astype(np.int64), out["ring"]
        assert np.all((cells >= 0) & (cells < out["dims"]))
        checked = 0
        for i in np.nonzero(ring >= 0)[0]:
            outside = np.abs(cells - cells[i]).max(1) > ring[i]
            if outside.any():
                d = np.sqrt(((x[outside] - x[i]) ** 2).sum(1)).min()
                assert d >= kth[i], (name, k, int(i), int(ring[i]), d, kth[i])
                checked += 1
        if ring_max == 64:
            assert np.all(ring >= 0) or int(out["dims"].max()) > 64      # every cube ends by covering the grid
            assert R.distance_error(out["dist"], R.reference(name, k)[0]) <= DIST_RTOL
        print(f"\nknn termination {name} k={k} ring limit {ring_max}: {checked} queries with points outside their cube, "
              f"{int((ring < 0).sum())} unresolved, deepest ring {int(ring.max())}")


@pytest.mark.parametrize("clamp", [None, RIGID_CLAMP])
def test_host_scale_epilogue_is_within_the_bound(shim, clamp):
    worst = (-math.inf, None)
    for name, k in CASE_KS:
        out = shim_run(shim, name, k, clamp)
        s64 = R.log_scales(R.reference(name, k)[0], clamp)
        s32 = R.log_scales(R.reference(name, k, np.float32)[0], clamp, np.float32)
        got = out["scale"]
        inf = np.isneginf(s64)
        assert np.all(np.isneginf(got[inf])) and np.all(np.isfinite(got[~inf])) and np.all(np.isfinite(s64[~inf])), (name, k)
        if clamp is None and name == "duplicates":
            assert inf.sum() == (len(s64) if k == 1 else 11)      # k = 1: every point has a copy; k = 3, 8: the point present 11 times
        if clamp is not None:
            assert not inf.any()
            low = R.reference(name, k)[0].mean(1) <= clamp[0]
            assert np.all(np.abs(got[low] - np.float32(math.log(0.002))) <= abs(np.spacing(np.float32(math.log(0.002))))), (name, k)
        err = np.abs(got[~inf].astype(np.float64) - s64[~inf]).max(initial=0.0)
        e32 = np.abs(s32[~inf].astype(np.float64) - s64[~inf]).max(initial=0.0)
        print(f"knn scale {name} k={k} clamp={clamp}: float32 restatement {e32:.3e}, shim {err:.3e}, excess {err - 2 * e32:.3e}")
        worst = max(worst, (err - 2 * e32, f"{name} k={k}"))
        assert err <= 2 * e32 + SCALE_FLOOR, (name, k, err, e32)
    print(f"\nknn scale epilogue clamp={clamp}: worst excess over twice the float32 restatement's error {worst[0]:.3e} ({worst[1]}); "
          f"SCALE_FLOOR {SCALE_FLOOR:.1e}")
    assert worst[0] <= SCALE_FLOOR


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_knn_kernel_resources():
    res = {short_name(k): v for k, v in kernel_resources("knn.hip").items()}
    want = ["knn_clear_kernel", "knn_bounds_kernel", "knn_hist_kernel", "knn_trim_kernel", "knn_count_kernel", "knn_scan_kernel",
            "knn_scatter_kernel"]
    want += [f"knn_{w}_kernel<{k}>" for w in ("query", "fallback") for k in range(1, 9)]
    assert sorted(res) == sorted(want), list(res)
    for k in want:
        print(f"\n{k}: occupancy {res[k]['Occupancy']} waves/SIMD, {res[k]['VGPRs']} VGPRs, LDS {res[k]['LDS Size']} bytes")
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["LDS Size"] <= 16 * 1024, (k, res[k])
        assert res[k]["Occupancy"] >= 4, (k, res[k])
    from bilateral_driving_amd import init
    assert res["knn_fallback_kernel<3>"]["LDS Size"] == 16 * init.TARGET_TILE


def test_entries_resolve_with_the_declared_signatures():
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_knn\w*", k)}
    assert sorted(decl) == ["bds_knn_self", "bds_knn_workspace_bytes"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    from bilateral_driving_amd import init
    for macro, value in (("BDS_KNN_MAX_K", init.MAX_K), ("BDS_KNN_MAX_POINTS", init.MAX_POINTS), ("BDS_KNN_QUERY_BLOCK", init.QUERY_BLOCK),
                         ("BDS_KNN_TARGET_TILE", init.TARGET_TILE), ("BDS_KNN_RING_MAX", init.RING_MAX),
                         ("BDS_KNN_STATS_WORDS", init.STATS_WORDS), ("BDS_KNN_STAT_EDGE", init.STAT_EDGE), ("BDS_KNN_STAT_DIMS", init.STAT_DIMS),
                         ("BDS_KNN_STAT_UNRESOLVED", init.STAT_UNRESOLVED), ("BDS_KNN_STAT_LO", init.STAT_LO),
                         ("BDS_KNN_STAT_HI", init.STAT_HI), ("BDS_KNN_STAT_CELLS", init.STAT_CELLS),
                         ("BDS_KNN_STAT_CLOUD_LO", init.STAT_CLOUD_LO), ("BDS_KNN_STAT_CLOUD_HI", init.STAT_CLOUD_HI)):
        assert f"#define {macro} {value}\n" in hdr, macro
    assert (R.QUERY_BLOCK, R.TARGET_TILE, R.RING_MAX) == (init.QUERY_BLOCK, init.TARGET_TILE, init.RING_MAX)
    assert init.MAX_POINTS <= 2 ** 31 - 1
    assert lib.bds_abi_version() == L.ABI_VERSION == 7 and "#define BDS_ABI_VERSION 7 " in hdr


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first
    inf, nan = math.inf, math.nan

    def run(N=100, x=p, K=3, dist=p, idx=p, ls=p, S=3, lo=0.0, hi=inf, ws=p, nb=1 << 40):
        return lib.bds_knn_self(N, x, K, dist, idx, ls, S, lo, hi, ws, nb, None)

    for K in (0, -1, 9, 100):
        assert run(K=K) == L.BDS_EINVAL, K
    for N, K in ((3, 3), (1, 1), (0, 1), (-5, 3), (8, 8), ((1 << 30) + 1, 3), (1 << 40, 3)):
        assert run(N=N, K=K) == L.BDS_EINVAL, (N, K)
    for N in (-1, 0, 1, (1 << 30) + 1, 1 << 40):
        assert lib.bds_knn_workspace_bytes(N) == 0, N
    for name in ("x", "dist", "ws"):
        assert run(**{name: None}) == L.BDS_EINVAL, name
    for name in ("x", "dist", "idx", "ls"):
        assert run(**{name: p + 2}) == L.BDS_EINVAL, name
    assert run(ws=p + 8) == L.BDS_EINVAL
    for S in (0, 4, -1):
        assert run(S=S) == L.BDS_EINVAL, S
    assert run(lo=1.0, hi=0.5) == L.BDS_EINVAL and run(lo=nan) == L.BDS_EINVAL and run(hi=nan) == L.BDS_EINVAL
    assert run(lo=nan, hi=nan) == L.BDS_EINVAL
    need = lib.bds_knn_workspace_bytes(100)
    assert need >= 64 + 100 * 28 and run(nb=need - 1) == L.BDS_EWORKSPACE and run(nb=0) == L.BDS_EWORKSPACE
    assert run(N=4, nb=lib.bds_knn_workspace_bytes(4) - 1) == L.BDS_EWORKSPACE      # N = K + 1 is accepted
    assert run(ls=None, S=0, lo=nan, hi=nan, nb=need - 1) == L.BDS_EWORKSPACE       # without log_scales, S and the clamps are not read
    assert run(idx=None, ls=None, nb=need - 1) == L.BDS_EWORKSPACE
    big = lib.bds_knn_workspace_bytes(2_000_000)
    assert 2_000_000 * 28 <= big <= 2_000_000 * 28 + 65536 and lib.bds_knn_workspace_bytes(1 << 30) > (1 << 30) * 28


def test_python_checks_arguments_and_refuses_cpu_tensors():
    from bilateral_driving_amd import init
    import bilateral_driving_amd
    assert bilateral_driving_amd.init is init
    x = torch.rand(10, 3)
    with pytest.raises(L.BdsError):
        init.k_nearest(x, 3)
    with pytest.raises(L.BdsError):
        init.init_scales(x)
    with pytest.raises(ValueError):
        init.k_nearest(torch.rand(3, 3), 3)           # N < k + 1, as sklearn: before anything touches a device
    for bad_k in (0, 9, 2.0):
        with pytest.raises(ValueError):
            init.k_nearest(x, bad_k)
    for bad in (torch.rand(10, 2), torch.rand(10), torch.rand(2, 5, 3)):
        with pytest.raises(ValueError):
            init.k_nearest(bad, 3)
    with pytest.raises(ValueError):
        init.init_scales(x, dims=4)
    with pytest.raises(ValueError):
        init.init_scales(x, clamp=(1.0, 0.5))
    a, b = types.ModuleType("vanilla"), types.ModuleType("rigid")
    former = a.k_nearest_sklearn = lambda x, k: None
    init.install(a, b)
    init.install(a)                                   # (twice: the former function is still the one remembered)
    assert a.k_nearest_sklearn is init.k_nearest_sklearn and b.k_nearest_sklearn is init.k_nearest_sklearn
    init.uninstall(a, b)
    assert a.k_nearest_sklearn is former and not hasattr(b, "k_nearest_sklearn")
    init.install(b)
    init.uninstall()
    assert not hasattr(b, "k_nearest_sklearn")
    torch.manual_seed(7)
    q1 = init.random_quat_tensor(5)
    torch.manual_seed(7)
    u, v, w = torch.rand(5), torch.rand(5), torch.rand(5)      # basics.py:51-53: the reference's three draws, in its order
    assert torch.equal(q1[:, 0], torch.sqrt(1 - u) * torch.sin(2 * math.pi * v)) and torch.equal(q1[:, 3], torch.sqrt(u) * torch.cos(2 * math.pi * w))
    assert torch.allclose(q1.norm(dim=1), torch.ones(5), atol=1e-6)
