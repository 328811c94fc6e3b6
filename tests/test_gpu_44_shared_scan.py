"""The shared workgroup scan (csrc/scan.h) at the count-table lengths at which a segmented scan can go wrong, through the public Python
entry of every site that uses it, and of the geometry metrics, whose kernels keep a scan of their own of the same shape.

A site counts per workgroup of R rows and scans the n = ceil(N / R) counts with ONE workgroup of T threads, thread t owning the
ceil(n / T) entries from t ceil(n / T) on (workgroup_scan_in_place).  The lengths: n = 1; T - 1 and T (every thread owns at most one
entry); T + 1 (segments of two, the upper half of the threads own nothing); 2 T + 1 (segments of three, the last one ragged).  The
rows are N = n R - 3, so that the last count is a partial workgroup's.  Every compared value that depends on a scan is an integer or a
copy of a row: equal means bit-equal."""
import numpy as np
import pytest
import torch

from oracle import gs_oracle
from tests import geometry_ref64 as GR
from tests import lidar_ref64 as LR
from tests import pvg_ref64 as PR
from tests.test_gpu_37_pvg import compare, fused

pytestmark = pytest.mark.gpu


def lengths(T):
    return [1, T - 1, T, T + 1, 2 * T + 1]


def rows(n, R):
    return n * R - 3


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    return _lib


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- geometry: depth_map_to_point_cloud ---------------------------------------------------------------------------------------------
GEO_T, GEO_R = 1024, 256      # kGeoScanBlock, kGeoBlock (csrc/geometry.hip)


@pytest.mark.parametrize("n", lengths(GEO_T))
def test_geometry_point_cloud_is_the_masked_rows_of_the_full_cloud(lib, n):
    from bilateral_driving_amd import geometry as G
    W = 253 if n > 1 else 23
    H = n * GEO_R // W      # the largest image of this width with n counts
    assert -(-H * W // GEO_R) == n and H * W % GEO_R != 0
    K, c2w = GR.camera(H, W)
    g = np.random.default_rng(n)
    depth = g.uniform(0.5, 79.0, (H, W)).astype(np.float32)
    mask = g.uniform(0, 1, (H, W)) < 0.5
    full = G.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), None)
    want = GR.unproject(depth, K, c2w, np.ones((H, W), bool), np.float64)
    tol = 4 * np.finfo(np.float32).eps * (np.abs(want).max() + 160)      # test_gpu_40's: an ulp of each term
    assert full.shape == want.shape and np.abs(full.cpu().numpy() - want).max() <= tol
    got = G.depth_map_to_point_cloud(dev(depth), dev(K), dev(c2w), dev(mask))
    keep = torch.nonzero(dev(mask).reshape(-1)).reshape(-1)
    assert got.shape == (int(mask.sum()), 3)
    assert torch.equal(bits(got), bits(full[keep]))


# ---- lidar: points_in_boxes, count / scan / emit ------------------------------------------------------------------------------------
LIDAR_T, LIDAR_R = 1024, 256      # kLidarScanBlock, kLidarBlock (csrc/lidar.hip)


def lidar_boxes():
    """Three overlapping oriented boxes around the origin: poses [1,3,4,4], sizes [3,3] float32."""
    def pose(rz, rx, t):
        cz, sz, cx, sx = np.cos(rz), np.sin(rz), np.cos(rx), np.sin(rx)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = Rz @ Rx, t
        return P
    poses = np.stack([pose(0.0, 0.0, (1.0, 0.0, 0.0)), pose(0.52, 0.0, (-2.0, 1.0, 0.5)), pose(-0.87, 0.35, (0.0, -1.0, -1.0))])[None]
    sizes = np.array([[14.0, 10.0, 8.0], [12.0, 12.0, 6.0], [9.0, 16.0, 10.0]])
    return poses.astype(np.float32), sizes.astype(np.float32)


@pytest.mark.parametrize("n", lengths(LIDAR_T))
def test_lidar_records_are_the_pairs_of_the_framework_formulation(lib, n):
    from bilateral_driving_amd import lidar as LD
    N = rows(n, LIDAR_R)
    pts = np.random.default_rng(100 + n).uniform(-10.0, 10.0, (N, 3)).astype(np.float32)
    poses, sizes = lidar_boxes()
    x, tp, ts, active = dev(pts), torch.from_numpy(poses), torch.from_numpy(sizes), torch.ones(1, 3, dtype=torch.bool)
    rec = LD.points_in_boxes(x, tp, ts, active, emit=True)
    inst, row = rec["instance"], rec["row"]
    M = row.numel()
    # (instance, frame, row) order: the kernel emits by (row, box), the entry's stable sort by box leaves each box's rows ascending
    assert bool((rec["frame"] == 0).all()) and bool((inst[1:] >= inst[:-1]).all())
    assert bool(((row[1:] > row[:-1]) | (inst[1:] > inst[:-1])).all())
    hits = [int(LD.points_in_boxes(x, tp, ts, active, instances=[b]).sum()) for b in range(3)]
    assert M == sum(hits) and min(hits) > 0
    assert [int((inst == b).sum()) for b in range(3)] == hits
    w2o, half, _ = LD.box_tables(tp, ts, active)
    w2o, half = w2o.cuda(), half.cuda()
    undecided = 0
    for b in range(3):
        o = x @ w2o[b, :, :3].T + w2o[b, :, 3]
        inside = ((o > -half[b]) & (o < half[b])).all(1)
        decided = dev(LR.in_box(poses[0, b], sizes[b], pts)[3])      # farther than MARGIN float32 errors from every face
        undecided += int((~decided).sum())
        got = torch.zeros(N, dtype=torch.bool, device="cuda")
        got[row[inst == b]] = True
        assert torch.equal(got[decided], inside[decided])
    assert undecided <= LR.CAP * max(M, 1)


# ---- periodic-vibration Gaussians: time_transform ------------------------------------------------------------------------------------
PVG_T, PVG_R = 256, 256      # kPvgBlock: the scan launch's and the row kernels' workgroup (csrc/pvg.hip)


@pytest.mark.parametrize("n", lengths(PVG_T))
def test_pvg_kept_rows_are_the_framework_masks_rows_in_order(lib, n):
    from bilateral_driving_amd import pvg as P
    N, deg = rows(n, PVG_R), 1
    d = PR.random_rows(N, 300 + n, K=4)      # about half the rows pass the marginal test
    setting = PR.SETTINGS[n % 3]
    PR.settle_clamp(d, setting, deg)
    ref = PR.run_framework(d, setting, deg, sh=gs_oracle.spherical_harmonics)
    bound, _ = PR.measured_bound(d, setting, deg, ref)
    got = fused(P, d, setting, deg)
    compare(got, ref, bound)      # test_gpu_37's check of every kept row and every gradient against float64
    cur, dt, smooth = setting
    on_dev = [d[k].cuda() for k in PR.RAW]
    fw_mask = P.framework_transform(*on_dev, d["cam_pos"].cuda(), cur, dt, smooth, PR.T, deg)[5]
    ids = torch.nonzero(fw_mask).reshape(-1)
    assert torch.equal(ids.cpu(), torch.nonzero(torch.as_tensor(got[1])).reshape(-1)) and 0.25 * N <= ids.numel() <= 0.75 * N
    assert PR.scaled_err(got[0]["scales"], np.exp(d["log_scales"].double().numpy())[ids.cpu().numpy()]) <= bound
    # the per-row math does not look at a row's position: the kept rows alone, transformed again, give the same bits at the same ranks
    *outs, _ = P.time_transform(*on_dev, d["cam_pos"].cuda(), cur, dt, smooth, PR.T, deg)
    *alone, m = P.time_transform(*[t[ids].contiguous() for t in on_dev], d["cam_pos"].cuda(), cur, dt, smooth, PR.T, deg)
    assert bool(m.all()) and all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, alone))


# ---- refinement: densify.plan -------------------------------------------------------------------------------------------------------
REF_T, REF_R = 1024, 256      # kScanThreads, kRefBlock (csrc/refine.hip)


@pytest.mark.parametrize("n", lengths(REF_T))
def test_refine_totals_and_ranks_are_the_scans_of_the_flag_bits(lib, n):
    from bilateral_driving_amd.densify import plan
    N = rows(n, REF_R)
    g = torch.Generator(device="cuda").manual_seed(500 + n)
    r = lambda *s: torch.rand(*s, generator=g, device="cuda")
    flags, ranks, totals = plan(r(N, 3) * 7.5 - 4.5, r(N, 1) * 9 - 6.5, r(N) * 0.004, torch.floor(r(N) * 6) + 1, r(N) * 0.2,
                                do_densify=True, grad_thresh=0.0003, size_thresh=0.06, split_by_screen=True, split_screen_size=0.05,
                                do_cull=True, cull_alpha_thresh=0.005, cull_by_scale=True, cull_scale_thresh=15.0, cull_by_screen=True,
                                cull_screen_size=0.15)
    bit = [((flags >> b) & 1).long() for b in range(5)]
    assert torch.equal(totals, torch.stack([b.sum() for b in bit]))
    assert all(int(t) > 0 for t in totals) or N < 1000      # every channel is exercised
    want = torch.stack([torch.cumsum(bit[b], 0) - bit[b] for b in (0, 2, 3, 4)], 1)
    assert ranks.shape == (N, 4) and torch.equal(ranks.long(), want)


# ---- scene initialisation: k_nearest ------------------------------------------------------------------------------------------------
KNN_T = 1024      # kKnnScanBlock (csrc/knn.hip); the table holds one count per grid cell and a closing zero: n = cells + 1
DIST_RTOL = 1e-6      # tests/test_gpu_41_knn_init.py


def line_cloud(N, seed):
    """N points uniform along 100 m of x, jittered by a fifth of their spacing in y and z: the grid drops the two thin axes and
    divides x into N or N + 1 cells (knn_choose_grid: edge = extent / N)."""
    g = np.random.default_rng(seed)
    w = 0.2 * 100.0 / N
    return np.stack([g.uniform(0, 100.0, N), g.uniform(0, w, N), g.uniform(0, w, N)], 1).astype(np.float32)


def check_knn(I, x, k):
    N = len(x)
    dist, idx, stats = I.k_nearest(dev(x), k, return_stats=True)
    xd = dev(x).double()
    d2 = torch.cdist(xd, xd, compute_mode="donot_use_mm_for_euclid_dist")
    d2.fill_diagonal_(float("inf"))
    want, want_i = torch.sort(d2, dim=1, stable=True)      # ties in row order: the search's (distance, row) rule
    want, want_i = want[:, :k + 1], want_i[:, :k + 1]
    zero = want[:, :k] == 0
    assert bool((dist[zero] == 0).all())
    rel = ((dist.double() - want[:, :k]).abs() / want[:, :k].clamp(min=1e-300))[~zero]
    assert rel.numel() == 0 or float(rel.max()) <= DIST_RTOL
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()) and bool((idx != torch.arange(N, device="cuda")[:, None]).all())
    # the reported rows' own distances, formed as the kernels form them (test_gpu_41's pair_f32), bit for bit
    diff = x[:, None, :] - x[idx.cpu().numpy()]
    sq = diff * diff
    assert np.array_equal(np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]).view(np.int32), dist.cpu().numpy().view(np.int32))
    # the rows themselves wherever float32 cannot reorder two candidates: every gap among the k + 1 nearest is clear, or all are 0
    gaps = (want[:, 1:] - want[:, :-1]) > 8 * DIST_RTOL * want[:, 1:]
    clear = gaps.all(1) | (want[:, :k] == 0).all(1)
    assert torch.equal(idx[clear], want_i[clear][:, :k]) and (int(clear.sum()) > 0.9 * N or N < 16)
    return stats["cells"]


def test_knn_matches_brute_force_at_cell_tables_around_the_scan_workgroup(lib):
    """A line cloud of N points gets N or N + 1 cells, whichever way its edge rounds: clouds of n - 2 and n - 1 points are tried (and
    checked, every one) until the table has the wanted length n."""
    from bilateral_driving_amd import init as I
    k = 3
    seen = {check_knn(I, np.full((k + 1, 3), 0.5, np.float32), k) + 1}      # one point repeated: one cell, the shortest table (n = 2)
    for n in (KNN_T - 1, KNN_T, KNN_T + 1, 2 * KNN_T + 1):
        for seed in range(8):
            if n in seen:
                break
            seen |= {check_knn(I, line_cloud(N, seed), k) + 1 for N in (n - 2, n - 1)}
    print(f"\nknn cell-table lengths seen: {sorted(seen)}")
    assert {2, KNN_T - 1, KNN_T, KNN_T + 1, 2 * KNN_T + 1} <= seen
    assert min(seen) - 1 < KNN_T and max(seen) - 1 > 2 * KNN_T


# ---- exchange: bds_union_slots ------------------------------------------------------------------------------------------------------
UNION_TILE, UNION_T = 4096, 256      # kUnionTile, kUnionBlock (csrc/exchange.hip): 257 tiles are more than one workgroup's threads


def union_mask(N, seed):
    return (torch.rand(N, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.uint8).cuda()


def check_union(mask, cap, row_map, ids, count):
    members = torch.nonzero(mask).reshape(-1)
    assert count == members.numel() <= cap
    assert torch.equal(ids[:count].long(), members) and bool((ids[count:] == -1).all())
    assert torch.equal(row_map.long(), (torch.cumsum(mask, 0, dtype=torch.int64) - 1).clamp(0, cap - 1))


@pytest.mark.parametrize("k", [1, 2, 257])
def test_union_slots_equal_the_framework_formulation(lib, k):
    L, l = lib, lib.lib()
    N, K = UNION_TILE * k - 5, 1
    mask = union_mask(N, k)
    cap = int(mask.sum()) + 7
    row_map = torch.empty(N, dtype=torch.int32, device="cuda")
    ids = torch.empty(cap, dtype=torch.int32, device="cuda")
    bufs = [torch.full(s, 7.0, device="cuda") for s in ((cap, 3), (cap, 4), (cap, 3), (cap,), (cap, K, 3))]
    cnt, cnt_dev = torch.zeros(1, dtype=torch.int64).pin_memory(), torch.zeros(1, dtype=torch.int64, device="cuda")
    wsb = l.bds_union_slots_workspace_bytes(N)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    L.check(l.bds_union_slots(N, L.ptr(mask), cap, K, L.ptr(row_map), L.ptr(ids), *[L.ptr(b) for b in bufs], L.ptr(ws), wsb, L.ptr(cnt_dev),
                              cnt.data_ptr(), L.stream()), "bds_union_slots")
    torch.cuda.synchronize()
    assert int(cnt[0]) == int(cnt_dev[0]) == int(mask.sum())
    check_union(mask, cap, row_map, ids, int(cnt_dev[0]))
    for b in bufs:
        assert float(b[:cap - 7].abs().max()) == 0.0 and bool((b[cap - 7:] == 7.0).all())


@pytest.mark.parametrize("k", [1, 2, 257])
def test_frame_exchange_targets_equal_the_framework_formulation(lib, k):
    """The caller in dist.py: the first frame sizes the buffers with framework operators, the second takes bds_union_slots."""
    from bilateral_driving_amd.dist import ROW_NAMES, FlatGradients, FrameExchange
    N = UNION_TILE * k - 5
    shapes = {"means": (N, 3), "quats": (N, 4), "log_scales": (N, 3), "opacity_logits": (N,), "sh": (N, 1, 3)}
    params = [torch.zeros(shapes[name], device="cuda", requires_grad=True) for name in ROW_NAMES]
    fx = FrameExchange(FlatGradients(params, sparse_rows=True), ROW_NAMES, force=True)
    mask = union_mask(N, 10 + k)
    for frame in range(2):
        fx.begin_frame()
        fx.begin_view({"radii": mask.to(torch.int32)})
        views, row_map = fx.targets(None)
        if frame == 1:
            cap = fx.cap
            assert views["means"].shape == (cap, 3)
            assert torch.equal(row_map.long(), (torch.cumsum(mask, 0, dtype=torch.int64) - 1).clamp(0, cap - 1))
            views["means"][:] = torch.arange(1, cap + 1, device="cuda", dtype=torch.float32)[:, None]
        fx.end_view()
        fx.end_frame()      # (raises if the count word says that the union outgrew the capacity)
    # the id list, through what it is for: slot s of the compact buffer is added to the row of the s-th member, no other row is touched
    members = torch.nonzero(mask).reshape(-1)
    want = torch.zeros(N, 3, device="cuda")
    want[members] = torch.arange(1, members.numel() + 1, device="cuda", dtype=torch.float32)[:, None]
    assert members.numel() <= fx.cap and torch.equal(fx.arena["means"], want)
