"""The pseudo-lidar generation (bilateral_driving_amd/pseudo_lidar.py, csrc/pseudo_lidar.hip) on the CPU: the float64 restatement
(tests/pseudo_lidar_ref64.py) against the reference's recorded results (tests/golden/pseudo_lidar.npz,
scripts/gen_golden_pseudo_lidar.py), the device math on the host (tests/hostmath_pseudo_lidar_shim.hip) against both, the kernels'
resources, and the C entries' signatures and argument checks.

What is compared how.  Every golden pixel and cloud row is DECIDED (pseudo_lidar_ref64: no float32 rounding of either route, nor the
double rounding of the angles, can move it across a crop face, a fov limit or a beam edge), so the counts and the emitted winners
(``source``) must be EQUAL, in beam order; coordinates are held to the derived bounds -- the reference's recorded value within e_ref
of the restatement, the shim's within e_dev of it and within e_dev + e_ref of the recorded value -- and a cloud's rows bit for bit.
Random cases leave out the beams an undecided pixel can reach with an index above the beam's decided winner (dirty beams), under the
caps of at most 1 % of a case's live pixels undecided and at most 2 % of its occupied beams dirty, asserted per case; every emitted
coordinate, dirty beam or not, is still held to e_dev of its own source pixel.

One test here needs nothing of the product: the check that every random seed stays within the caps runs on the restatement alone."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from tests import pseudo_lidar_ref64 as R
from tests.util import build_shim, declared_signatures, header, kernel_resources, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH_NAMES = tuple(R.GOLDEN_DEPTH)


def module():
    from bilateral_driving_amd import pseudo_lidar
    return pseudo_lidar


# ---- the restatement against the reference's recorded results -----------------------------------------------------------------------
@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_restatement_equals_the_references_depth_cases(name):
    z, case = R.golden(), R.golden_depth_case(name)
    ref = R.depth_reference(case)
    assert ref["decided"].all() and not ref["dirty"].any()
    gold, src = z[f"{name}_points"], z[f"{name}_source"]
    assert gold.dtype == np.float64 and gold.shape == (len(ref["emitted"]), 3)
    assert np.array_equal(src, ref["emitted"])
    assert np.all(np.abs(gold - ref["p"][src]) <= ref["e_ref"][src])
    per_beam = np.bincount(ref["cell"][ref["live"]], minlength=case["H"] * case["W"])
    occupied, collided = int((per_beam > 0).sum()), int((per_beam > 1).sum())
    print(f"\npseudo-lidar {name}: {int(ref['live'].sum())} live pixels, {occupied} occupied beams, {collided} with collisions, "
          f"{len(src)} emitted")
    assert collided > occupied // 3      # heavy collisions
    # the cases hold what they were built to hold
    d = case["depth"]
    with np.errstate(invalid="ignore"):
        assert (d == 0).sum() > 10 and (d >= 80).sum() > 10 and np.isnan(d).any() and np.isinf(d).any() and (d < 0).any()
    assert (ref["valid"] & ~ref["live"]).sum() > 50      # outside the crop or the fov
    if name == "side":
        assert (ref["valid"] & (ref["p"][:, 0] < 0)).sum() > 50
        col = ref["cell"][ref["live"]] % case["W"]
        az = np.arctan2(ref["p"][ref["live"], 1], ref["p"][ref["live"], 0])
        assert ((az > np.radians(45.5)) & (col == 0)).sum() > 50      # beyond +45 degrees: clamped into column 0, not dropped
    if name == "slice":
        assert case["slice"] == 2 and case["H"] == 9 and case["downscale"] == 2
        rows = ref["cells"] // case["W"]
        assert np.all(rows % 2 == 0) and len(np.unique(rows)) >= 2 and (ref["winner"].reshape(9, -1)[1::2] >= 0).any()


def test_restatement_equals_the_references_cloud_case():
    z, case = R.golden(), R.golden_cloud_case()
    ref = R.cloud_reference(case)
    assert ref["decided"].all() and np.array_equal(z["cloud_source"], ref["emitted"])
    assert np.array_equal(z["cloud_out"], case["cloud"][ref["emitted"]])      # rows copied: intensity too
    assert (~ref["live"]).sum() > 100 and len(ref["emitted"]) > 500
    keep = z["cloud_vertical_keep"]      # pto_ang_map_vertical called directly, no crop
    vref = R.cloud_reference(dict(case, cloud=case["cloud"][keep], mode="vertical", crop=None, H=16))
    assert vref["decided"].all() and np.array_equal(np.nonzero(keep)[0][vref["emitted"]], z["cloud_vertical_source"])


def test_every_random_seed_stays_within_the_caps_for_the_restatement_alone():
    worst = [0.0, 0.0]
    some_dirty = 0
    for seed in R.RANDOM_SEEDS:
        ref = R.depth_reference(R.random_case(seed), "device")
        und, dirty, live, occ = R.case_stats(ref)
        worst = [max(worst[0], und), max(worst[1], dirty)]
        some_dirty += dirty > 0
        assert und <= R.CAP_UNDECIDED and dirty <= R.CAP_DIRTY and live > 5000 and occ > 200, (seed, und, dirty, live, occ)
    print(f"\npseudo-lidar random cases: at worst {worst[0]:.4%} of the live pixels undecided (cap {R.CAP_UNDECIDED:.0%}), "
          f"{worst[1]:.4%} of the occupied beams dirty (cap {R.CAP_DIRTY:.0%})")
    assert some_dirty >= 2 and len(R.RANDOM_SEEDS) == 6      # the exclusion of dirty beams is exercised


# ---- the device math on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("pseudo_lidar")
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    h.hm_pl_pixel.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.c_float, vp]
    h.hm_pl_point.argtypes = [vp, ci, ci, ci, ci, vp]
    h.hm_pl_from_depth.argtypes = [ci, ci, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]
    h.hm_pl_from_depth.restype = None
    h.hm_pl_from_points.argtypes = [ll, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    h.hm_pl_from_points.restype = None
    return h


def shim_depth(shim, case):
    """One camera of a case through the shim, with the tables the product's Python layer forms.  -> points [cap,3], count, source."""
    P = module()
    cams = P.camera_table(torch.from_numpy(case["K"])[None], torch.from_numpy(case["c2w"])[None], torch.from_numpy(case["l2w"]),
                          case["downscale"]).numpy()
    beams = P.beam_table(case["H"], case["W"], case["mode"])
    Hi, Wi = case["depth"].shape
    H, W, s = case["H"], case["W"], case["slice"]
    cap = -(-H // s) * W
    d = np.ascontiguousarray(case["depth"])
    winner, points = np.zeros(H * W, np.int32), np.zeros((cap, 3), np.float32)
    counts, source = np.zeros(1, np.int32), np.zeros(cap, np.int32)
    shim.hm_pl_from_depth(1, Hi, Wi, d.ctypes.data, cams.ctypes.data, beams.ctypes.data, H, W, s, P._MODES[case["mode"]], winner.ctypes.data,
                          points.ctypes.data, counts.ctypes.data, source.ctypes.data)
    return points, int(counts[0]), source


def shim_cloud(shim, case):
    P = module()
    beams = P.beam_table(case["H"], case["W"], case["mode"], crop=case["crop"])
    H, W, s = case["H"], case["W"], case["slice"]
    cap = -(-H // s) * W
    x = np.ascontiguousarray(case["cloud"])
    winner, points = np.zeros(H * W, np.int32), np.zeros((cap, 4), np.float32)
    counts, source = np.zeros(1, np.int32), np.zeros(cap, np.int32)
    shim.hm_pl_from_points(len(x), x.ctypes.data, beams.ctypes.data, int(case["crop"] is not None), H, W, s, P._MODES[case["mode"]],
                           winner.ctypes.data, points.ctypes.data, counts.ctypes.data, source.ctypes.data)
    return points, int(counts[0]), source


@pytest.mark.parametrize("name", DEPTH_NAMES)
def test_host_generation_equals_the_reference(shim, name):
    z, case = R.golden(), R.golden_depth_case(name)
    ref = R.depth_reference(case)
    points, count, source = shim_depth(shim, case)
    assert count == len(z[f"{name}_source"]) and np.array_equal(source[:count], z[f"{name}_source"])
    stats = R.compare(ref, points, count, source, label=name)
    err = np.abs(points[:count].astype(np.float64) - z[f"{name}_points"])
    src = source[:count]
    assert np.all(err <= ref["e_dev"][src] + ref["e_ref"][src])
    print(f"\npseudo-lidar shim {name}: {stats}; against the reference's float64 output at most {err.max():.2e} m")


def test_host_cloud_generation_equals_the_reference(shim):
    z, case = R.golden(), R.golden_cloud_case()
    points, count, source = shim_cloud(shim, case)
    assert count == len(z["cloud_source"]) and np.array_equal(source[:count], z["cloud_source"])
    assert np.array_equal(points[:count].view(np.int32), z["cloud_out"].view(np.int32))      # intensities too, bit for bit
    keep = z["cloud_vertical_keep"]
    points, count, source = shim_cloud(shim, dict(case, cloud=case["cloud"][keep], mode="vertical", crop=None, H=16))
    assert np.array_equal(np.nonzero(keep)[0][source[:count]], z["cloud_vertical_source"])


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_host_generation_matches_the_restatement_on_random_cases(shim, seed):
    case = R.random_case(seed)
    ref = R.depth_reference(case, "device")
    und, dirty, _, _ = R.case_stats(ref)
    assert und <= R.CAP_UNDECIDED and dirty <= R.CAP_DIRTY
    stats = R.compare(ref, *shim_depth(shim, case), label=f"seed {seed}")
    print(f"\npseudo-lidar shim seed {seed}: {stats}")


def test_host_unprojection_rounds_every_operation_on_its_own(shim):
    g = np.random.default_rng(0)
    beams = module().beam_table(16, 32, crop=None)
    f = np.float32
    for _ in range(2000):
        cam = np.concatenate([g.uniform(50, 120, 2), g.uniform(20, 90, 2), g.uniform(-1, 1, 12)]).astype(np.float32)
        cam[[7, 11, 15]] = g.uniform(-300, 300, 3).astype(np.float32)
        u, v, d = int(g.integers(0, 160)), int(g.integers(0, 96)), f(g.uniform(0.1, 79.0))
        p = np.zeros(3, np.float32)
        shim.hm_pl_pixel(cam.ctypes.data, beams.ctypes.data, 16, 32, 1, u, v, float(d), p.ctypes.data)
        pc = [f(f(f(u) - cam[2]) * d) / cam[0], f(f(f(v) - cam[3]) * d) / cam[1], d]      # float32, in the reference's order
        want = [f(f(f(f(cam[4 + 4 * r] * pc[0]) + f(cam[5 + 4 * r] * pc[1])) + f(cam[6 + 4 * r] * pc[2])) + cam[7 + 4 * r]) for r in range(3)]
        assert np.array_equal(p, np.array(want, np.float32))      # no fused multiply-add


def test_host_known_answers(shim):
    P = module()
    H, W = 16, 32

    def point(p, mode="vertical", fov=(10.0, -30.0), crop=None):
        beams = P.beam_table(H, W, mode, fov, crop)
        q = np.array(list(p) + [0.5], np.float32)
        return shim.hm_pl_point(beams.ctypes.data, int(crop is not None), H, W, P._MODES[mode], q.ctypes.data), beams

    def cell_of(t_row, t_col):
        return int(min(max(t_row, 0.0), H - 1.0)) * W + int(min(max(t_col, 0.0), W - 1.0))
    # d == 0: both radii become 1e-6, both angles 0 -- the same double quotients here as there
    got, b = point((0.0, 0.0, 0.0))
    assert got == cell_of((0.0 - b[2]) / b[4], b[0] / b[1]) and got >= 0
    got, b = point((0.0, 0.0, 0.0), "classic")
    assert got == cell_of(b[2] / b[4], b[0] / b[1])
    # r == 0: straight up / down; the vertical rule drops it, the classic rule clamps the row
    assert point((0.0, 0.0, 2.0))[0] == -1 and point((0.0, 0.0, -2.0))[0] == -1
    got, b = point((0.0, 0.0, 2.0), "classic")
    assert got == 0 * W + int(b[0] / b[1])
    assert point((0.0, 0.0, -2.0), "classic")[0] == (H - 1) * W + int(b[0] / b[1])
    # theta exactly at a fov limit is kept (asin(0) = 0 = rad(0)), the next float beyond it is not
    tiny = float(np.float32(1e-6))
    got, b = point((3.0, 1.0, 0.0), fov=(10.0, 0.0))
    assert got >= 0 and got // W == 0
    assert point((3.0, 1.0, -tiny), fov=(10.0, 0.0))[0] == -1 and point((3.0, 1.0, tiny), fov=(10.0, 0.0))[0] // W == 0
    got, b = point((3.0, 1.0, 0.0), fov=(0.0, -30.0))
    assert got >= 0 and got // W == H - 1      # (theta - down) / dtheta = H: clamped
    assert point((3.0, 1.0, tiny), fov=(0.0, -30.0))[0] == -1 and point((3.0, 1.0, -tiny), fov=(0.0, -30.0))[0] // W == H - 1
    # azimuth beyond +-45 degrees: the edge columns, nothing dropped
    assert point((1.0, 5.0, 0.0))[0] % W == 0 and point((1.0, -5.0, 0.0))[0] % W == W - 1
    assert point((-1.0, 5.0, 0.0))[0] % W == 0 and point((-1.0, -5.0, 0.0))[0] % W == W - 1      # behind: asin sees |x| only
    assert point((5.0, 0.0, 0.0))[0] % W == int(b[0] / b[1])
    # the crop: lo <= p < hi
    for p, want in (((0.0, 1.0, 0.0), True), ((-tiny, 1.0, 0.0), False), ((80.0, 1.0, 0.0), False), ((79.99, 1.0, 0.0), True),
                    ((5.0, -50.0, 0.0), True), ((5.0, 50.0, 0.0), False), ((5.0, 1.0, -2.5), True), ((30.0, 1.0, 3.0), False)):
        assert (point(p, "classic", crop=R.CROP)[0] >= 0) == want, p
    # depths: a camera that looks along the lidar's x axis from its origin
    cam = np.array([80, 80, 80, 48, 0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0], np.float32)
    beams = P.beam_table(H, W)
    p = np.zeros(3, np.float32)
    for d, want in ((np.nan, False), (0.0, False), (-1.0, False), (np.inf, False), (80.0, False), (float(np.nextafter(np.float32(80), np.float32(0))), True),
                    (10.0, True)):
        got = shim.hm_pl_pixel(cam.ctypes.data, beams.ctypes.data, H, W, 0, 80, 48, d, p.ctypes.data)
        assert (got >= 0) == want, d
    assert np.array_equal(p, np.array([10.0, 0.0, 0.0], np.float32))
    assert got == cell_of((0.0 - beams[2]) / beams[4], beams[0] / beams[1])


# ---- resources, signatures and argument validation ------------------------------------------------------------------------------------
def test_pseudo_lidar_kernel_resources():
    assert "pseudo_lidar.hip" in B.SOURCES
    res = {short_name(k): v for k, v in kernel_resources("pseudo_lidar.hip").items()}
    want = ["pseudo_lidar_bin_kernel<0>", "pseudo_lidar_bin_kernel<1>", "pseudo_lidar_emit_kernel<0>", "pseudo_lidar_emit_kernel<1>"]
    assert sorted(res) == sorted(want), list(res)
    for k in want:
        print(f"\n{k}: occupancy {res[k]['Occupancy']} waves/SIMD, {res[k]['VGPRs']} VGPRs, LDS {res[k]['LDS Size']} bytes")
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["LDS Size"] <= 16 * 1024, (k, res[k])
        assert res[k]["Occupancy"] >= 8, (k, res[k])
    src = open(os.path.join(B.CSRC, "pseudo_lidar.hip")).read()
    assert "atomicAdd" not in src and "block_excl_scan" in src and '#include "scan.h"' in src      # no float atomics; the shared scan


def test_entries_resolve_with_the_declared_signatures():
    full = open(os.path.join(ROOT, "include", "bds.h")).read()
    hdr = header()
    decl = {k: v for k, v in declared_signatures().items() if re.fullmatch(r"bds_pseudo_lidar\w*", k)}
    assert sorted(decl) == ["bds_pseudo_lidar_from_depth", "bds_pseudo_lidar_from_points"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    P = module()
    for macro, value in (("BDS_PSEUDO_LIDAR_BEAMS", P.BEAMS), ("BDS_PSEUDO_LIDAR_VERTICAL", P.VERTICAL), ("BDS_PSEUDO_LIDAR_CLASSIC", P.CLASSIC)):
        assert f"#define {macro} {value}\n" in hdr, macro
    from bilateral_driving_amd import lidar
    assert P.MAX_ROWS == lidar.MAX_ROWS == 2 ** 31 - 1 - 256
    assert lib.bds_abi_version() == L.ABI_VERSION == 7      # (what each version changed: include/bds.h)
    for cite in ("generate_lidar/generate_lidar_from_depth.py:95-162", "generate_lidar/generate_lidar_from_depth.py:42-92",
                 "generate_lidar/depth2lidar.py:41-90"):
        assert cite in full, cite


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first
    big = 1 << 31

    def depth(C=2, Hi=48, Wi=80, d=p, cams=p, beams=p, H=8, W=16, s=1, mode=0, win=p, pts=p, cnt=p, src=p):
        return lib.bds_pseudo_lidar_from_depth(C, Hi, Wi, d, cams, beams, H, W, s, mode, win, pts, cnt, src, None)
    assert depth(C=0) == 0 and lib.bds_pseudo_lidar_from_depth(0, 0, 0, None, None, None, 0, 0, 0, 0, None, None, None, None, None) == 0
    for kw in (dict(C=-1), dict(C=65536), dict(Hi=0), dict(Wi=0), dict(H=0), dict(W=0), dict(s=0), dict(s=-1), dict(mode=2), dict(mode=-1),
               dict(d=None), dict(cams=None), dict(beams=None), dict(win=None), dict(pts=None), dict(cnt=None), dict(d=p + 2),
               dict(cams=p + 2), dict(beams=p + 4), dict(win=p + 2), dict(pts=p + 2), dict(cnt=p + 2), dict(src=p + 2),
               dict(C=1 << 12, Hi=1 << 10, Wi=1 << 10), dict(H=1 << 16, W=1 << 15), dict(C=4, H=1 << 14, W=1 << 15),
               dict(C=1, H=1 << 14, W=1 << 15, s=1)):
        assert depth(**kw) == L.BDS_EINVAL, kw

    def cloud(N=1000, x=p, beams=p, crop=0, H=64, W=512, s=1, mode=1, win=p, pts=p, cnt=p, src=p):
        return lib.bds_pseudo_lidar_from_points(N, x, beams, crop, H, W, s, mode, win, pts, cnt, src, None)
    for kw in (dict(N=-1), dict(N=big), dict(x=None), dict(beams=None), dict(crop=2), dict(crop=-1), dict(H=0), dict(W=0), dict(s=0),
               dict(mode=5), dict(win=None), dict(pts=None), dict(cnt=None), dict(x=p + 4), dict(x=p + 8), dict(beams=p + 4), dict(win=p + 2),
               dict(pts=p + 4), dict(pts=p + 8), dict(cnt=p + 2), dict(src=p + 2), dict(H=1 << 16, W=1 << 15), dict(H=1 << 15, W=1 << 14)):
        assert cloud(**kw) == L.BDS_EINVAL, kw
    assert lib.bds_strerror(L.BDS_EINVAL)


def test_python_checks_arguments_and_refuses_cpu_tensors():
    P = module()
    import bilateral_driving_amd
    assert bilateral_driving_amd.pseudo_lidar is P
    case = R.golden_depth_case("front")
    d, K = torch.from_numpy(case["depth"])[None], torch.from_numpy(case["K"])[None]
    c2w, l2w = torch.from_numpy(case["c2w"])[None], torch.from_numpy(case["l2w"])
    with pytest.raises(L.BdsError):
        P.depth_to_lidar(d, K, c2w, l2w, 8, 16)
    with pytest.raises(L.BdsError):
        P.depth_map_to_lidar_points(d[0], K[0], c2w[0], 80, 48, l2w, H=8, W=16)
    with pytest.raises(L.BdsError):
        P.cloud_to_lidar(torch.rand(10, 4))
    for kw in (dict(H=0), dict(W=0), dict(slice=0), dict(H=-3), dict(mode="radial"), dict(downscale_when_loading=0), dict(fov=(-30.0, 10.0)),
               dict(H=1 << 16, W=1 << 15), dict(crop=(0, 1, 2)), dict(max_depth=float("nan"))):
        with pytest.raises(ValueError):
            P.depth_to_lidar(d, K, c2w, l2w, **{"H": 8, "W": 16, **kw})
    bad = c2w.clone()
    bad[0, 1, 3] = float("nan")
    inf_l2w = l2w.clone()
    inf_l2w[0, 3] = float("inf")
    nanK = K.clone()
    nanK[0, 2] = float("nan")
    for args in ((d, K, bad, l2w), (d, K, c2w, inf_l2w), (d, nanK, c2w, l2w), (d, K, c2w, torch.zeros(4, 4)), (d, K * 0, c2w, l2w),
                 (d, K, c2w[0], l2w), (d, K[:, :3], c2w, l2w), (d.expand(2, -1, -1), K, c2w, l2w), (d[0, 0], K, c2w, l2w),
                 (d, K, c2w, l2w[None].expand(3, 4, 4))):
        with pytest.raises(ValueError):
            P.depth_to_lidar(*args, 8, 16)
    for x in (torch.rand(10, 3), torch.rand(10), torch.rand(2, 10, 4)):
        with pytest.raises(ValueError):
            P.cloud_to_lidar(x)
    with pytest.raises(ValueError):
        P.cloud_to_lidar(torch.rand(10, 4), H=0)
    with pytest.raises(ValueError):
        P.depth_map_to_lidar_points(d[0], K[0], c2w[0], 48, 80, l2w)      # width and height swapped
    # the tables: the reference's constants, the float64 matrix rounded once
    for mode in ("vertical", "classic"):
        assert np.array_equal(P.beam_table(9, 16, mode)[:5], np.array(R.beam_constants(9, 16, mode)))
    t = P.beam_table(8, 16)
    assert np.array_equal(t[5:11], np.array(R.CROP)) and t[11] == 80.0 and t.dtype == np.float64 and len(t) == P.BEAMS
    assert np.all(np.isinf(P.beam_table(8, 16, crop=None)[5:11]))
    for name in DEPTH_NAMES:
        c = R.golden_depth_case(name)
        table = P.camera_table(torch.from_numpy(c["K"])[None], torch.from_numpy(c["c2w"])[None], torch.from_numpy(c["l2w"]), c["downscale"])
        assert table.dtype == torch.float32 and tuple(table.shape) == (1, 16)
        assert np.array_equal(table[0, :4].numpy(), R.scaled_intrinsics(c["K"], c["downscale"]))
        M = R.exact_matrix(c["c2w"], c["l2w"])
        assert np.all(np.abs(table[0, 4:].numpy().reshape(3, 4) - M) <= 2.0 ** -24 * np.abs(M) + 1e-12)      # the float64 product, rounded once
    # install / uninstall
    mod = types.ModuleType("generate_lidar_from_depth")
    mod.pto_ang_map = former = lambda *a, **k: "former"
    mod.depth_map_to_lidar_points = former
    P.install(mod)
    P.install(mod)      # (twice: the former function is still the one remembered)
    assert mod.pto_ang_map is P.pto_ang_map and mod.depth_map_to_lidar_points is P.depth_map_to_lidar_points
    assert not hasattr(mod, "gen_sparse_points")      # only the names the module defines
    empty = types.ModuleType("empty")
    P.install(empty)
    assert all(getattr(empty, n) is getattr(P, n) for n in ("depth_map_to_lidar_points", "pto_ang_map", "pto_ang_map_vertical", "gen_sparse_points"))
    P.uninstall()
    assert mod.pto_ang_map is former and mod.depth_map_to_lidar_points is former and not hasattr(empty, "pto_ang_map")
