"""The projection's kept-blocks mode (include/bds.h bds_project_view_fwd_kept) and the compaction's early-out for scan tiles without a
visible entry (csrc/tiles.hip visible_compact_block): persistent output buffers whose rejected blocks are written once must hold,
after every call, byte for byte what the plain entry writes into fresh buffers -- and the state words must show that blocks really
were left alone.

The scene is built so that the block decisions are known: four groups of rows around fixed centres, two cameras A and B;
group 0 is seen by both, group 1 by neither, group 2 by A only, group 3 by B only.  ``test_block_rejection_by_construction`` checks that
on the CPU with the kernel's own test (csrc/gs_math.h box_may_be_visible through tests/hostmath_shim.hip); the GPU tests then read the
same decisions back from the state words."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from tests.util import fptr, hostmath

# ---- the scene, as constants -----------------------------------------------------------------------------------------------------
W, H = 64, 48
FOCAL = 64.0
K_MAT = [[FOCAL, 0.0, W / 2], [0.0, FOCAL, H / 2], [0.0, 0.0, 1.0]]
# world -> camera (x right, y down, z forward).  A: at the origin, looks along +x.  B: at (20, -20, 0), looks along +y.
VIEWMAT_A = [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
VIEWMAT_B = [[1.0, 0.0, 0.0, -20.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 20.0], [0.0, 0.0, 0.0, 1.0]]
GROUP_CENTRES = [(20.0, 0.0, 0.0),      # 0: 20 in front of A, 20 in front of B -- seen by both
                 (-30.0, -30.0, 0.0),   # 1: behind both
                 (40.0, 0.0, 0.0),      # 2: 40 in front of A; 45 degrees off B's axis (half field of view: 26.6)
                 (20.0, 20.0, 0.0)]     # 3: 40 in front of B; 45 degrees off A's axis
JITTER = 1.0             # centres: uniform in the cube of this half width round the group's centre
SCALE = 0.6              # activated scale (x 0.9 .. 1.1): 6-7 px of radius at depth 20, 4 at depth 40
SUBPIXEL_SCALE = 1e-3    # radius 2 (the eps2d blur alone) <= RADIUS_CLIP: culled row by row, the block survives
BEHIND_A = (-1.0, 0.0, 0.0)     # a centre behind A's near plane (and off B's image)
EPS2D, NEAR, FAR, RADIUS_CLIP = 0.3, 0.1, 1e10, 2.5
SEEN = {"A": (True, False, True, False), "B": (True, False, False, True)}     # per group


def make_scene(G: int, tail: int, seed: int = 0):
    """Groups 0-2 hold G rows, group 3 ``tail`` rows (a partial last block when tail % 256 != 0); CPU float32 tensors.  In every seen
    group a few rows are culled one by one: sub-pixel in groups 0, 2, 3, behind A's near plane in group 0."""
    g = torch.Generator().manual_seed(seed)
    sizes = [G, G, G, tail]
    N = sum(sizes)
    group = torch.repeat_interleave(torch.arange(4), torch.tensor(sizes))
    means = torch.tensor(GROUP_CENTRES)[group] + (torch.rand(N, 3, generator=g) * 2 - 1) * JITTER
    log_scales = (math.log(SCALE) + (torch.rand(N, 3, generator=g) * 0.2 - 0.1)).contiguous()
    quats = torch.randn(N, 4, generator=g)
    logits = torch.randn(N, generator=g)
    start = [0, G, 2 * G, 3 * G]
    for row in (start[0] + 9, start[0] + 200, start[2] + 3, start[2] + 100, start[3] + 2):
        log_scales[row] = math.log(SUBPIXEL_SCALE)
    for row in (start[0] + 5, start[0] + 77):
        means[row] = torch.tensor(BEHIND_A)
    sh = torch.randn(N, 16, 3, generator=g) * 0.2
    return dict(means=means.contiguous(), quats=quats, log_scales=log_scales, opacity_logits=logits, sh=sh), group


def _cam_arrays(name):
    return np.array(VIEWMAT_A if name == "A" else VIEWMAT_B, np.float32), np.array(K_MAT, np.float32)


@pytest.mark.parametrize("G,tail", [(256, 37), (2048, 293)])
def test_block_rejection_by_construction(G, tail):
    """CPU: the kernel's own block test on the boxes of the scene's 256-row blocks gives the table above (every block lies inside one
    group: G is a multiple of 256)."""
    hm = hostmath()
    p, group = make_scene(G, tail)
    N = group.numel()
    smax_all = p["log_scales"].exp().amax(1)
    for name in ("A", "B"):
        vm, Km = _cam_arrays(name)
        for b in range((N + 255) // 256):
            rows = slice(256 * b, min(256 * (b + 1), N))
            lo = p["means"][rows].amin(0).numpy().astype(np.float32).copy()
            hi = p["means"][rows].amax(0).numpy().astype(np.float32).copy()
            got = hm.hm_box_may_be_visible(fptr(lo), fptr(hi), C.c_float(float(smax_all[rows].max())), fptr(vm), fptr(Km), W, H,
                                           C.c_float(EPS2D), C.c_float(NEAR), C.c_float(FAR))
            assert bool(got) == SEEN[name][int(group[256 * b])], (name, b)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import fused_view as FV
    from bilateral_driving_amd import graph_view as GV
    from bilateral_driving_amd import harness as Hn
    return _lib, FV, GV, Hn


def _gpu_cams(Hn, dev="cuda"):
    Km = torch.tensor(K_MAT, device=dev)
    centres = {"A": (0.0, 0.0, 0.0), "B": (20.0, -20.0, 0.0)}
    return {n: Hn.Camera(torch.tensor(vm, device=dev), Km.clone(), W, H, torch.tensor(centres[n], device=dev))
            for n, vm in (("A", VIEWMAT_A), ("B", VIEWMAT_B))}


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


class _Outputs:
    """One set of projection output buffers in the row or the column form."""

    def __init__(self, N, rows, aa, fill):
        dev = "cuda"
        mk = (lambda *s: torch.zeros(*s, device=dev)) if fill == "zero" else (lambda *s: torch.full(s, float("nan"), device=dev))
        self.t = {"scales": mk(N, 3), "opac": mk(N), "radii": mk(N), "tpg": mk(N)}      # (radii / tpg: int32 words behind float storage)
        if rows:
            self.t["rows"] = mk(N, 8)
        else:
            self.t.update(m2=mk(N, 2), dep=mk(N), con=mk(N, 3))
            if aa:
                self.t["opac_eff"] = mk(N)
        self.rows = rows

    def fill_nan(self):
        for t in self.t.values():
            t.fill_(float("nan"))

    def ptrs(self):
        t = self.t
        if self.rows:
            base = t["rows"].data_ptr()
            m2, dep, con = base, base + 8, base + 16
        else:
            m2, dep, con = t["m2"].data_ptr(), t["dep"].data_ptr(), t["con"].data_ptr()
        oe = t["opac_eff"].data_ptr() if "opac_eff" in t else None
        return t["scales"].data_ptr(), t["opac"].data_ptr(), oe, t["radii"].data_ptr(), m2, dep, con


@pytest.fixture(scope="module")
def small_scene(mods):
    L = mods[0]
    p, group = make_scene(256, 37)
    d = {k: v.cuda() for k, v in p.items()}
    N = group.numel()
    bounds = torch.zeros((N + 255) // 256, 8, device="cuda")
    L.check(L.lib().bds_gaussian_block_bounds(N, L.ptr(d["means"]), L.ptr(d["log_scales"]), L.ptr(bounds), L.stream()), "block_bounds")
    return d, N, bounds


@pytest.mark.gpu
@pytest.mark.parametrize("rows,aa,prep", list(itertools.product((True, False), (False, True), (True, False))))
def test_kept_blocks_equal_the_plain_entry_call_by_call(mods, small_scene, rows, aa, prep):
    """Calls A, A, B, A into zeroed persistent buffers + zeroed state against the plain entry into NaN-filled buffers: every dense
    output and the per-block visible counts bit for bit after every call; the state words walk as the scene dictates; a canary in a
    twice-rejected block survives the call (the skip really happened); after a reset one call reproduces the plain entry."""
    L = mods[0]
    Hn = mods[3]
    lib, st = L.lib(), L.stream()
    d, N, bounds = small_scene
    assert N == 3 * 256 + 37
    cams = _gpu_cams(Hn)
    nb = (N + 255) // 256
    ws_bytes = int(lib.bds_isect_prepare_workspace_bytes(1, N))
    sums_off = int(lib.bds_isect_block_counts_offset(1, N))
    kept, ref = _Outputs(N, rows, aa, "zero"), _Outputs(N, rows, aa, "nan")
    state = torch.zeros(nb, device="cuda", dtype=torch.int32)
    ws_k, ws_r = (torch.zeros(max(ws_bytes, 16), device="cuda", dtype=torch.uint8) for _ in range(2))

    def call(out, ws, cam, state_t):
        head = (L.PROJ_ANTIALIASED if aa else 0, N, L.ptr(d["means"]), L.ptr(d["quats"]), L.ptr(d["log_scales"]), L.ptr(d["opacity_logits"]),
                L.ptr(cam.viewmat), L.ptr(cam.K), W, H, EPS2D, NEAR, FAR, RADIUS_CLIP, *out.ptrs())
        tail = (out.t["tpg"].data_ptr(), L.ptr(ws), ws_bytes) if prep else (None, None, 0)
        if state_t is None:
            L.check(lib.bds_project_view_fwd(*head, *tail, L.ptr(bounds), st), "bds_project_view_fwd")
        else:
            L.check(lib.bds_project_view_fwd_kept(*head, *tail, L.ptr(bounds), L.ptr(state_t), st), "bds_project_view_fwd_kept")

    def sums(ws):
        return ws[sums_off:sums_off + 4 * nb].view(torch.int32)

    def step(name, what):
        ref.fill_nan()
        call(ref, ws_r, cams[name], None)
        call(kept, ws_k, cams[name], state)
        torch.cuda.synchronize()
        return what

    def compare(what):
        for k in kept.t:
            if k == "tpg" and not prep:
                continue      # (not written without prep_ws, by either entry)
            assert torch.equal(_bits(kept.t[k]), _bits(ref.t[k])), (what, k)
            assert not bool(torch.isnan(ref.t[k]).any()), (what, k)      # (the plain entry wrote every row)
        if prep:
            assert torch.equal(sums(ws_k), sums(ws_r)), what
            assert torch.equal(ws_k[:16], ws_r[:16]), what       # (M cleared)
            vis = kept.t["radii"].view(torch.int32) > 0
            per_block = torch.zeros(nb, device="cuda", dtype=torch.int64).scatter_add_(0, torch.arange(N, device="cuda") // 256, vis.long())
            assert torch.equal(sums(ws_k).long(), per_block), what

    def expect_state(seen):
        assert state.tolist() == [0 if s else 1 for s in seen], (state.tolist(), seen)

    compare(step("A", "A #1"))
    expect_state(SEEN["A"])
    radii = kept.t["radii"].view(torch.int32)
    assert int((radii[:256] > 0).sum()) == 256 - 4 and int((radii[512:768] > 0).sum()) == 256 - 2      # (rows culled one by one)
    assert int((radii[256:512] > 0).sum()) == 0 and int((radii[768:] > 0).sum()) == 0
    assert float(kept.t["scales"][9].max()) > 0 and float(kept.t["scales"][256:512].abs().max()) == 0     # culled row vs rejected block
    # the skip itself: a canary inside block 1 (rejected before, state 1) must survive the next call
    canary = (256 + 5, 1)
    kept.t["scales"][canary] = 123.0
    step("A", "A #2")
    assert int(state[1]) == 1
    assert float(kept.t["scales"][canary]) == 123.0, "a kept block was written"
    kept.t["scales"][canary] = 0.0
    compare("A #2")
    expect_state(SEEN["A"])
    compare(step("B", "B #1"))
    expect_state(SEEN["B"])          # block 2: 0 -> 1, block 3: 1 -> 0
    assert int((kept.t["radii"].view(torch.int32)[768:] > 0).sum()) == 37 - 1
    compare(step("A", "A #3"))
    expect_state(SEEN["A"])
    # reset: unknown state over buffers that hold anything
    state.zero_()
    kept.fill_nan()
    compare(step("A", "A after reset"))
    expect_state(SEEN["A"])


def _lists(out, M, nv):
    i = out["info"]
    return i["flatten_ranks"][:M].clone(), i["visible_ids"][:nv].clone(), i["isect_offsets"].clone(), i["tiles_per_gauss"].clone()


@pytest.mark.gpu
def test_compaction_skips_empty_scan_tiles_without_changing_the_lists(mods, monkeypatch):
    """The device-count tile stage (bds_isect_prepare / bds_isect_build behind the kept-blocks projection) over a scene in which whole
    2048-row scan tiles hold no visible entry, against the general path, which has no compaction kernel (option 4 off: flags, scan,
    scatter, radix sort; host counts): visible ids, per-tile lists in depth order, offsets, per-Gaussian tile counts and both counts
    bit for bit -- for A, A again (kept blocks), then B and A on the same persistent buffers."""
    L, FV, GV, Hn = mods
    monkeypatch.setattr(FV, "SH_IN_PACK", FV.SH_IN_PACK_DEV)
    G, tail = 2048, 293
    p, group = make_scene(G, tail)
    N = group.numel()
    p = {k: v.cuda() for k, v in p.items()}
    cams = _gpu_cams(Hn)
    bounds = torch.zeros((N + 255) // 256, 8, device="cuda")
    L.check(L.lib().bds_gaussian_block_bounds(N, L.ptr(p["means"]), L.ptr(p["log_scales"]), L.ptr(bounds), L.stream()), "block_bounds")
    grids = Hn.make_grids(1, device="cuda")
    gen = torch.Generator().manual_seed(3)
    sky, target = torch.rand(H, W, 3, generator=gen).cuda(), torch.rand(H, W, 3, generator=gen).cuda()
    kw = dict(radius_clip=RADIUS_CLIP, near_plane=NEAR)
    want = {}
    keep_opt = int(L.lib().bds_get_option(L.OPT_SHORT_SORT))
    try:
        L.set_option(L.OPT_SHORT_SORT, 0)
        for name in ("A", "B"):
            ref = Hn.train_view(p, cams[name], grids, 0, sky, target, **kw)
            torch.cuda.synchronize()
            M, nv = ref["info"]["n_isects"], ref["info"]["n_visible"]
            want[name] = (M, nv, _lists(ref, M, nv), ref["radii"].clone())
    finally:
        L.set_option(L.OPT_SHORT_SORT, keep_opt)
    # A: groups 0 and 2 less their rows culled one by one; B: groups 0 (the two centres behind A are off B's image) and 3
    assert want["A"][1] == 2 * G - 6 and want["B"][1] == G + tail - 5
    ws_bytes = int(L.lib().bds_isect_prepare_workspace_bytes(1, N))
    ws = torch.zeros(max(ws_bytes, 16), device="cuda", dtype=torch.uint8)
    sums_off = int(L.lib().bds_isect_block_counts_offset(1, N))
    nb = (N + 255) // 256
    fb = FV.FrontBuffers()
    for i, name in enumerate(("A", "A", "B", "A")):
        M, nv, lists, radii = want[name]
        caps = FV.ListCapacity(int(M * 1.3) + 100, int(nv * 1.3) + 100)
        out = Hn.train_view(p, cams[name], grids, 0, sky, target, caps=caps, prep_ws=ws, block_bounds=bounds, front_bufs=fb, **kw)
        torch.cuda.synchronize()
        assert caps.observed() == (M, nv) and not caps.overflowed(), (i, name, caps.observed(), (M, nv))
        assert torch.equal(out["radii"], radii), (i, name)
        for a, b, what in zip(_lists(out, M, nv), lists, ("flatten_ranks", "visible_ids", "isect_offsets", "tiles_per_gauss")):
            assert torch.equal(a, b), (i, name, what)
        assert torch.equal(lists[1].long(), (radii.reshape(-1) > 0).nonzero().squeeze(1)), (i, name)      # ascending visible ids
        sums = ws[sums_off:sums_off + 4 * nb].view(torch.int32)
        per_tile = torch.nn.functional.pad(sums, (0, (-nb) % 8)).view(-1, 8).sum(1)
        assert int(sums.sum()) == nv
        assert int((per_tile == 0).sum()) >= 1 and int((per_tile > 0).sum()) >= 2, per_tile.tolist()     # whole scan tiles without an entry
        assert fb.state.tolist() == [0 if SEEN[name][int(group[256 * b])] else 1 for b in range(nb)], (i, name)


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", [False, True], ids=["fixed", "dynamic"])
def test_frame_replays_are_unchanged_by_the_mode(mods, monkeypatch, dynamic):
    """FrameGraph, two view slots (A, B), ~2 k Gaussians in Morton order, 64 x 48: three replays with the mode on against the switch
    off -- images bit for bit, losses and the flat gradient within the bounds of selfcheck.frame_against_eager (what
    tests/test_gpu_04 holds a replay to against the eager frame: 1e-5 absolute, 1e-4 norm-relative; float atomics order only).
    dynamic: then the slots swap cameras (set_view) and replay twice more."""
    L, FV, GV, Hn = mods
    from bilateral_driving_amd.selfcheck import GRAD_TOL, LOSS_TOL
    scene, _ = make_scene(640, 165)
    scene = {k: v.cuda() for k, v in scene.items()}
    order = Hn.spatial_order(scene["means"])
    scene = {k: v[order].contiguous() for k, v in scene.items()}
    gen = torch.Generator().manual_seed(5)
    sky_t = [torch.rand(H, W, 3, generator=gen).cuda() for _ in range(2)]
    tgt_t = [torch.rand(H, W, 3, generator=gen).cuda() for _ in range(2)]
    grid_t = Hn.make_grids(2, device="cuda")

    def run(keep):
        monkeypatch.setattr(GV, "BLOCK_KEEP", keep)
        cams = _gpu_cams(Hn)
        cams = [cams["A"], cams["B"]]
        p = {k: v.clone().requires_grad_(True) for k, v in scene.items()}
        grids = [g.clone().requires_grad_(True) for g in grid_t]
        skies = [s.clone().requires_grad_(True) for s in sky_t]
        frame = GV.FrameGraph(p, cams, grids, skies, [t.clone() for t in tgt_t], dynamic=dynamic)
        assert (frame.front_bufs is not None) == keep
        seen = []

        def replay():
            assert frame.step() is True
            torch.cuda.synchronize()
            seen.append(([vg.rgb.detach().clone() for vg in frame.views], [float(vg.loss) for vg in frame.views],
                         frame.flat.flat.detach().clone()))
        for _ in range(3):
            replay()
        if keep:       # (not vacuous: both slots hold blocks their camera rejects, and have kept them)
            states = [fb.state.clone() for fb in frame.front_bufs]
            assert all(0 < int(s.sum()) < s.numel() for s in states) and not torch.equal(states[0], states[1])
        if dynamic:
            frame.set_view(0, cams[1], tgt_t[1], sky_t[1], 1)
            frame.set_view(1, cams[0], tgt_t[0], sky_t[0], 0)
            replay()
            replay()
            if keep:
                assert torch.equal(frame.front_bufs[0].state, states[1]) and torch.equal(frame.front_bufs[1].state, states[0])
        return seen

    on, off = run(True), run(False)
    assert len(on) == len(off) == (5 if dynamic else 3)
    for i, ((rgb_a, loss_a, g_a), (rgb_b, loss_b, g_b)) in enumerate(zip(on, off)):
        for v in range(2):
            assert torch.equal(rgb_a[v], rgb_b[v]), (i, v)
            assert float(rgb_a[v].std()) > 0
            assert abs(loss_a[v] - loss_b[v]) <= LOSS_TOL, (i, v, loss_a[v], loss_b[v])
        assert float(g_b.norm()) > 0
        assert float((g_a.double() - g_b.double()).norm()) <= GRAD_TOL * float(g_b.double().norm()), i
