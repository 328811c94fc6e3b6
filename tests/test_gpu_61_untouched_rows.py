"""-m gpu: the Gaussian half of the backward leaves alone the visible rows no pixel blended (include/bds.h UNTOUCHED ROWS).

A view lists every visible Gaussian; its pixels saturate after some tens of blends, so most listed Gaussians are never blended and
their gradient record stays all zero.  The skipping forms -- ``bds_sh_view_bwd_list`` with ``BDS_SH_SKIP_UNTOUCHED``,
``bds_project_view_bwd_list_touched`` with ``BDS_PROJ_SKIP_UNTOUCHED``, ``bds_view_grads_clear_list_touched`` -- move nothing for such
a rank.  Three levels:

1. kernel level, hand-made records: the skipping forms against the dense entries on the same inputs, every output array equal as
   floats (``np.array_equal``: a skipped row may differ from the dense one in the sign of a zero only), the mask equal to "floats
   0-11 of the record not all +-0";
2. the masked clear: rows with mask 1 zero, canaries alive everywhere else;
3. frame level: ``graph_view.FrameGraph`` over a scene with an opaque wall in front of 500 Gaussians, the wall switched transparent
   and opaque again between frames, against the eager dense frame.

Bounds.  Level 1 is equality; the pose slots of lists longer than one workgroup go through float atomics and are held to the
projection's pose tolerance of tests/test_gpu_01_gs_parity.py (1e-4 norm-relative).  Level 3 uses the replay-against-eager bounds of
tests/test_gpu_04 (bilateral_driving_amd/selfcheck.py): gradients 1e-4 norm-relative, pose gradients 1e-3."""
import math

import numpy as np
import pytest
import torch

from tests.util import make_scene

pytestmark = pytest.mark.gpu

LIST_NS = (1, 255, 256, 257, 600)
PATTERNS = ("all_zero", "all_nonzero", "alternating", "block_zero_middle", "block_zero_end", "neg_zero_only", "depth_only", "opacity_only",
            "absgrad_only", "colour_killed_by_clamp")
POSE_TOL = 1e-4          # tests/test_gpu_01_gs_parity.py::test_projection_fwd_bwd
GRAD_TOL, FRAME_POSE_TOL = 1e-4, 1e-3      # selfcheck.GRAD_TOL; tests/test_gpu_04 test_replayed_frame_at_full_size_equals_eager_frame
W0, H0 = 320, 200


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib as L
    L.lib()
    return L


@pytest.fixture(scope="module")
def scene(env):
    """3000 Gaussians in front of one camera, projected once: the activated parameters and the ids of the visible ones (any order)."""
    L = env
    lib, st = L.lib(), L.stream()
    N = 3000
    s = {k: v.cuda() for k, v in make_scene(N, W0, H0, seed=0).items()}
    log_scales, logits = s["scales"].log(), torch.logit(s["opacities"].clamp(1e-4, 1 - 1e-4))
    vm, K = s["viewmats"][0].contiguous(), s["Ks"][0].contiguous()
    scales, opac = torch.empty(N, 3, device="cuda"), torch.empty(N, device="cuda")
    radii = torch.empty(1, N, dtype=torch.int32, device="cuda")
    m2, dep, con = torch.empty(1, N, 2, device="cuda"), torch.empty(1, N, device="cuda"), torch.empty(1, N, 3, device="cuda")
    L.check(lib.bds_project_view_fwd(0, N, L.ptr(s["means"]), L.ptr(s["quats"]), L.ptr(log_scales), L.ptr(logits), L.ptr(vm), L.ptr(K), W0, H0,
                                     0.3, 0.01, 1e10, 0.0, L.ptr(scales), L.ptr(opac), None, L.ptr(radii), L.ptr(m2), L.ptr(dep), L.ptr(con),
                                     None, None, 0, None, st), "fwd")
    g = torch.Generator().manual_seed(61)
    ids = (radii[0] > 0).nonzero().squeeze(1).to(torch.int32)
    ids = ids[torch.randperm(ids.numel(), generator=g).cuda()].contiguous()
    assert ids.numel() >= max(LIST_NS), ids.numel()
    cam_pos = torch.linalg.inv(vm)[:3, 3].contiguous()
    return dict(N=N, means=s["means"].contiguous(), quats=s["quats"].contiguous(), scales=scales, opac=opac, vm=vm, K=K, ids=ids, cam_pos=cam_pos)


def make_records(pattern, n, gen):
    """[n,16] gradient records + the un-clamped colours [n,3] (by rank) that decide the clamp."""
    rec = torch.randn(n, 16, generator=gen)
    sh_rgb = torch.rand(n, 3, generator=gen) * 1.4 - 0.7        # some channels beyond both ends of the clamp
    r = torch.arange(n)
    if pattern == "all_zero":
        rec[:, :12] = 0                                         # (floats 12-15 are no part of the record's gradient: left as junk)
    elif pattern == "alternating":
        rec[r % 2 == 1, :12] = 0
    elif pattern == "block_zero_middle":
        rec[(r >= 256) & (r < 512), :12] = 0
    elif pattern == "block_zero_end":
        rec[r >= 256 * ((n - 1) // 256), :12] = 0
    elif pattern == "neg_zero_only":
        rec[:, :12] = -0.0
    elif pattern in ("depth_only", "opacity_only", "absgrad_only"):
        keep = {"depth_only": [3], "opacity_only": [11], "absgrad_only": [9, 10]}[pattern]
        z = torch.zeros(n, 16)
        z[:, keep] = rec[:, keep]
        rec = z
    elif pattern == "colour_killed_by_clamp":
        rec[:, 3:] = 0
        sh_rgb = torch.where(torch.rand(n, 3, generator=gen) < 0.5, torch.full((n, 3), 0.9), torch.full((n, 3), -0.9))
    else:
        assert pattern == "all_nonzero"
    return rec.cuda().contiguous(), sh_rgb.cuda().contiguous()


def eq(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sh_call(L, n, ids, K, deg, sc, sh_rgb, rec, dst, row_map, mode):
    """dst: (v_coeffs, v_rest or None)."""
    L.check(L.lib().bds_sh_view_bwd_list(n, None, L.ptr(ids), K, deg, L.ptr(sc["means"]), L.ptr(sc["cam_pos"]), L.ptr(sh_rgb), 1, L.ptr(rec),
                                         L.ptr(dst[0]), L.ptr(dst[1]), L.ptr(row_map), mode, L.stream()), "sh bwd list")


@pytest.mark.parametrize("K,deg", [(16, 3), (4, 1)])
@pytest.mark.parametrize("n", LIST_NS)
def test_sh_backward_skipping_equals_dense(env, scene, n, K, deg):
    """One-array and split storage x store / accumulate x row_map: every array equal as floats, untouched rows keep their bits."""
    L = env
    sc = scene
    gen = torch.Generator().manual_seed(1000 * n + K)
    ids = sc["ids"][:n].contiguous()
    il = ids.long()
    N = sc["N"]
    rows_mapped = n + 7
    row_map = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    row_map[il] = torch.randperm(rows_mapped, generator=gen)[:n].to(torch.int32).cuda()
    for pattern in PATTERNS:
        rec, sh_rgb = make_records(pattern, n, gen)
        x = sh_rgb + 0.5
        colour = torch.where((x >= 0) & (x <= 1), rec[:, :3], torch.zeros_like(rec[:, :3]))
        live = (colour != 0).any(1)
        if pattern in ("all_zero", "neg_zero_only", "depth_only", "opacity_only", "absgrad_only", "colour_killed_by_clamp"):
            assert not bool(live.any())
        # the kernel's three write paths: whole 16-byte pieces (one array), float by float (one array whose base lies 4 bytes past a
        # 16-byte boundary), the split storage's 16-byte pieces at 4-byte alignment
        for storage in ("one", "one_offset", "split"):
            for mapped in ((False, True) if storage != "split" else (False,)):      # (the split storage takes no row_map)
                rows = rows_mapped if mapped else N
                dst_rows = (row_map[il] if mapped else ids).long()
                for acc in (0, 1):
                    prior = torch.randn(rows, K, 3, generator=gen).cuda() if acc else torch.zeros(rows, K, 3, device="cuda")
                    res = []
                    for skip in (0, L.SH_SKIP_UNTOUCHED):
                        if storage == "one":
                            dst = (prior.clone(), None)
                        elif storage == "one_offset":
                            buf = torch.empty(prior.numel() + 1, device="cuda")
                            body = buf[1:].view(prior.shape)
                            body.copy_(prior)
                            assert body.data_ptr() % 16 == 4
                            dst = (body, None)
                        else:
                            dst = (prior[:, 0].contiguous(), prior[:, 1:].contiguous())
                        _sh_call(L, n, ids, K, deg, sc, sh_rgb, rec, dst, row_map if mapped else None, acc | skip)
                        res.append(dst[0] if storage != "split" else torch.cat([dst[0][:, None], dst[1]], 1))
                    dense, skipped = res
                    assert eq(dense, skipped), (pattern, storage, mapped, acc)
                    dead = dst_rows[~live]
                    assert same_bits(skipped[dead], prior[dead]), (pattern, storage, mapped, acc)      # neither read nor written
                    if bool(live.any()):
                        assert same_bits(skipped[dst_rows[live]], dense[dst_rows[live]]), (pattern, storage, mapped, acc)
                        assert bool((skipped[dst_rows[live]] != prior[dst_rows[live]]).any())


def _proj_call(L, touched_entry, flags, n, ids, sc, rec, outs, slots, g2d, ag2d, row_map, touched=None):
    lib, st = L.lib(), L.stream()
    head = (flags, n, None, L.ptr(ids), L.ptr(sc["means"]), L.ptr(sc["quats"]), L.ptr(sc["scales"]), L.ptr(sc["opac"]), L.ptr(sc["vm"]),
            L.ptr(sc["K"]), W0, H0, 0.3, L.ptr(rec), *outs, None, L.ptr(slots), L.ptr(g2d), L.ptr(ag2d), L.ptr(row_map))
    if touched_entry:
        L.check(lib.bds_project_view_bwd_list_touched(*head, L.ptr(touched), st), "project bwd list, touched")
    else:
        L.check(lib.bds_project_view_bwd_list(*head, st), "project bwd list")


def _grad_outs(L, layout, prior):
    """prior [rows,16] random or zero -> (tensors the kernel writes, the four pointers v_means / v_quats / v_scales / v_opacities, what
    the tensors held before)."""
    if layout == "block":
        block = prior.clone()
        base = L.ptr(block)
        return [block], [base, base + 16, base + 32, base + 12], [prior]
    before = [prior[:, 0:3].contiguous(), prior[:, 4:8].contiguous(), prior[:, 8:11].contiguous(), prior[:, 3].contiguous()]
    t = [x.clone() for x in before]
    return t, [L.ptr(x) for x in t], before


@pytest.mark.parametrize("n", LIST_NS)
def test_projection_backward_skipping_equals_dense(env, scene, n):
    """Separate arrays and the [N,16] row block x store / accumulate x row_map: parameter gradients, both screen-space arrays and the
    pose slots against the dense entry; the mask rank by rank."""
    L = env
    sc = scene
    gen = torch.Generator().manual_seed(7000 + n)
    ids = sc["ids"][:n].contiguous()
    il = ids.long()
    N = sc["N"]
    rows_mapped = n + 7
    row_map = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    row_map[il] = torch.randperm(rows_mapped, generator=gen)[:n].to(torch.int32).cuda()
    for pattern in PATTERNS:
        rec, _ = make_records(pattern, n, gen)
        want_mask = (rec[:, :12] != 0).any(1)
        if pattern in ("all_zero", "neg_zero_only"):
            assert not bool(want_mask.any())
        if pattern in ("depth_only", "opacity_only", "absgrad_only", "colour_killed_by_clamp", "all_nonzero"):
            assert bool(want_mask.all())
        for layout in ("separate", "block"):
            for mapped in (False, True):
                rows = rows_mapped if mapped else N
                dst_rows = (row_map[il] if mapped else ids).long()
                for acc in (0, 1):
                    prior = torch.randn(rows, 16, generator=gen).cuda() if acc else torch.zeros(rows, 16, device="cuda")
                    res = []
                    for skip in (False, True):
                        outs, ptrs, before = _grad_outs(L, layout, prior)
                        slots = torch.zeros(L.POSE_GRAD_SLOTS, 4, 4, device="cuda")
                        g2d, ag2d = torch.zeros(N, 2, device="cuda"), torch.zeros(N, 2, device="cuda")     # (stored in both modes)
                        mask = torch.full((n + 9,), 7, dtype=torch.uint8, device="cuda")
                        flags = (L.PROJ_ACCUMULATE if acc else 0) | (L.PROJ_SKIP_UNTOUCHED if skip else 0)
                        _proj_call(L, skip, flags, n, ids, sc, rec, ptrs, slots, g2d, ag2d, row_map if mapped else None, mask)
                        res.append((outs, slots, g2d, ag2d, mask))
                    (d_outs, d_slots, d_g2d, d_ag2d, _), (s_outs, s_slots, s_g2d, s_ag2d, s_mask) = res
                    tag = (pattern, layout, mapped, acc)
                    dead = dst_rows[~want_mask]
                    for a, b, pr in zip(d_outs, s_outs, before):
                        assert eq(a, b), tag
                        assert same_bits(b[dead], pr[dead]), tag                      # an untouched rank's row: neither read nor written
                    assert eq(d_g2d, s_g2d) and eq(d_ag2d, s_ag2d), tag
                    if n <= 256:
                        assert eq(d_slots, s_slots), tag
                    else:
                        assert float((d_slots.sum(0) - s_slots.sum(0)).norm()) <= POSE_TOL * float(d_slots.sum(0).norm()), tag
                    assert torch.equal(s_mask[:n].bool(), want_mask) and bool((s_mask[:n] <= 1).all()), tag
                    assert bool((s_mask[n:] == 7).all()), tag
    # the mask without the flag: written, nothing skipped (bit-equal to the dense entry on one workgroup)
    rec, _ = make_records("alternating", n, gen)
    res = []
    for with_mask in (False, True):
        prior = torch.zeros(N, 16, device="cuda")
        outs, ptrs, _ = _grad_outs(L, "separate", prior)
        mask = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        _proj_call(L, with_mask, 0, n, ids, sc, rec, ptrs, None, None, None, None, mask)
        res.append((outs, mask))
    for a, b in zip(res[0][0], res[1][0]):
        assert same_bits(a, b)
    assert torch.equal(res[1][1].bool(), (rec[:, :12] != 0).any(1))
    # the dense entry refuses the flag
    outs, ptrs, _ = _grad_outs(L, "separate", torch.zeros(N, 16, device="cuda"))
    head = (L.PROJ_SKIP_UNTOUCHED, n, None, L.ptr(ids), L.ptr(sc["means"]), L.ptr(sc["quats"]), L.ptr(sc["scales"]), L.ptr(sc["opac"]),
            L.ptr(sc["vm"]), L.ptr(sc["K"]), W0, H0, 0.3, L.ptr(rec), *ptrs, None, None, None, None, None)
    assert L.lib().bds_project_view_bwd_list(*head, L.stream()) == L.BDS_EINVAL


@pytest.mark.parametrize("K", [16, 4, 9])
@pytest.mark.parametrize("n", LIST_NS)
def test_masked_clear(env, n, K):
    """Rows with mask != 0 are zero afterwards; canaries survive in listed rows with mask 0, in unlisted rows and under negative
    (padding) ids; a null mask is today's clear."""
    L = env
    lib, st = L.lib(), L.stream()
    N = 700
    gen = torch.Generator().manual_seed(100 * n + K)
    ids_t = torch.randperm(N, generator=gen)[:n].to(torch.int32)
    ids_t[2::3] = -1
    mask_t = torch.randint(0, 3, (n,), generator=gen).to(torch.uint8) * 127       # 0, 127, 254: any non-zero byte is "touched"
    want = torch.zeros(N, dtype=torch.bool)
    sel = (ids_t >= 0) & (mask_t != 0)
    want[ids_t[sel].long()] = True
    want_all = torch.zeros(N, dtype=torch.bool)
    want_all[ids_t[ids_t >= 0].long()] = True
    ids, mask, want, want_all = ids_t.cuda(), mask_t.cuda(), want.cuda(), want_all.cuda()
    shapes = ((3,), (4,), (3,), (), (K, 3), (2,), (2,))
    prior = [torch.randn(N, *s, generator=gen).cuda() for s in shapes]
    block_t = torch.randn(N, 16, generator=gen).cuda()
    assert not bool(torch.cat([p.reshape(N, -1) for p in prior] + [block_t], 1).eq(0).any())      # the canaries are non-zero

    def cleared(t, rows):
        t = t.clone()
        t[rows] = 0
        return t

    for m, rows in ((mask, want), (None, want_all)):
        bufs = [p.clone() for p in prior]
        L.check(lib.bds_view_grads_clear_list_touched(n, None, L.ptr(ids), K, *[L.ptr(b) for b in bufs], L.ptr(m), st), "masked clear")
        for b, p in zip(bufs, prior):
            assert same_bits(b, cleared(p, rows)), (n, K, m is None, tuple(p.shape))
        # the [N,16] row block + the screen-space pair only
        block, v_sh = block_t.clone(), prior[4].clone()
        base = L.ptr(block)
        L.check(lib.bds_view_grads_clear_list_touched(n, None, L.ptr(ids), K, base, base + 16, base + 32, base + 12, L.ptr(v_sh), None, None,
                                                      L.ptr(m), st), "masked clear, row block")
        assert same_bits(block, cleared(block_t, rows)) and same_bits(v_sh, cleared(prior[4], rows)), (n, K, m is None)
        g2, a2 = prior[5].clone(), prior[6].clone()
        L.check(lib.bds_view_grads_clear_list_touched(n, None, L.ptr(ids), K, None, None, None, None, None, L.ptr(g2), L.ptr(a2), L.ptr(m), st),
                "masked clear, screen space only")
        assert same_bits(g2, cleared(prior[5], rows)) and same_bits(a2, cleared(prior[6], rows)), (n, K, m is None)
    # a null mask is the existing entry, bit for bit
    a, b = [p.clone() for p in prior], [p.clone() for p in prior]
    L.check(lib.bds_view_grads_clear_list(n, None, L.ptr(ids), K, *[L.ptr(t) for t in a], st), "clear")
    L.check(lib.bds_view_grads_clear_list_touched(n, None, L.ptr(ids), K, *[L.ptr(t) for t in b], None, st), "clear, null mask")
    assert all(same_bits(x, y) for x, y in zip(a, b))
    # a device count below the list length: the ranks past it keep their rows whatever their mask says
    cnt = 2 * n // 3
    n_dev = torch.tensor([cnt], dtype=torch.int64, device="cuda")
    rows_c = torch.zeros(N, dtype=torch.bool)
    sel_c = sel.clone()
    sel_c[cnt:] = False
    rows_c[ids_t[sel_c].long()] = True
    bufs = [p.clone() for p in prior]
    L.check(lib.bds_view_grads_clear_list_touched(n, L.ptr(n_dev), L.ptr(ids), K, *[L.ptr(t) for t in bufs], L.ptr(mask), st), "masked clear, device count")
    for t, p in zip(bufs, prior):
        assert same_bits(t, cleared(p, rows_c.cuda())), (n, K)


# ---- frame level -------------------------------------------------------------------------------------------------------------------
WALL, HIDDEN, FRONT, BEHIND = 4, 500, 60, 130
FW, FH = 64, 48


def wall_scene(device="cpu"):
    """World frame of harness.ring_cameras (x forward, y left, z up), the rig at the origin.  Rows: [0, WALL) a wall of flat Gaussians
    across the whole image at x = 2 .. 2.3; then FRONT small ones in front of the wall; then HIDDEN small ones at x = 4 .. 8 inside
    both cameras' images; then BEHIND ones behind the cameras (in no list).  A view's list is in ascending row order, so with the wall
    opaque the ranks [WALL + FRONT, WALL + FRONT + HIDDEN) = [64, 564) are untouched: the whole workgroup of ranks 256 .. 511.  Checked with oracle.gs_oracle.rasterization when this
    test was written (loss = sum of the render + sum of the alphas, both cameras): with the wall opaque all 564 = WALL + HIDDEN +
    FRONT rows are visible in both views, every hidden row has an all-zero gradient (two wall rows and the 60 front rows have one) and
    every pixel's alpha is >= 0.990; with the wall transparent all 500 hidden rows have a non-zero one in both views."""
    g = torch.Generator().manual_seed(61)
    fx = 0.5 * FW / math.tan(math.radians(35.0))

    def inside(n, x, half_u, half_v):     # points at depth x whose image in camera 0 lies within (+-half_u, +-half_v) px of the centre
        u = (torch.rand(n, generator=g) * 2 - 1) * half_u
        v = (torch.rand(n, generator=g) * 2 - 1) * half_v
        return torch.stack([x, -u * x / fx, -v * x / fx], -1)

    N = WALL + HIDDEN + FRONT + BEHIND
    means = torch.zeros(N, 3)
    log_scales = torch.zeros(N, 3)
    logits = torch.zeros(N)
    quats = torch.zeros(N, 4)
    quats[:, 0] = 1.0
    means[:WALL, 0] = 2.0 + 0.1 * torch.arange(WALL)
    log_scales[:WALL] = torch.tensor([0.01, 8.0, 8.0]).log()
    logits[:WALL] = 10.0
    f0, h0, b0 = WALL, WALL + FRONT, WALL + FRONT + HIDDEN
    means[f0:h0] = inside(FRONT, torch.rand(FRONT, generator=g) * 0.8 + 0.8, 22.0, 18.0)
    log_scales[f0:h0] = math.log(0.03) + 0.2 * torch.randn(FRONT, 3, generator=g)
    logits[f0:h0] = 0.0
    means[h0:b0] = inside(HIDDEN, torch.rand(HIDDEN, generator=g) * 4 + 4, 22.0, 18.0)
    log_scales[h0:b0] = math.log(0.12) + 0.2 * torch.randn(HIDDEN, 3, generator=g)
    logits[h0:b0] = -0.5
    means[b0:] = torch.stack([-torch.rand(BEHIND, generator=g) * 5 - 1, torch.randn(BEHIND, generator=g), torch.randn(BEHIND, generator=g)], -1)
    log_scales[b0:] = math.log(0.1)
    quats[f0:] = torch.nn.functional.normalize(torch.randn(N - f0, 4, generator=g), dim=-1)
    sh = torch.zeros(N, 16, 3)
    sh[:, 0] = (torch.rand(N, 3, generator=g) - 0.5) / 0.28209479177387814
    sh[:, 1:] = torch.randn(N, 15, 3, generator=g) * 0.05
    p = dict(means=means, quats=quats, log_scales=log_scales, opacity_logits=logits, sh=sh)
    return {k: v.to(device).contiguous() for k, v in p.items()}


FRAME_YAWS = (0.0, 8.0)


def _eager_frame(frame, p, cams, grids, skies, targets):
    """The eager dense frame on the same parameters (selfcheck.frame_against_eager's driver): the five gradients summed over the
    views, per view (grad2d, absgrad2d), the pose gradients; the frame's own gradient tensors are put back afterwards."""
    from bilateral_driving_amd import harness as Hn
    leaves = list(frame.flat.params) + list(skies) + [c.viewmat for c in cams]
    try:
        for t in leaves:
            t.grad = None
        g2 = []
        for v, cam in enumerate(cams):
            out = Hn.render_view(p, cam, grids, v, skies[v])
            out["info"]["means2d"].retain_grad()
            Hn.training_loss(out, targets[v], grids, tv_weight=frame.tv_weight).backward()
            m2 = out["info"]["means2d"]
            g2.append((m2.grad[0].detach().clone(), m2.absgrad[0].detach().clone()))
        torch.cuda.synchronize()
        grads = {k: t.grad.detach().clone() for k, t in p.items()}
        pose = [c.viewmat.grad.detach().clone() for c in cams]
    finally:
        for t in leaves:
            t.grad = None
        frame._point_grads_at_flat()
        for v, vg in enumerate(frame.views):
            skies[v].grad, cams[v].viewmat.grad = vg.v_sky, vg.v_viewmat
    return grads, g2, pose


def _touched_rows(frame, N):
    """Per view: the rows of the ranks the view's last backward marked (bool [N]), and the mask by rank."""
    out = []
    for v in range(frame.V):
        nv = int(frame.counts()[v][1])
        ids = frame.prep_ws[v][frame._ids_off:frame._ids_off + 4 * nv].view(torch.int32).long()
        m = frame.touched[v][:nv].bool()
        rows = torch.zeros(N, dtype=torch.bool, device=ids.device)
        rows[ids[m]] = True
        out.append((rows, m, ids))
    return out


@pytest.mark.parametrize("mode", ["overlap", "one_stream", "recapture", "consume"])
def test_frame_rows_move_between_touched_and_untouched(env, mode):
    """Three frames -- wall opaque, transparent, opaque -- against the eager dense frame; every row outside a frame's touched set is
    exactly zero.  ``recapture``: the graphs are captured again between frame 1 and 2; ``consume``: ``clear_grads=False`` with
    ``FusedAdam(consume_grads=True)`` stepping between the frames."""
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.graph_view import FrameGraph
    from bilateral_driving_amd.optim import FusedAdam
    dev = "cuda"
    cams = Hn.ring_cameras(FW, FH, yaws_deg=FRAME_YAWS, device=dev)
    for c in cams:
        c.viewmat.requires_grad_(True)
    p = {k: t.requires_grad_(True) for k, t in wall_scene(dev).items()}
    N = p["means"].shape[0]
    grids = [g.requires_grad_(True) for g in Hn.make_grids(len(cams), device=dev)]
    gen = torch.Generator().manual_seed(5)
    skies = [torch.rand(FH, FW, 3, generator=gen).to(dev).requires_grad_(True) for _ in cams]
    targets = [torch.rand(FH, FW, 3, generator=gen).to(dev) for _ in cams]
    consume = mode == "consume"
    frame = FrameGraph(p, cams, grids, skies, targets, overlap=(mode != "one_stream"), clear_grads=not consume)
    opt = None
    if consume:
        groups = [{"params": [t], "lr": 1e-4, "eps": 1e-15} for t in list(p.values()) + grids]
        opt = FusedAdam(groups, lr=0.0, eps=1e-15, consume_grads=True)
    hidden = torch.arange(WALL + FRONT, WALL + FRONT + HIDDEN, device=dev)
    for f, wall_logit in enumerate((10.0, -10.0, 10.0)):
        with torch.no_grad():
            p["opacity_logits"][:WALL] = wall_logit
        if mode == "recapture" and f == 1:
            frame.recapture()
        assert frame.step() is True
        torch.cuda.synchronize()
        got = {k: frame.arena[k].detach().clone() for k in p}
        got2 = [frame.g2d[v].detach().clone() for v in range(frame.V)]
        got_pose = [c.viewmat.grad.detach().clone() for c in cams]
        views = _touched_rows(frame, N)
        any_rows = torch.zeros(N, dtype=torch.bool, device=dev)
        for rows, m, ids in views:
            any_rows |= rows
            assert bool(m.any()), (mode, f)                                             # at least one rank is touched in every view
        if wall_logit > 0:      # the wall hides: no hidden row is touched, and (frames 1 and 3) a whole 256-rank block is untouched
            assert not bool(any_rows[hidden].any()), (mode, f)
            full_blocks = [bool((~m[b:b + 256]).all()) for rows, m, ids in views for b in range(0, m.numel() - 255, 256)]
            assert any(full_blocks), (mode, f, [int(m.numel()) for _, m, _ in views])
        else:                   # every wall-hidden row is touched
            assert bool(any_rows[hidden].all()), (mode, f, int(any_rows[hidden].sum()))
        # every row outside the frame's touched set is exactly zero
        for k, t in got.items():
            assert float(t[~any_rows].abs().max()) == 0.0, (mode, f, k)
        for v, (rows, m, ids) in enumerate(views):
            assert float(got2[v][:, ~rows].abs().max()) == 0.0, (mode, f, v)
        # ... and the frame is the eager dense frame's
        ref, ref2, ref_pose = _eager_frame(frame, p, cams, grids, skies, targets)
        num = sum(float((got[k].double() - ref[k].double()).pow(2).sum()) for k in p)
        den = sum(float(ref[k].double().pow(2).sum()) for k in p)
        assert den > 0 and (num / den) ** 0.5 <= GRAD_TOL, (mode, f, (num / den) ** 0.5)
        for k in p:
            assert float((got[k].double() - ref[k].double()).norm()) <= GRAD_TOL * float(ref[k].double().norm()), (mode, f, k)
            assert float(ref[k][~any_rows].abs().max()) == 0.0, (mode, f, k)           # (the dense frame agrees on what is untouched)
        for v in range(frame.V):
            for i, name in ((0, "grad2d"), (1, "absgrad2d")):
                a, b = got2[v][i].double(), ref2[v][i].double()
                assert float(b.norm()) > 0 and float((a - b).norm()) <= GRAD_TOL * float(b.norm()), (mode, f, v, name)
            assert float((got_pose[v].double() - ref_pose[v].double()).norm()) <= FRAME_POSE_TOL * float(ref_pose[v].double().norm()), (mode, f, v)
        if opt is not None:
            opt.step()
            torch.cuda.synchronize()
            assert float(frame.flat.flat.abs().max()) == 0.0
