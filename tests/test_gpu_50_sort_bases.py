"""-m gpu: the tile stage's workgroup-major radix passes at the boundaries of their partial histogram rows (csrc/tiles.hip
grouped_bases: a scatter workgroup's bases = the group rows in front of its group of 64 workgroups + the sub-group rows in front of
its sub-group of 8 + the workgroup rows in front of itself), against ``oracle.gs_oracle.isect_tiles`` BIT FOR BIT: tiles_per_gauss,
isect_ids, flatten_ids, isect_offsets.

The inputs of ``gs_ops.isect_tiles`` are built directly, one camera, no projection: a visible Gaussian sits at the centre of a 16-px
tile with radius 1, so it touches exactly that tile -- the list length M equals the visible count, and both are set exactly.

Short passes (chunks of 1024 pairs; 256 x 256 image, 256 tiles, N = 80 x 1024 rows, the rest with radius 0): visible counts
1024 k - 1, 1024 k, 1024 k + 1 for k in 1, 7, 8, 9 (a sub-group's edge), 63, 64, 65, 72, 73 (a group's edge, and the second group's
first sub-group edge), with five inputs each: random depths; depths whose upper two bytes take three values (a chunk then hits ONE
counter in the third and fourth pass); all depths equal (stability: ids ascending per tile); and the visible rows as one block at the
end, and at the start, of the rows -- for counts up to 2048 that is "only in the last / first 2048-row scan tile" to the letter, for
larger counts the block cannot fit one scan tile and is the nearest input that still has whole scan tiles without an entry in front
(the compaction's offset stays 0 over its early-outs) or behind (the early-outs carry the full offset).

Wide pass (chunks of 4096 packed entries; 512 x 256 image, 512 lists, 9-bit tile key, one pass): M = 4096 k - 1, 4096 k, 4096 k + 1 for
k in 1, 7, 8, 9, 64, 65; tiles filled evenly, all pairs in one tile, every second tile empty.  Packed entries on take the wide pass, off
the 8-bit passes over (key, id) pairs: both must equal the oracle; with the 64-bit keys not asked for the wide pass also writes the
offsets itself, which is checked as well.

Every input runs with OPT_SHORT_SORT and OPT_PACKED both ways; the reference is computed once per input.  The device-count form (the
one-view projection leaves the visible counts and clears the tables, capacities instead of counts) goes through one small frame:
graph_view's replay against the eager harness.render_view, images bit-equal."""
import pytest
import torch

from oracle import gs_oracle as G

pytestmark = pytest.mark.gpu

TS = 16
N_SHORT = 80 * 1024
SHORT_KS = (1, 7, 8, 9, 63, 64, 65, 72, 73)
SHORT_COUNTS = [1024 * k + e for k in SHORT_KS for e in (-1, 0, 1)]
SHORT_SETS = ("random", "hot_upper_bytes", "equal", "block_last", "block_first")
WIDE_KS = (1, 7, 8, 9, 64, 65)
WIDE_COUNTS = [4096 * k + e for k in WIDE_KS for e in (-1, 0, 1)]
WIDE_FILLS = ("even", "one_tile", "every_second_empty")
N_WIDE = 264 * 1024


def _scene(N, rows, tiles, depths_vis, tw):
    """rows: ascending row indices of the visible Gaussians; tiles / depths_vis: their tile and depth."""
    m2 = torch.zeros(N, 2)
    radii = torch.zeros(N, dtype=torch.int32)
    d = torch.zeros(N)
    m2[rows, 0] = ((tiles % tw) * TS + TS // 2).float()
    m2[rows, 1] = ((tiles // tw) * TS + TS // 2).float()
    radii[rows] = 1
    d[rows] = depths_vis
    return m2, radii, d


def _short_case(count, kind):
    g = torch.Generator().manual_seed(1000 * count + SHORT_SETS.index(kind))
    tw = th = 256 // TS
    if kind == "block_last":
        rows = torch.arange(N_SHORT - count, N_SHORT)
    elif kind == "block_first":
        rows = torch.arange(count)
    else:
        rows = torch.randperm(N_SHORT, generator=g)[:count].sort().values
    tiles = torch.randint(0, tw * th, (count,), generator=g)
    if kind == "hot_upper_bytes":     # fp32 bits 0x40400000 | 0x41200000 | 0x42480000 + random lower two bytes: 3.0.., 10.0.., 50.0..
        hi = torch.tensor([0x4040, 0x4120, 0x4248], dtype=torch.int32)[torch.randint(0, 3, (count,), generator=g)]
        depths = ((hi << 16) | torch.randint(0, 1 << 16, (count,), generator=g, dtype=torch.int32)).view(torch.float32)
    elif kind == "equal":
        depths = torch.full((count,), 7.5)
    else:
        depths = torch.rand(count, generator=g) * 99.0 + 0.5
    return _with_reference(_scene(N_SHORT, rows, tiles, depths, tw), tw, th)


def _wide_case(count, fill):
    g = torch.Generator().manual_seed(7000 * count + WIDE_FILLS.index(fill))
    tw, th = 512 // TS, 256 // TS
    rows = torch.randperm(N_WIDE, generator=g)[:count].sort().values
    i = torch.arange(count)
    tiles = {"even": i % (tw * th), "one_tile": torch.full((count,), 301), "every_second_empty": 2 * (i % (tw * th // 2))}[fill]
    tiles = tiles[torch.randperm(count, generator=g)]
    depths = torch.rand(count, generator=g) * 99.0 + 0.5
    return _with_reference(_scene(N_WIDE, rows, tiles, depths, tw), tw, th)


def _with_reference(scene, tw, th):
    m2, radii, d = scene
    tpg, keys, vals = G.isect_tiles(m2, radii, d, TS, tw, th)
    offs = G.isect_offset_encode(keys, tw, th)
    return m2, radii, d, tw, th, tpg, keys, vals, offs


def _check(case, count, tag, fused_offsets=False):
    import bilateral_driving_amd.gs_ops as ops
    from bilateral_driving_amd import _lib as L
    L.lib()
    m2, radii, d, tw, th, tpg_r, keys_r, vals_r, offs_r = case
    assert keys_r.numel() == count and int((radii > 0).sum()) == count, tag      # one tile per visible Gaussian
    dm2, dr, dd = m2.cuda()[None], radii.cuda()[None], d.cuda()[None]
    try:
        for short in (0, 1):
            for packed in (0, 1):
                L.set_option(L.OPT_SHORT_SORT, short); L.set_option(L.OPT_PACKED, packed)
                tpg, iids, fids, offs = ops.isect_tiles(dm2, dr, dd, TS, tw, th)
                t = (tag, dict(short=short, packed=packed))
                assert torch.equal(tpg.cpu()[0], tpg_r), t
                assert iids.numel() == count and torch.equal(iids.cpu(), keys_r), t
                assert torch.equal(fids.cpu(), vals_r), t
                assert torch.equal(offs.cpu()[0], offs_r), t
                if fused_offsets:    # (no 64-bit keys: a single wide pass leaves the per-tile offsets itself)
                    tpg, _, fids, offs = ops.isect_tiles(dm2, dr, dd, TS, tw, th, want_isect_ids=False)
                    assert torch.equal(tpg.cpu()[0], tpg_r) and torch.equal(fids.cpu(), vals_r) and torch.equal(offs.cpu()[0], offs_r), t
    finally:
        L.set_option(L.OPT_SHORT_SORT, 1); L.set_option(L.OPT_PACKED, 1)


@pytest.mark.parametrize("kind", SHORT_SETS)
@pytest.mark.parametrize("count", SHORT_COUNTS)
def test_short_passes_at_row_boundaries(count, kind):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    case = _short_case(count, kind)
    if kind == "equal":      # stability, stated on the reference itself: per tile the ids ascend
        keys, vals = case[6], case[7].long()
        assert bool(((keys[1:] != keys[:-1]) | (vals[1:] > vals[:-1])).all())
    _check(case, count, dict(count=count, kind=kind))


@pytest.mark.parametrize("fill", WIDE_FILLS)
@pytest.mark.parametrize("count", WIDE_COUNTS)
def test_wide_pass_at_row_boundaries(count, fill):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    _check(_wide_case(count, fill), count, dict(count=count, fill=fill), fused_offsets=True)


def test_device_count_form_small_frame_replay_equals_eager():
    """capacities >= 0, the one-view projection leaving the counts: FrameGraph's replay against eager harness.render_view."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.graph_view import FrameGraph
    from bilateral_driving_amd.selfcheck import frame_against_eager
    dev, W, H = "cuda", 256, 192
    cams = Hn.ring_cameras(W, H, device=dev)[:2]
    for c in cams:
        c.viewmat.requires_grad_(True)
    p = {k: t.requires_grad_(True) for k, t in Hn.synthetic_scene(2000, seed=3, device=dev).items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(len(cams), levels=Hn.LEVELS_3, device=dev)]
    gen = torch.Generator().manual_seed(11)
    skies = [torch.rand(H, W, 3, generator=gen).to(dev).requires_grad_(True) for _ in cams]
    targets = [torch.rand(H, W, 3, generator=gen).to(dev) for _ in cams]
    frame = FrameGraph(p, cams, grids, skies, targets, factors=Hn.FACTORS_3)
    for rep in range(2):
        res = frame_against_eager(frame, p, cams, grids, skies, targets, Hn.FACTORS_3)
        assert res["image_bit_equal"] and res["ok"], (rep, res)
    assert all(M > 0 and 0 < nv <= 2000 for M, nv in frame.counts()), frame.counts()
