"""-m gpu: the tile stage's radix passes (csrc/tiles.hip) at the lengths at which a pass can go wrong, through the public entry
``gs_ops.isect_tiles``, in all four regimes of the size hooks (two-launch short passes | generic passes; packed entries | pairs).

A pass cuts its input into chunks of 1024 (short form) or 4096 entries (the other forms), one workgroup each, and the grouped forms
sum 64 chunks' histograms into a group row.  The visible counts n sit on those boundaries:

    1                             smallest input
    1023, 1024, 1025              the short form's chunk
    4095, 4096, 4097              the other forms' chunk
    65535, 65536, 65537           first group boundary of the short form (64 chunks of 1024)
    262143, 262144, 262145        first group boundary of the wide form (64 chunks of 4096); five group rows of the short form, so
                                  that the group loop's unrolled step and its remainder both run
    5 * 262144 + 4097             the same for the wide form; a ragged last chunk; row remainders of both unrolled row loops

Every Gaussian covers exactly one tile (radius 1 around the centre of a tile drawn at random), so M = n and the expected lists are a
stable sort of n keys.  About a fifth of the rows are invisible (radius 0), mixed in at random, so that the compaction takes part; the
depths are random bit patterns of positive normal floats, so that all four digits of the depth sort vary, and every fourth row carries
one shared depth, so that stability decides the order.  The tile grids give a tile key of 8 bits (one 8-bit pass), 9 and 10 bits (the
single wide pass, <512> and <1024>) and 13 bits (two passes; packed entries fall back to pairs on their own above 2^19 visible rows).

Expected: tiles_per_gauss = the visibility mask; isect_ids = the keys  tile << 32 | depth bits  under torch.sort(stable=True);
flatten_ids = the visible rows' indices in that order; isect_offsets = searchsorted of the sorted tile numbers (as test_gpu_33 forms
it).  At n <= 4097 the same expectation is also tied to oracle.gs_oracle.isect_tiles (beyond that the oracle takes seconds).
All outputs are integers: equal means bit-equal."""
import functools

import pytest
import torch

from oracle import gs_oracle as G

pytestmark = pytest.mark.gpu

LENGTHS = [1, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 262143, 262144, 262145, 5 * 262144 + 4097]
GRIDS = [(16, 16, 16), (30, 17, 64), (40, 20, 64), (120, 68, 16)]      # tiles across, tiles down, tile size in px
REGIMES = [(1, 1), (0, 1), (1, 0), (0, 0)]      # options 4 (short sort) and 6 (packed entries)
ORACLE_MAX = 4097


@functools.lru_cache(maxsize=1)
def case(n, grid):
    """Inputs on the device and the expected outputs, formed once per (n, grid) and left unchanged."""
    tw, th, ts = grid
    g = torch.Generator(device="cuda").manual_seed(1000 * n + tw)
    N = n + max(1, n // 4)
    vis = torch.zeros(N, dtype=torch.bool, device="cuda")
    vis[torch.randperm(N, generator=g, device="cuda")[:n]] = True
    tile = torch.randint(0, tw * th, (N,), generator=g, device="cuda")
    means2d = torch.stack([(tile % tw).float() + 0.5, (tile // tw).float() + 0.5], 1) * ts
    dbits = torch.randint(0x00800000, 0x7f7fffff + 1, (N,), generator=g, device="cuda", dtype=torch.int64)
    dbits[::4] = int(dbits[0])
    depths = dbits.to(torch.int32).view(torch.float32)
    radii = vis.to(torch.int32)
    rows = torch.nonzero(vis).reshape(-1)
    keys, order = torch.sort((tile[rows] << 32) | dbits[rows], stable=True)
    offsets = torch.searchsorted((keys >> 32).contiguous(), torch.arange(tw * th, device="cuda")).to(torch.int32).reshape(1, th, tw)
    want = (radii[None], keys, rows[order].to(torch.int32), offsets)
    if n <= ORACLE_MAX:
        t, k, v = G.isect_tiles(means2d.cpu(), radii.cpu(), depths.cpu(), ts, tw, th)
        assert torch.equal(t, want[0][0].cpu()) and torch.equal(k, keys.cpu()) and torch.equal(v, want[2].cpu())
        assert torch.equal(G.isect_offset_encode(k, tw, th), offsets[0].cpu())
    return (means2d[None].contiguous(), radii[None].contiguous(), depths[None].contiguous()), want


@pytest.mark.parametrize("regime", REGIMES, ids=lambda r: f"short{r[0]}-packed{r[1]}")
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}px")
@pytest.mark.parametrize("n", LENGTHS)
def test_lists_are_the_stable_sort_of_the_keys(n, grid, regime):
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import bilateral_driving_amd.gs_ops as ops
    from bilateral_driving_amd import _lib as L
    L.lib()
    tw, th, ts = grid
    (means2d, radii, depths), (want_tpg, want_keys, want_ids, want_off) = case(n, grid)
    try:
        L.set_option(L.OPT_SHORT_SORT, regime[0]); L.set_option(L.OPT_PACKED, regime[1])
        for want_isect_ids in (True, False):
            tag = dict(n=n, grid=grid, regime=regime, want_isect_ids=want_isect_ids)
            tpg, iids, fids, offs = ops.isect_tiles(means2d, radii, depths, ts, tw, th, want_isect_ids=want_isect_ids)
            assert torch.equal(tpg, want_tpg), tag
            assert fids.numel() == n and torch.equal(fids, want_ids), tag
            assert torch.equal(offs, want_off), tag
            if want_isect_ids:
                assert iids.numel() == n and torch.equal(iids, want_keys), tag
            else:
                assert iids is None, tag
    finally:
        L.set_option(L.OPT_SHORT_SORT, 1); L.set_option(L.OPT_PACKED, 1)
