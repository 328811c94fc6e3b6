"""The float64 restatement of the one-view SH colour entries (tests/sh_view_ref64.py) against float64 autograd through
clamp(SH + 0.5, 0, 1): the analytic coefficient-gradient rows, the exact zeros of the unused bands, the clamp's closed interval at
planted values, the split / join round trip and the record layout.  No GPU, no library."""
import pytest
import torch

from tests import sh_view_ref64 as R


def _inputs(K, n=97, seed=0):
    g = torch.Generator().manual_seed(1000 * K + seed)
    means = torch.randn(n, 3, generator=g, dtype=torch.float64) * 3
    cam_pos = torch.randn(3, generator=g, dtype=torch.float64)
    coeffs = torch.randn(n, K, 3, generator=g, dtype=torch.float64) * 2.0
    v_rec = torch.randn(n, R.GRAD_RECORD_FLOATS, generator=g, dtype=torch.float64)
    return means, cam_pos, coeffs, v_rec


def test_the_matrix_has_seventeen_pairs():
    assert len(R.K_DEG) == 17 and len(set(R.K_DEG)) == 17
    assert all((d + 1) ** 2 <= K for K, d in R.K_DEG) and {K for K, _ in R.K_DEG} == set(R.KS)
    assert (4, 1) in R.K_DEG and (9, 2) in R.K_DEG and (16, 3) in R.K_DEG and (8, 2) not in R.K_DEG


@pytest.mark.parametrize("K,deg", R.K_DEG)
def test_rows_equal_autograd_through_the_clamp(K, deg):
    means, cam_pos, coeffs, v_rec = _inputs(K)
    c = coeffs.clone().requires_grad_(True)
    sh = R.colour64(deg, means, cam_pos, c)
    x = sh.detach() + 0.5
    # (the restatement decides the clamp in float32: keep the comparison away from the two places where float32 could decide otherwise)
    assert float(torch.minimum(x.abs(), (x - 1).abs()).min()) > 1e-5
    assert bool((x < 0).any()) and bool((x > 1).any()) and bool(((x > 0) & (x < 1)).any())     # all three branches are exercised
    (R.packed_colour(sh) * v_rec[:, :3]).sum().backward()
    rows = R.coeff_grad_rows(K, deg, means, cam_pos, v_rec, sh.detach().float())
    assert rows.shape == (means.shape[0], K, 3) and rows.dtype == torch.float64
    assert float((rows - c.grad).abs().max()) <= 1e-14 * float(c.grad.abs().max())
    nb = R.num_bases(deg)
    assert bool((rows[:, nb:] == 0).all()) and bool((c.grad[:, nb:] == 0).all())               # bands >= nb: exact zeros
    assert float(rows[:, :nb].abs().max()) > 0


def test_the_clamp_passes_the_gradient_on_the_closed_interval():
    f32 = torch.float32
    lo, hi = torch.tensor(-0.5, dtype=f32), torch.tensor(0.5, dtype=f32)
    below = torch.nextafter(lo, torch.tensor(-1.0, dtype=f32))                 # sh + 0.5 = -2^-24: outside
    # the float32 neighbour of sh + 0.5 = 1 on the outside is 1 + 2^-23, reached from sh = 0.5 + 2^-23 (the sum is exact)
    above = torch.nextafter(torch.tensor(1.0, dtype=f32), torch.tensor(2.0, dtype=f32)) - hi
    assert float(above + hi) == 1.0 + 2.0 ** -23 and float(below + hi) == -(2.0 ** -24)
    # nextafter(0.5) itself: sh + 0.5 = 1 + 2^-24 rounds (to even) to exactly 1 in float32 -- torch.clamp on float32 colours passes it too
    tie = torch.nextafter(hi, torch.tensor(1.0, dtype=f32))
    sh = torch.stack([lo, hi, below, above, tie, torch.tensor(0.0, dtype=f32)])
    want = torch.tensor([True, True, False, False, True, True])
    assert torch.equal(R.clamp_pass(sh), want)
    x = sh.clone().requires_grad_(True)                                        # torch's own float32 clamp takes the same decisions
    (x + 0.5).clamp(0.0, 1.0).sum().backward()
    assert torch.equal(x.grad != 0, want)
    # through the rows: a planted sh_rgb decides, whatever the coefficients say
    K, deg = 4, 1
    means, cam_pos, coeffs, v_rec = _inputs(K, n=6)
    planted = sh[:, None].expand(6, 3).contiguous()
    rows = R.coeff_grad_rows(K, deg, means, cam_pos, v_rec, planted)
    for r in range(6):
        assert bool((rows[r] == 0).all()) == (not bool(want[r]))
    mixed = torch.stack([lo, below, hi])[None].expand(6, 3).contiguous()       # per channel, not per row
    rows = R.coeff_grad_rows(K, deg, means, cam_pos, v_rec, mixed)
    assert bool((rows[:, :, 1] == 0).all()) and bool((rows[:, :, 0] != 0).all()) and bool((rows[:, :, 2] != 0).all())


@pytest.mark.parametrize("K", [k for k in R.KS if k >= 2])
def test_split_and_join_round_trip(K):
    rows = torch.randn(13, K, 3, dtype=torch.float64)
    dc, rest = R.split_rows(rows)
    assert dc.shape == (13, 3) and rest.shape == (13, K - 1, 3) and dc.is_contiguous() and rest.is_contiguous()
    assert torch.equal(dc, rows[:, 0]) and torch.equal(rest[:, 0], rows[:, 1]) and torch.equal(rest[:, -1], rows[:, -1])
    assert torch.equal(R.join_rows(dc, rest), rows)
    # the flat row of the joined array is band 0 followed by the rest's flat row: the piece arithmetic of the split kernels
    flat = R.join_rows(dc, rest).reshape(13, K * 3)
    assert torch.equal(flat[:, :3], dc) and torch.equal(flat[:, 3:], rest.reshape(13, (K - 1) * 3))


def test_scatter_rows_store_accumulate_and_row_map():
    g = torch.Generator().manual_seed(3)
    prior = torch.randn(9, 4, 3, generator=g, dtype=torch.float64)
    rows = torch.randn(3, 4, 3, generator=g, dtype=torch.float64)
    ids = torch.tensor([7, 2, 5], dtype=torch.int32)
    out = R.scatter_rows(prior, ids, rows)
    assert torch.equal(out[[7, 2, 5]], rows) and torch.equal(out[[0, 1, 3, 4, 6, 8]], prior[[0, 1, 3, 4, 6, 8]])
    out = R.scatter_rows(prior, ids, rows, accumulate=True)
    assert torch.equal(out[[7, 2, 5]], prior[[7, 2, 5]] + rows)
    row_map = torch.full((9,), -1, dtype=torch.int32)
    row_map[[7, 2, 5]] = torch.tensor([0, 8, 3], dtype=torch.int32)
    assert torch.equal(R.destination_rows(ids, row_map), torch.tensor([0, 8, 3]))
    out = R.scatter_rows(prior, ids, rows, row_map=row_map)
    assert torch.equal(out[[0, 8, 3]], rows) and torch.equal(out[[1, 2, 4, 5, 6, 7]], prior[[1, 2, 4, 5, 6, 7]])


def test_record_layout():
    g = torch.Generator().manual_seed(4)
    N = 11
    m2, con = torch.rand(N, 2, generator=g) * 100, torch.rand(N, 3, generator=g) + 0.1
    opac, dep = torch.rand(N, generator=g), torch.rand(N, generator=g) * 10
    radii = torch.randint(1, 50, (N,), generator=g, dtype=torch.int32)
    ids = torch.tensor([4, 0, 9], dtype=torch.int32)
    sh = torch.tensor([[-0.7, 0.1, 0.9], [0.0, -0.5, 0.5], [0.2, 0.3, 0.4]], dtype=torch.float64)
    rec, rad = R.splat_records(ids, m2, con, opac, dep, radii, sh)
    assert rec.shape == (3, R.SPLAT_RECORD_FLOATS) and torch.equal(rad, radii[[4, 0, 9]])
    assert torch.equal(rec[:, :2], m2.double()[[4, 0, 9]]) and torch.equal(rec[:, 5], opac.double()[[4, 0, 9]])
    assert torch.equal(rec[:, 9], dep.double()[[4, 0, 9]]) and bool((rec[:, 10] == 0).all())
    assert torch.equal(rec[:, 6:9], torch.tensor([[0.0, 0.6, 1.0], [0.5, 0.0, 1.0], [0.7, 0.8, 0.9]], dtype=torch.float64))
    # the conic in base-2 units: exp2(rec . (dx^2, dx dy, dy^2)) = exp(-(a dx^2 + 2 b dx dy + c dy^2) / 2)
    dx, dy = 0.7, -1.3
    a, b, c = con.double()[4]
    q2 = rec[0, 2] * dx * dx + rec[0, 3] * dx * dy + rec[0, 4] * dy * dy
    assert abs(float(torch.exp2(q2)) - float(torch.exp(-0.5 * (a * dx * dx + 2 * b * dx * dy + c * dy * dy)))) < 1e-14
