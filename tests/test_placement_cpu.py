"""tests/placement.py on the host: ``placed`` yields the stated alignment, contiguity and values for every dtype and offset the GPU
tests use, ``regrad`` hands a node's backward a gradient at the chosen phase, and ``cat_grad`` is the source of such gradients in
autograd itself."""
import pytest
import torch

from tests import placement as PL

CASES = [(dt, off) for dt, offs in PL.OFFSETS.items() for off in (0,) + tuple(offs)]


def _values(dtype, shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) > 0.5
    if dtype.is_floating_point:
        return torch.randn(shape, generator=g).to(dtype)
    return torch.randint(0, 200, shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype,off", CASES, ids=[f"{str(d)[6:]}-off{o}" for d, o in CASES])
@pytest.mark.parametrize("shape", [(1,), (5,), (7, 3), (4, 5, 3)], ids=["1", "5", "7x3", "4x5x3"])
def test_placed_has_the_stated_alignment_contiguity_and_values(dtype, off, shape):
    t = _values(dtype, shape)
    p = PL.placed(t, off)
    assert p.dtype == t.dtype and p.shape == t.shape and p.device == t.device
    assert p.is_contiguous() and p.contiguous().data_ptr() == p.data_ptr()      # what ``.contiguous()`` in a wrapper returns: itself
    assert PL.phase(p) == (off * t.element_size()) % 16
    assert torch.equal(p, t)
    assert not p.requires_grad
    if t.numel():
        assert p.data_ptr() != t.data_ptr()
        keep = t.clone()
        p.view(-1)[0] = not bool(p.view(-1)[0]) if dtype == torch.bool else p.view(-1)[0] + 1       # a copy, not a view
        assert torch.equal(t, keep)


def test_every_offset_of_a_four_byte_type_is_a_distinct_misaligned_phase():
    for dt in (torch.float32, torch.int32):
        assert sorted(PL.phase(PL.placed(torch.zeros(9, dtype=dt), o)) for o in (0,) + PL.OFFSETS[dt]) == [0, 4, 8, 12]
    assert [PL.phase(PL.placed(torch.zeros(9, dtype=torch.uint8), o)) for o in PL.OFFSETS[torch.uint8]] == [1, 5]
    assert PL.phase(PL.placed(torch.zeros(9, dtype=torch.int64), 1)) == 8


class _Probe(torch.autograd.Function):
    """Identity that records what its backward was handed."""
    seen = []

    @staticmethod
    def forward(ctx, t):
        return t * 1.0

    @staticmethod
    def backward(ctx, g):
        _Probe.seen.append((PL.phase(g), g.is_contiguous(), g.clone()))
        return g


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_regrad_replaces_the_gradient_and_nothing_else(off):
    _Probe.seen.clear()
    x = torch.randn(7, 3, requires_grad=True)
    w = torch.randn(7, 3)
    y = PL.regrad(_Probe.apply(x), off)
    assert torch.equal(y.detach(), x.detach())
    (y * w).sum().backward()
    (ph, contig, g), = _Probe.seen
    assert ph == 4 * off and contig
    assert torch.equal(g, w) and torch.equal(x.grad, w)


@pytest.mark.parametrize("n_first", [1, 2, 3, 5])
def test_cat_hands_the_second_part_a_view_at_the_first_parts_phase(n_first):
    """No ``regrad`` here: the misaligned gradient is autograd's own (``n_first`` rows of three floats in front of it)."""
    _Probe.seen.clear()
    a = torch.randn(n_first, 3, requires_grad=True)
    b = torch.randn(6, 3, requires_grad=True)
    w = torch.randn(n_first + 6, 3)
    out = PL.cat_grad([_Probe.apply(a), _Probe.apply(b)])
    (out * w).sum().backward()
    by_rows = {g.shape[0]: (ph, contig, g) for ph, contig, g in _Probe.seen}
    assert len(_Probe.seen) == 2
    ph, contig, g = by_rows[6] if n_first != 6 else _Probe.seen[1]
    assert contig and ph == (4 * 3 * n_first) % 16 and ph != 0
    assert torch.equal(g, w[n_first:]) and torch.equal(b.grad, w[n_first:]) and torch.equal(a.grad, w[:n_first])
