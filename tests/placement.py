"""Where a test's inputs lie in memory.  ``torch.rand(...).cuda()``, ``torch.from_numpy(...).cuda()`` and ``.clone()`` are fresh
allocations whose ``data_ptr()`` is 512-byte aligned; a contiguous row slice ``t[k:]`` of an [N,3] tensor, the gradient autograd hands
a node whose output went into a ``torch.cat`` along dim 0, and a sub-tensor of a flat buffer are contiguous too, at 4-byte alignment
only.  The library picks forms by ``aligned16(ptr)`` (16-byte loads or float by float), refuses some arrays with BDS_EINVAL and reads
others with 8- / 16-byte loads whatever their phase; these helpers hand an op its inputs and incoming gradients at a chosen phase.

``placed(t, off)``   the values of ``t`` on its device, contiguous, ``off`` elements behind a fresh allocation's base
``regrad(t, off)``   identity whose backward hands the incoming gradient on re-placed at ``off``
``cat_grad(parts)``  ``torch.cat(parts, 0)``: autograd's own source of such gradients (d cat / d parts[i] is a ``narrow`` of the gradient)
``OFFSETS``          the offsets worth testing per dtype"""
import torch

# element offsets behind a 16-byte boundary: every phase of a 4-byte type, an odd and a beyond-one-word phase of a byte mask, the one
# phase of an 8-byte index
OFFSETS = {torch.float32: (1, 2, 3), torch.int32: (1, 2, 3), torch.uint8: (1, 5), torch.bool: (1, 5), torch.int64: (1,)}


def phase(t):
    """Bytes between ``t``'s first element and the 16-byte boundary in front of it."""
    return t.data_ptr() % 16


def placed(t, off):
    """``t``'s values on its device as a contiguous tensor whose base lies ``off`` elements behind a fresh allocation's (``off`` = 0: a
    fresh aligned copy).  Never ``t`` itself and never a view of it; ``requires_grad`` is not carried over (the result is a new leaf)."""
    assert off >= 0
    src = t.detach()
    flat = torch.empty(src.numel() + off, dtype=src.dtype, device=src.device)
    assert flat.data_ptr() % 16 == 0, "a fresh allocation is 16-byte aligned"
    if off:
        flat[:off] = 0
    body = flat[off:].view(src.shape)
    body.copy_(src)
    assert src.numel() > 0, "an empty tensor has no first element to place"
    assert body.is_contiguous() and phase(body) == (off * src.element_size()) % 16, (phase(body), off, src.dtype)
    return body


class _Regrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, off):
        ctx.off = off
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return placed(g, ctx.off), None


def regrad(t, off):
    """``t`` itself to the forward pass; in the backward pass the node that produced ``t`` receives its gradient as
    ``placed(g, off)``: the alignment autograd would hand it behind a ``cat``, chosen deterministically."""
    return _Regrad.apply(t, off)


def cat_grad(parts):
    """``torch.cat(parts, 0)``.  The gradient that reaches ``parts[i]`` is ``grad.narrow(0, start_i, len_i)``: a contiguous view whose
    phase is ``4 * start_i * row_floats % 16``."""
    return torch.cat(list(parts), 0)
