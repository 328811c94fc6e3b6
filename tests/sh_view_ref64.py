"""Float64 restatement of the one-view SH colour entries (test infrastructure): ``bds_sh_view_fwd``, ``bds_splat_pack_sh``,
``bds_sh_view_bwd_list`` and the row bookkeeping of ``bds_view_grads_clear_list`` / ``bds_view_grads_add_list``, built on
``oracle.gs_oracle.spherical_harmonics`` (models/gaussians/vanilla.py:383-389: SH of normalise(means - cam_pos), + 0.5, clamp to
[0, 1]).  Shared by tests/test_sh_view_ref64_cpu.py (the restatement against float64 autograd) and
tests/test_gpu_56_sh_view_forms.py (the kernels against the restatement).

The one decision that is NOT taken in float64 is the clamp's: the kernels decide from the float32 ``sh_rgb`` array they are handed,
as ``torch.clamp`` does on the reference's float32 colours, so ``clamp_pass`` forms ``sh_rgb + 0.5`` in float32 from the same bits."""
import math

import torch

from oracle import gs_oracle as G

KS = (1, 4, 5, 8, 9, 12, 16)
K_DEG = tuple((K, d) for K in KS for d in range(4) if (d + 1) ** 2 <= K)      # 17 pairs
LOG2E = 1.4426950408889634
SPLAT_RECORD_FLOATS, GRAD_RECORD_FLOATS = 12, 16                                # include/bds.h


def num_bases(deg: int) -> int:
    return (deg + 1) ** 2


def view_dirs(means, cam_pos):
    return means.double() - cam_pos.double()


def colour64(deg, means, cam_pos, coeffs):
    """The un-clamped colour ``sh_rgb`` [n,3] in float64; coeffs [n,K,3] with K >= (deg+1)^2."""
    return G.spherical_harmonics(deg, view_dirs(means, cam_pos), coeffs.double())


def packed_colour(sh):
    """What the compositor gets: clamp(sh + 0.5, 0, 1), in the dtype of ``sh``."""
    return (sh + 0.5).clamp(0.0, 1.0)


def clamp_pass(sh_rgb32):
    """Where the clamp passes the gradient: the CLOSED interval 0 <= sh_rgb + 0.5 <= 1 with the sum formed in float32."""
    assert sh_rgb32.dtype == torch.float32
    x = sh_rgb32 + torch.tensor(0.5, dtype=torch.float32, device=sh_rgb32.device)
    return (x >= 0) & (x <= 1)


def coeff_grad_rows(K, deg, means, cam_pos, v_records, sh_rgb32):
    """Rows [n,K,3] (float64) of d loss / d coeffs for the entries whose gradient records are ``v_records`` [n,16] (colour gradient =
    floats 0-2), positions ``means`` [n,3] and un-clamped float32 colours ``sh_rgb32`` [n,3]: basis value x gated colour gradient for
    the bands below (deg+1)^2, exact zeros above."""
    nb = num_bases(deg)
    assert K >= nb and v_records.shape[-1] == GRAD_RECORD_FLOATS
    B = G.sh_bases(deg, view_dirs(means, cam_pos))                                          # [n,nb]
    v = v_records[:, :3].double() * clamp_pass(sh_rgb32).to(torch.float64)
    rows = torch.zeros(means.shape[0], K, 3, dtype=torch.float64, device=means.device)
    rows[:, :nb] = B[:, :, None] * v[:, None, :]
    return rows


def split_rows(rows):
    """[N,K,3] -> (dc [N,3], rest [N,K-1,3]), the reference's two parameters (vanilla.py:96-104), each contiguous."""
    return rows[:, 0, :].contiguous(), rows[:, 1:, :].contiguous()


def join_rows(dc, rest):
    """The inverse of ``split_rows`` (vanilla.py:382)."""
    return torch.cat([dc[:, None, :], rest], dim=1)


def destination_rows(ids, row_map=None):
    """The row of the gradient array that entry r of the list lands in: ids[r], or row_map[ids[r]]."""
    ids = ids.long()
    return ids if row_map is None else row_map.long()[ids]


def scatter_rows(prior, ids, rows, row_map=None, accumulate=False):
    """``prior`` [R,K,3] (float64) with the list's rows stored, or added to."""
    out = prior.clone()
    dst = destination_rows(ids, row_map)
    out[dst] = (out[dst] + rows) if accumulate else rows
    return out


def splat_records(ids, means2d, conics, opacities, depths, radii, sh):
    """The 12-float splat records of the entries ``ids`` as include/bds.h states them: [n,12] float64 with
    0-1 means2d | 2-4 the conic in base-2 units (-log2e/2 a, -log2e b, -log2e/2 c) | 5 opacity | 6-8 clamp(sh + 0.5, 0, 1) | 9 depth |
    10 zero; slot 11 holds the radius' integer BITS and is returned separately (int32 [n])."""
    il = ids.long()
    rec = torch.zeros(il.numel(), SPLAT_RECORD_FLOATS, dtype=torch.float64, device=means2d.device)
    cn = conics.double()[il]
    rec[:, 0:2] = means2d.double()[il]
    rec[:, 2] = -0.5 * LOG2E * cn[:, 0]
    rec[:, 3] = -LOG2E * cn[:, 1]
    rec[:, 4] = -0.5 * LOG2E * cn[:, 2]
    rec[:, 5] = opacities.double()[il]
    rec[:, 6:9] = packed_colour(sh.double())
    rec[:, 9] = depths.double()[il]
    return rec, radii[il].to(torch.int32)


def degree_of(K: int) -> int:
    """The class's sh_degree for K coefficients (K a square)."""
    d = math.isqrt(K) - 1
    assert (d + 1) ** 2 == K
    return d
