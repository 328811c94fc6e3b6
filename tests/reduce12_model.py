"""Lane-by-lane model of the two wave64 transpose-reduces of csrc/bds_common.h (butterfly_sum16 / butterfly_sum12) in float32:
the cross-lane moves of gfx950 on 64-entry arrays, the adds in the kernels' order.  Shared by tests/test_reduce12_model.py (CPU)
and tests/test_gpu_48_reduce12.py (the same assertions on the device's results)."""
import numpy as np

LANES = np.arange(64)
B2, B3 = ((LANES >> 2) & 1).astype(bool), ((LANES >> 3) & 1).astype(bool)
# documented lane -> value maps and the lanes that commit (one per quad; the 12-value form's quads with b2 & b3 are duplicates)
SLOT16 = ((LANES >> 2) & 1) + 2 * ((LANES >> 3) & 1) + 4 * (LANES >> 4)
SLOT12 = np.where(B2, 2, B3.astype(np.int64)) + 3 * ((LANES >> 4) & 1) + 6 * (LANES >> 5)
COMMIT12 = ((LANES & 3) == 0) & ~(B2 & B3)
COMMIT12_LANES = [0, 4, 8, 16, 20, 24, 32, 36, 40, 48, 52, 56]


def permlane32_swap(a, b):
    """v_permlane32_swap: lanes 32..63 of the first operand change places with lanes 0..31 of the second."""
    return np.concatenate([a[:32], b[:32]]), np.concatenate([a[32:], b[32:]])


def permlane16_swap(a, b):
    """v_permlane16_swap: the odd rows (of 16 lanes) of the first operand change places with the even rows of the second."""
    ra, rb = a.reshape(4, 16), b.reshape(4, 16)
    return np.stack([ra[0], rb[0], ra[2], rb[2]]).reshape(64), np.stack([ra[1], rb[1], ra[3], rb[3]]).reshape(64)


def row_ror8(v):
    return v[LANES ^ 8]          # DPP row_ror:8: a rotation by half a row


def row_half_mirror(v):
    return v[LANES ^ 7]          # DPP row_half_mirror: lane i <-> 7 - i inside every 8 lanes


def quad_perm_1032(v):
    return v[LANES ^ 1]


def quad_perm_2301(v):
    return v[LANES ^ 2]


def _swap_add(swap, a, b):
    r0, r1 = swap(a, b)
    return (r0 + r1).astype(np.float32)


def _tail(sa, sb):
    w = np.where(B2, sb, sa)
    w = (w + quad_perm_1032(w)).astype(np.float32)
    return (w + quad_perm_2301(w)).astype(np.float32)


def butterfly_sum16(v):
    """v [64 lanes][16 values] float32 -> [64]: what every lane holds on return."""
    v = np.asarray(v, np.float32)
    s = [_swap_add(permlane32_swap, v[:, i], v[:, i + 8]) for i in range(8)]
    t = [_swap_add(permlane16_swap, s[i], s[i + 4]) for i in range(4)]
    u = []
    for j in range(2):
        sa = (t[j] + row_ror8(t[j])).astype(np.float32)
        sb = (t[j + 2] + row_ror8(t[j + 2])).astype(np.float32)
        u.append(np.where(B3, sb, sa))
    return _tail((u[0] + row_half_mirror(u[0])).astype(np.float32), (u[1] + row_half_mirror(u[1])).astype(np.float32))


def butterfly_sum12(v):
    """v [64 lanes][12 values] float32 -> [64]."""
    v = np.asarray(v, np.float32)
    s = [_swap_add(permlane32_swap, v[:, i], v[:, i + 6]) for i in range(6)]
    t = [_swap_add(permlane16_swap, s[i], s[i + 3]) for i in range(3)]
    sa = (t[0] + row_ror8(t[0])).astype(np.float32)
    sb = (t[1] + row_ror8(t[1])).astype(np.float32)
    u0 = np.where(B3, sb, sa)
    u1 = (t[2] + row_ror8(t[2])).astype(np.float32)
    return _tail((u0 + row_half_mirror(u0)).astype(np.float32), (u1 + row_half_mirror(u1)).astype(np.float32))


def pad16(v12):
    v12 = np.asarray(v12, np.float32)
    return np.concatenate([v12, np.zeros((64, 4), np.float32)], 1)


def inputs():
    """(name, [64][12] float32) cases: random over six decades, cancelling triples, one-hot per (lane, value)."""
    rng = np.random.default_rng(48)
    out = []
    for r in range(200):
        mag = 10.0 ** rng.uniform(-3, 3, (64, 12))
        out.append((f"random{r}", (rng.standard_normal((64, 12)) * mag).astype(np.float32)))
    for r in range(8):
        v = np.zeros((64, 12), np.float32)
        for k in range(12):
            lanes = rng.permutation(64)
            for j in range(0, 63, 3):      # 1e8, -1e8, 1 on three lanes each: the total depends on the order of the adds
                v[lanes[j], k], v[lanes[j + 1], k], v[lanes[j + 2], k] = 1e8, -1e8, 1.0
        out.append((f"cancelling{r}", v))
    for lane in range(64):
        for k in range(12):
            v = np.zeros((64, 12), np.float32)
            v[lane, k] = 1.0 + k + 16.0 * lane      # (exact in float32; names its origin)
            out.append((f"onehot_l{lane}_k{k}", v))
    return out


def check(v12, got16, got12):
    """The assertions both tests make on the per-lane results of one input: the 12 totals bit-equal between the forms, in the lanes
    the documented maps name (and in all four lanes of every quad)."""
    got16, got12 = np.asarray(got16, np.float32), np.asarray(got12, np.float32)
    tot = np.full(12, np.nan, np.float32)
    for lane in range(64):
        if SLOT16[lane] < 12 and lane % 4 == 0:
            tot[SLOT16[lane]] = got16[lane]
    assert not np.isnan(tot).any()
    assert np.array_equal(got16.view(np.uint32)[SLOT16 < 12], tot[SLOT16[SLOT16 < 12]].view(np.uint32)), "16-value form: quads disagree"
    assert np.array_equal(got12.view(np.uint32), tot[SLOT12].view(np.uint32)), "12-value form: a total differs from the 16-value form's"
    ref = np.asarray(v12, np.float64).sum(0)
    scale = np.abs(np.asarray(v12, np.float64)).sum(0)
    assert np.all(np.abs(tot - ref) <= 64 * 2.0 ** -24 * scale + 1e-30), "a total is not the sum of its column"
