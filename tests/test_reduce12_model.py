"""CPU: the 12-value wave64 transpose-reduce (csrc/bds_common.h butterfly_sum12) against the 16-value one it replaces where at most
12 values are live, on a lane-by-lane float32 model of v_permlane32_swap / v_permlane16_swap and the DPP controls
(tests/reduce12_model.py).  Every value goes through the same pairing sequence in both forms, so the 12 totals are bit-equal;
tests/test_gpu_48_reduce12.py makes the same assertions on the device's results."""
import numpy as np
import pytest

from tests import reduce12_model as M


def test_slot_maps_and_committing_lanes():
    lanes = np.arange(64)
    assert M.SLOT12.tolist() == [(2 if (l >> 2) & 1 else (l >> 3) & 1) + 3 * ((l >> 4) & 1) + 6 * (l >> 5) for l in range(64)]
    assert lanes[M.COMMIT12].tolist() == M.COMMIT12_LANES
    assert sorted(M.SLOT12[M.COMMIT12].tolist()) == list(range(12))            # every slot once
    assert all(M.SLOT12[l] == M.SLOT12[l & ~3] for l in range(64))             # identical inside a quad
    b23 = ((lanes >> 2) & 1).astype(bool) & ((lanes >> 3) & 1).astype(bool)
    assert np.array_equal(M.SLOT12[b23], M.SLOT12[lanes[b23] ^ 8])             # the b2 & b3 quads duplicate the b2 & !b3 ones
    committers16 = lanes[(lanes % 4 == 0) & (M.SLOT16 < 12)]
    assert sorted(M.SLOT16[committers16].tolist()) == list(range(12))


@pytest.mark.parametrize("kind", ["random", "cancelling", "onehot"])
def test_twelve_totals_bit_equal_to_the_16_value_form(kind):
    cases = [(n, v) for n, v in M.inputs() if n.startswith(kind)]
    assert len(cases) >= 8
    for name, v in cases:
        got16, got12 = M.butterfly_sum16(M.pad16(v)), M.butterfly_sum12(v)
        M.check(v, got16, got12)
        if kind == "onehot":      # the value arrives in the lanes of its slot and nowhere else: a wrong pairing shows
            lane, k = [int(x[1:]) for x in name.split("_")[1:]]
            assert np.array_equal(got12 != 0, M.SLOT12 == k) and np.all(got12[M.SLOT12 == k] == v[lane, k]), name
            assert np.array_equal(got16 != 0, M.SLOT16 == k), name


def test_the_cancelling_inputs_do_depend_on_the_order():
    """(so that bit-equality on them says something: summed lane by lane the same columns give another float32 total)"""
    differs = 0
    for name, v in M.inputs():
        if name.startswith("cancelling"):
            tree = M.butterfly_sum12(v)[M.COMMIT12][np.argsort(M.SLOT12[M.COMMIT12])]
            serial = np.zeros(12, np.float32)
            for lane in range(64):
                serial = (serial + v[lane]).astype(np.float32)
            differs += int(np.any(tree != serial))
    assert differs > 0
