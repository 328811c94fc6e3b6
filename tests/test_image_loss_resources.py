"""hipcc's resource report of the image-loss kernels of csrc/loss.hip under the product's build flags (cross-compiled: needs no GPU).

The kernels stream: no scratch, and no LDS beyond the reduction (the forward's 4 waves x 9 sums = 144 bytes, the finish's 9 totals =
36 bytes, the backward none).  As built: forward 40 VGPRs / 94 SGPRs, finish 15 / 35, backward 28 / 58, each at the full 8 waves per
SIMD; held at 8 waves and under 64 VGPRs (the last count that gives 8 waves of 512 / 64)."""
from tests.util import kernel_resources

LDS = {"image_loss_fwd_kernel": 4 * 9 * 4, "image_loss_finish_kernel": 9 * 4, "image_loss_bwd_kernel": 0}


def test_image_loss_kernel_resources():
    res = {k.split("kernel")[0][:-1] + "_kernel": r for k, r in kernel_resources("loss.hip").items() if k.startswith("image_loss_")}
    assert sorted(res) == sorted(LDS)
    for name, r in sorted(res.items()):
        print(f"\n{name}: {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs, occupancy {r['Occupancy']} waves/SIMD, LDS {r['LDS Size']} bytes, "
              f"scratch {r['ScratchSize']}")
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] == LDS[name], (name, r)
        assert r["Occupancy"] == 8 and r["VGPRs"] <= 64, (name, r)
