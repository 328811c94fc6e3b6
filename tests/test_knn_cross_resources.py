"""hipcc's resource report of csrc/knn_cross.hip under the product's build flags (cross-compiled: needs no GPU).

No kernel may use scratch: the K-best list is indexed statically in unrolled loops and must stay in registers.  The Kc = 32
instantiation (K = 17..32, the skinning field's K = 30) is held at the 5 waves per SIMD it was tuned at: its list alone is 64 VGPRs,
the search adds the query, the candidate and the compare masks' selects (84), and the blend epilogue reads the features through
buffer loads with ONE register of address per slot -- with 64-bit addresses it stood at 123 VGPRs and 4 waves.  88 allocated
registers is the last step before 96, and 96 the last that gives 5 waves (512 / 96)."""
import re

from bilateral_driving_amd import p3d
from tests.util import kernel_resources

KC32_WAVES = 5
KC32_MAX_VGPRS = 96


def test_knn_cross_kernel_resources():
    res = kernel_resources("knn_cross.hip")
    names = {}
    for mangled, r in res.items():
        m = re.match(r"knn_cross_kernelILi(\d+)ELi(\d)EEE", mangled)
        assert m, mangled
        names[(int(m.group(1)), int(m.group(2)))] = r
    assert sorted(names) == [(kc, norm) for kc in (4, 8, 16, 32) for norm in (1, 2)]
    for (kc, norm), r in sorted(names.items()):
        print(f"\nknn_cross_kernel<{kc}, {norm}>: {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs, occupancy {r['Occupancy']} waves/SIMD, "
              f"LDS {r['LDS Size']} bytes, scratch {r['ScratchSize']}")
        assert r["ScratchSize"] == 0, (kc, norm, r)
        assert r["LDS Size"] == 16 * p3d.TARGET_TILE, (kc, norm, r)
        assert r["Occupancy"] >= (8 if kc <= 16 else KC32_WAVES), (kc, norm, r)
    for norm in (1, 2):
        assert names[(32, norm)]["VGPRs"] <= KC32_MAX_VGPRS and names[(32, norm)]["Occupancy"] == KC32_WAVES
