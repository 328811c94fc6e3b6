"""Resources of the SMPL regularisers' kernels (csrc/smpl_reg.hip) from hipcc's report under the product's build flags: no kernel of
the file may use scratch -- the attribute group of a channel is picked by unrolled selects, never by indexing an array with a lane's
value, and the K gathered values are read again in the second pass instead of being kept in an array of K.

Recorded (gfx950, -O3):
    smpl_knn_reg_fwd_kernel      43 VGPRs, 80 bytes of LDS (the waves' five sums)
    smpl_knn_reg_finish_kernel   25 VGPRs, no LDS
    smpl_knn_reg_bwd_kernel      19 VGPRs, no LDS
    voxel_reg_fwd_kernel         26 VGPRs, 64 bytes of LDS (the waves' four sums)
    voxel_reg_finish_kernel      14 VGPRs, 16 bytes of LDS
    voxel_reg_bwd_kernel         20 VGPRs, no LDS"""
from tests.util import kernel_resources

KERNELS = ("smpl_knn_reg_fwd_kernel", "smpl_knn_reg_finish_kernel", "smpl_knn_reg_bwd_kernel", "voxel_reg_fwd_kernel",
           "voxel_reg_finish_kernel", "voxel_reg_bwd_kernel")


def test_no_smpl_reg_kernel_uses_scratch():
    res = kernel_resources("smpl_reg.hip")
    assert len(res) == len(KERNELS), list(res)
    for name in KERNELS:
        ks = [k for k in res if k.startswith(name)]
        assert len(ks) == 1, (name, list(res))
        r = res[ks[0]]
        print(f"\n{name}: {r['VGPRs']} VGPRs, {r['LDS Size']} bytes of LDS, occupancy {r['Occupancy']}")
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 64 and r["LDS Size"] <= 1024 and r["Occupancy"] >= 8, (name, r)
