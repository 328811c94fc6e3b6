"""Resources of the SMPL skinning kernels (csrc/smpl.hip) from hipcc's report under the product's build flags: no kernel of the file
may use scratch -- the parent table is packed into two words and every thread-local array is indexed by unrolled constants, so
nothing is indexed by ``parents[j]`` in registers.

Recorded (gfx950, -O3):
    smpl_skin_fwd_kernel    122 VGPRs,  3456 bytes of LDS (the chain: local, world and skinning matrices of 24 joints)
    smpl_skin_bwd_kernel    150 VGPRs, 38160 bytes of LDS (A, and the 24 weights and 12 blend-gradient floats of 256 points)
    smpl_pose_bwd_kernel     60 VGPRs,  5488 bytes of LDS (the chain, its gradients, the reduced workgroup rows)"""
from tests.util import kernel_resources

KERNELS = ("smpl_skin_fwd_kernel", "smpl_skin_bwd_kernel", "smpl_pose_bwd_kernel")


def test_no_smpl_kernel_uses_scratch():
    res = kernel_resources("smpl.hip")
    assert len(res) == len(KERNELS), list(res)
    for name in KERNELS:
        ks = [k for k in res if k.startswith(name)]
        assert len(ks) == 1, (name, list(res))
        r = res[ks[0]]
        print(f"\n{name}: {r['VGPRs']} VGPRs, {r['LDS Size']} bytes of LDS, occupancy {r['Occupancy']}")
        assert r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] <= 40 * 1024 and r["Occupancy"] >= 2, (name, r)
