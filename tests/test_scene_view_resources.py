"""Resources of the scene view's two kernels (csrc/scene_view.hip) from hipcc's report under the product's build flags: neither may
use scratch -- the segment table is a kernel argument read through scalar registers (the segment loop's index is wave-uniform), the
SH bases are indexed by unrolled constants only, and no per-thread array is indexed by a segment number.

Recorded (gfx950, -O3):
    scene_pack_kernel      86 VGPRs, 64 SGPRs, 0 bytes of LDS, occupancy 5 (four SH degrees behind one wave-uniform switch)
    scene_sh_bwd_kernel    41 VGPRs, 50 SGPRs, 0 bytes of LDS, occupancy 8"""
from tests.util import kernel_resources

KERNELS = ("scene_pack_kernel", "scene_sh_bwd_kernel")


def test_no_scene_view_kernel_uses_scratch():
    res = kernel_resources("scene_view.hip")
    assert len(res) == len(KERNELS), list(res)
    for name in KERNELS:
        ks = [k for k in res if k.startswith(name)]
        assert len(ks) == 1, (name, list(res))
        r = res[ks[0]]
        print(f"\n{name}: {r['VGPRs']} VGPRs, {r['LDS Size']} bytes of LDS, occupancy {r['Occupancy']}")
        assert "ScratchSize" in r and r["ScratchSize"] == 0, (name, r)
