"""-m gpu: the four expected-depth glue entries (bds_expected_depth_fwd / _bwd and their split forms, csrc/rasterize.hip: one kernel
template each way over the output layout) called directly -- sizes around the 256-thread block edge, alphas on both sides of the
clamp's constant, every optional gradient absent in turn.  The packed and the split form agree bit for bit in every channel they
share, and both meet the bounds of the host cases (tests/pixel_formulas_ref64.py) against the float64 restatement, the quotients'
widened to 3 * 2^-23 |ref|: the build does not pin a correctly rounded division, and the device's own is within 2.5 ulp."""
import numpy as np
import pytest
import torch

from tests import pixel_formulas_ref64 as PF

pytestmark = pytest.mark.gpu
QUOTIENT = 3 * 2.0 ** -23


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    from bilateral_driving_amd import _lib
    return _lib


def _poisoned(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("P", [1, 255, 256, 257])
@pytest.mark.parametrize("channels,ed", [(3, 0), (4, 0), (4, 1)])
def test_packed_and_split_glue_agree_and_match_float64(L, P, channels, ed):
    lib, st = L.lib(), L.stream()
    z = PF.cases(P, seed=P)
    if P >= len(PF.ALPHAS):
        assert set(z["alpha"].tolist()) == set(PF.ALPHAS.tolist())
    cu = lambda a: torch.from_numpy(a).cuda()
    alphas, D, v_rgb, v_depth, va_in = cu(z["alpha"]), cu(z["D"]), cu(z["v"]), cu(z["vd"]), cu(z["va_in"])
    render = torch.cat([cu(z["sky"]), D[:, None]], -1).contiguous()          # (any colour: it passes through)

    # ---- forward: the packed entry always normalises, the split one on request ----
    rgb3, depth1 = _poisoned(P, 3), _poisoned(P)
    L.check(lib.bds_expected_depth_split_fwd(P, ed, L.ptr(render), L.ptr(alphas), L.ptr(rgb3), L.ptr(depth1), st), "split_fwd")
    assert torch.equal(rgb3, render[:, :3])
    if ed:
        out4 = _poisoned(P, 4)
        L.check(lib.bds_expected_depth_fwd(P, L.ptr(render), L.ptr(alphas), L.ptr(out4), st), "fwd")
        assert torch.equal(out4[:, :3], rgb3) and torch.equal(out4[:, 3], depth1)
        PF.check(dict(depth=depth1.cpu().numpy()), PF.reference(z, blend=False), quotient_bound=QUOTIENT)
    else:
        assert torch.equal(depth1, D)

    # ---- backward: all gradients present, then each one absent (NULL = zeros) in turn ----
    for absent in (None, "v_out", "v_rgb3", "v_depth1", "v_alphas_in"):
        has_rgb, has_depth, has_va = absent not in ("v_out", "v_rgb3"), absent not in ("v_out", "v_depth1"), absent != "v_alphas_in"
        if channels == 3 and absent == "v_depth1":
            continue                                                          # (a 3-channel image gradient has no depth to drop)
        if channels == 3:
            v_out = v_rgb if has_rgb else None
        elif absent == "v_out":
            v_out = None
        else:   # the packed form cannot drop one part of v_out: hand it the zeros that the split form's NULL stands for
            v_out = torch.cat([v_rgb if has_rgb else torch.zeros_like(v_rgb), (v_depth if has_depth else torch.zeros_like(v_depth))[:, None]], -1)
        has_depth = has_depth and channels == 4
        vr_p, va_p, vr_s, va_s = _poisoned(P, 4), _poisoned(P), _poisoned(P, 4), _poisoned(P)
        L.check(lib.bds_expected_depth_bwd(P, channels, ed, L.ptr(render), L.ptr(alphas), L.ptr(v_out),
                                           L.ptr(va_in if has_va else None), L.ptr(vr_p), L.ptr(va_p), st), "bwd")
        L.check(lib.bds_expected_depth_split_bwd(P, ed, L.ptr(render), L.ptr(alphas), L.ptr(v_rgb if has_rgb else None),
                                                 L.ptr(v_depth if has_depth else None), L.ptr(va_in if has_va else None), L.ptr(vr_s),
                                                 L.ptr(va_s), st), "split_bwd")
        torch.cuda.synchronize()
        assert torch.equal(vr_p, vr_s) and torch.equal(va_p, va_s), absent
        assert torch.equal(vr_p[:, :3], v_rgb if has_rgb else torch.zeros_like(v_rgb)), absent
        zz = dict(z, vd=z["vd"] if has_depth else np.zeros_like(z["vd"]), va_in=z["va_in"] if has_va else np.zeros_like(z["va_in"]))
        ref = PF.reference(zz, expected_depth=bool(ed), blend=False)
        PF.check(dict(v_D=vr_p[:, 3].cpu().numpy(), v_alpha=va_p.cpu().numpy()), ref, quotient_bound=QUOTIENT, alpha_is_gated=not has_va)
