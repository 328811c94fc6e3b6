"""float64 restatement (torch autograd over the float32 inputs) of the pixel formulas in front of and behind the colour transform --
expected depth ``D / clamp(alpha, min=1e-10)`` and the blend ``clamp(rgb, max=1) + sky * (1 - alpha)`` (csrc/bilagrid_math.h
expected_depth, expected_depth_backward, sky_clamp_backward) -- with the edge-case inputs and the error bounds that both the host
shim (tests/test_hostmath_vs_oracle.py) and the expected-depth glue kernels (tests/test_gpu_51_expected_depth_glue.py) are held to."""
import numpy as np
import torch

U = 2.0 ** -24                      # unit round-off of float32
FLOOR = np.float32(1e-10)           # the clamp's constant as the kernels have it
ALPHAS = np.array([0.0, 5e-11, FLOOR, np.nextafter(FLOOR, np.float32(0)), np.nextafter(FLOOR, np.float32(1)), 0.5, 1.0], np.float32)
COLOURS = np.array([0.999999, 1.0, 1.0000001, 1.3], np.float32)    # around torch.clamp(max=1)'s gate: 1 - 1 ulp .. 1 + 1 ulp


def cases(P, seed=0):
    """P pixels: every alpha of ALPHAS in turn and, against it, every colour of COLOURS in each channel; D, vd, v, sky, va_in uniform in
    [-4, 4] (D * vd / 1e-20 stays finite in float32).  float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-4.0, 4.0, s).astype(np.float32)
    i = np.arange(P)
    colour = np.stack([COLOURS[(i // len(ALPHAS) + c) % len(COLOURS)] for c in range(3)], -1)
    return dict(alpha=ALPHAS[i % len(ALPHAS)].copy(), colour=colour, D=u(P), vd=u(P), v=u(P, 3), sky=u(P, 3), va_in=u(P))


def reference(z, expected_depth=True, blend=True):
    """float64 values and gradients for the loss  sum(depth * vd) + sum(blend * v) + sum(alpha * va_in): depth, v_D, v_colour, v_sky,
    v_alpha, and ``alpha_terms`` = |va_in| + sum_c |v_c sky_c| + |D vd / ac^2|, the magnitudes that the alpha gradient adds up."""
    t = {k: torch.from_numpy(np.asarray(x)).double() for k, x in z.items()}
    D, alpha, colour, sky = (t[k].clone().requires_grad_(True) for k in ("D", "alpha", "colour", "sky"))
    ac = alpha.clamp(min=float(FLOOR))
    depth = D / ac if expected_depth else D
    loss = (depth * t["vd"]).sum() + (alpha * t["va_in"]).sum()
    terms = t["va_in"].abs()
    if expected_depth:
        terms = terms + (t["D"] * t["vd"] / ac.detach() ** 2).abs() * (t["alpha"] >= float(FLOOR))
    if blend:
        loss = loss + ((colour.clamp(max=1.0) + sky * (1.0 - alpha[:, None])) * t["v"]).sum()
        terms = terms + (t["v"] * t["sky"]).abs().sum(-1)
    loss.backward()
    zeros3 = torch.zeros_like(t["v"])
    return dict(depth=depth.detach().numpy(), v_D=D.grad.numpy(), v_alpha=alpha.grad.numpy(), alpha_terms=terms.numpy(),
                v_colour=(colour.grad if blend else zeros3).numpy(), v_sky=(sky.grad if blend else zeros3).numpy())


def check(got, ref, quotient_bound=2 * U, alpha_is_gated=False):
    """The bounds, from the operation counts: `quotient_bound` |ref| for the two quotients (one division each), 4u |ref| for v_sky (a
    subtraction and a product), 8u sum|term| for the alpha gradient (at most five terms of at most three roundings each, plus four
    additions); the gated outputs (the colour gradient behind clamp(max=1); with `alpha_is_gated` -- only the depth feeds it -- the
    alpha gradient) have the reference's zero / non-zero pattern exactly, and a colour gradient that passes is the incoming one."""
    for k in ("depth", "v_D"):
        if k in got:
            err = np.abs(got[k].astype(np.float64) - ref[k])
            assert np.all(err <= quotient_bound * np.abs(ref[k])), (k, float((err / np.maximum(np.abs(ref[k]), 1e-300)).max()))
    if "v_sky" in got:
        assert np.all(np.abs(got["v_sky"].astype(np.float64) - ref["v_sky"]) <= 4 * U * np.abs(ref["v_sky"])), "v_sky"
    if "v_colour" in got:
        assert np.array_equal(got["v_colour"].astype(np.float64), ref["v_colour"]), "v_colour"
    if "v_alpha" in got:
        err = np.abs(got["v_alpha"].astype(np.float64) - ref["v_alpha"])
        assert np.all(err <= 8 * U * ref["alpha_terms"]), ("v_alpha", float((err / np.maximum(ref["alpha_terms"], 1e-300)).max() / U))
        if alpha_is_gated:
            assert np.array_equal(got["v_alpha"] != 0, ref["v_alpha"] != 0), "v_alpha zero pattern"
