#!/usr/bin/env python3
"""Golden vectors for the deformation network of deformable Gaussians by IMPORTING THE REFERENCE: models/modules.py
ConditionalDeformNetwork (:967-1012; embed_dim 16, deform_quat on, deform_scale off: DeformableNodes in every OmniRe config) and
DeformNetwork (:925-964; configs/deformablegs.yaml), both at D 8, W 256, multires 10 / 10.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_deform_network.py        (build machine only: needs the reference tree)

Weights are int16 codes x 2^-k (exact in float32) drawn by a fixed integer hash of (seed, parameter name, index)
(tests/deform_ref64.py hashed_codes), so a file carries only the state_dict's keys, shapes and seed, not the weights.  Each file: those,
the inputs x / t / cond (|x| up to 4, some points outside [-1, 1]), the outputs, the loss weights and the autograd gradients of
loss = sum(w_xyz * d_xyz) + sum(w_rot * rotation) + sum(w_scale * scaling) w.r.t. cond, x, t, every bias, the heads and linear.0, and
of linear.5 its encoding columns plus every 8th hidden column (gradcols_ / cols_).  The six 256 x 256 weight gradients and the rest of
linear.5 are pinned by the float64 restatement (tests/test_deform_network_cpu.py), which must match every stored value."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.gen_golden_neural_modules import import_reference  # noqa: E402  (the stubbing of tensorly / pytorch3d / nvdiffrast)
from tests.deform_ref64 import hashed_state_dict  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def run(name, mod, N, cond_dim, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict(hashed_state_dict(shapes, seed), strict=True)
    rec = {"sd_keys": np.array(list(shapes)), "seed": np.array(seed)}
    for k, sh in shapes.items():
        rec["shape_" + k] = np.array(sh, dtype=np.int64)
    x = torch.randn(N, 3, generator=g) * 0.8
    x[: N // 10] *= 4.0
    x = x.clamp(-4.0, 4.0).requires_grad_(True)
    t = torch.rand(N, 1, generator=g).requires_grad_(True)
    args = [x, t]
    if cond_dim:
        cond = (torch.randn(N, cond_dim, generator=g) * 0.5).requires_grad_(True)
        args.append(cond)
    outs = mod(*args)
    loss = 0.0
    for nm, o in zip(("xyz", "rot", "scale"), outs):
        if o is None:
            continue
        w = torch.randn(o.shape, generator=g)
        rec["w_" + nm], rec["out_" + nm] = w.numpy(), o.detach().numpy()
        loss = loss + (o * w).sum()
    loss.backward()
    rec["x"], rec["t"], rec["grad_x"], rec["grad_t"] = x.detach().numpy(), t.detach().numpy(), x.grad.numpy(), t.grad.numpy()
    if cond_dim:
        rec["cond"], rec["grad_cond"] = cond.detach().numpy(), cond.grad.numpy()
    K0 = mod.linear[0].in_features
    cols = np.concatenate([np.arange(K0), K0 + np.arange(0, 256, 8)])
    for k, p in mod.named_parameters():
        if k.endswith("bias") or not k.startswith("linear.") or k == "linear.0.weight":
            rec["grad_" + k] = p.grad.numpy()
    rec["gradcols_linear.5.weight"], rec["cols_linear.5.weight"] = mod.linear[5].weight.grad.numpy()[:, cols], cols
    np.savez_compressed(os.path.join(OUT, f"deform_network_{name}.npz"), **rec)
    print(name, N, [None if o is None else tuple(o.shape) for o in outs], float(loss))


def main():
    torch.set_num_threads(8)
    M = import_reference()
    run("cond", M.ConditionalDeformNetwork(D=8, W=256, input_ch=3, embed_dim=16, x_multires=10, t_multires=10, deform_quat=True,
                                           deform_scale=False), 300, 16, 1)
    run("plain", M.DeformNetwork(D=8, W=256, input_ch=3, x_multires=10, t_multires=10), 300, 0, 2)


if __name__ == "__main__":
    main()
