#!/usr/bin/env python3
"""Golden vectors for the fused image loss (bilateral_driving_amd/losses.py ``image_terms``, csrc/image_loss_math.h), produced by the
REFERENCE's own ``DepthLoss``, ``binary_cross_entropy`` and ``safe_binary_cross_entropy`` (models/losses.py) in float32 on the CPU,
called as ``BasicTrainer.compute_losses`` calls them (models/trainers/base.py:527-565).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_image_loss.py        (needs the reference tree that oracle/gen_golden_losses.py loads; CPU only)

Never imported by a test.  image_loss.npz: one 24 x 40 view with an egocar mask (tests/image_loss_ref64.make, seed 7); the rgb term; the
sky term under both mask kinds; the depth term under all 12 forms (3 loss types x normalize x inverse) with mean_on_hit and one form
each with mean_on_hw and sum.  Every value is weighted by tests/image_loss_ref64.W6 and every gradient is that of V6[k] x the term,
so the records compare directly with ``ref`` run with that one term switched on."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "image_loss.npz")
H, W, SEED = 24, 40, 7


def main():
    sys.path.insert(0, ROOT)
    from oracle import gen_golden_losses as G
    from tests import image_loss_ref64 as R
    ref = G.load_reference_losses()
    d = R.make(H, W, SEED)
    rec = {k: v.numpy() for k, v in d.items() if k != "dyn"}
    valid = (1.0 - d["ego"]).float()
    pixels = d["pixels"]

    def leaf(k):
        return d[k].clone().requires_grad_(True)

    rgb = leaf("rgb")
    term = R.W6[0] * torch.abs(pixels * valid[..., None] - rgb * valid[..., None]).mean()
    (R.V6[0] * term).backward()
    rec["rgb_value"], rec["rgb_grad"] = term.detach().numpy(), rgb.grad.numpy()
    for kind, fn in (("bce", lambda x, y: ref.binary_cross_entropy(x, y, reduction="mean")),
                     ("safe_bce", lambda x, y: ref.safe_binary_cross_entropy(x, y, limit=0.1, reduction="mean"))):
        opacity = leaf("opacity")
        term = fn(opacity.squeeze() * valid, (1.0 - d["sky"]).float() * valid) * R.W6[1]
        (R.V6[1] * term).backward()
        rec[f"mask_{kind}_value"], rec[f"mask_{kind}_grad"] = term.detach().numpy(), opacity.grad.numpy()
    cases = [(t, n, i, "mean_on_hit") for t, n, i in R.DEPTH_FORMS] + [("smooth_l1", True, False, "mean_on_hw"), ("l2", False, True, "sum")]
    for k, (t, n, i, r) in enumerate(cases):
        depth = leaf("depth")
        fn = ref.DepthLoss(loss_type=t, normalize=n, use_inverse_depth=i, reduction=r)
        term = fn(depth, d["lidar"], (d["lidar"] > 0).float() * valid) * R.W6[2]
        (R.V6[2] * term).backward()
        rec[f"depth_{k}_value"], rec[f"depth_{k}_grad"] = term.detach().numpy(), depth.grad.numpy()
    rec["depth_cases"] = np.array([f"{t},{int(n)},{int(i)},{r}" for t, n, i, r in cases])
    np.savez_compressed(OUT, **rec)
    print(f"wrote image_loss.npz ({os.path.getsize(OUT)} bytes), {len(cases)} depth cases")


if __name__ == "__main__":
    main()
