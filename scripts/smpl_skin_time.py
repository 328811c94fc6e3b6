#!/usr/bin/env python3
"""Time of the fused pose chain and skinning of the SMPL nodes (csrc/smpl.hip through ``smpl.skin_transform``, B) against the same
expression as framework ops (``smpl.framework_transform``, A: quaternion_to_matrix, the 23-step chain, base + correction, the 5-D
grid_sample, the blend einsum, matrix_to_quaternion, quat_mult, the index_add scatters), forward + backward (gradients of means, quats,
the two quaternion tables, the translations and the field correction, as the trainer needs) and forward only.

    python scripts/smpl_skin_time.py [--out profiles/smpl_skin_time.json] [--humans 8] [--field 16,64,64] [--reps 30]
    python scripts/smpl_skin_time.py --profile fused|framework [--steps 5]     (that side only, for rocprofv3 --kernel-trace --stats:
                                                                                its launches per step = kernel calls / steps)

The paper_legacy sizes: I = 8 humans, V = 6890 points each, a [8,24,16,64,64] field, every human present.  Device events around each
call after a warm-up, A and B alternated over the repeats; the median is reported (ms).  Both sides include the loss's own reductions
and the zero fill of the parameter gradients autograd makes."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import smpl  # noqa: E402

V, F, FRAME = 6890, 40, 7
GRADS = ("means", "quats", "instances_quats", "smpl_quats", "instances_trans", "voxel_corr")


def make(I, dhw, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    d, h, w = dhw
    ratio = h / d
    u = (torch.rand(I, V, 3, generator=g) * 2 - 1) * 1.05
    u[..., 2] /= ratio
    offset, scale = n(I, 1, 3) * 0.1, torch.rand(I, 1, 1, generator=g) + 0.8
    t = dict(means=(offset + scale * u).reshape(I * V, 3), quats=n(I * V, 4), instances_quats=n(F, I, 1, 4), smpl_quats=n(F, I, 23, 4),
             instances_trans=n(F, I, 3) * 5, voxel_corr=n(I, 24, d, h, w) * 0.01)
    t = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
    kw = dict(J_canonical=(n(I, 24, 3) * 0.3).cuda(), A0_inv=(torch.eye(4).expand(I, 24, 4, 4) + n(I, 24, 4, 4) * 0.2).cuda(),
              parents=smpl.SMPL_PARENTS, voxel_base=torch.softmax(n(I, 24, d, h, w) * 2, dim=1).cuda(), offset=offset.cuda(),
              scale=scale.cuda(), ratio=ratio, ratio_dim=-1)
    fv = torch.ones(F, I, dtype=torch.bool).cuda()
    ws = (n(I * V, 3).cuda(), n(I * V, 4).cuda())
    return t, kw, fv, ws


def step(t, kw, fv, ws, fused, backward):
    for k in GRADS:
        t[k].grad = None
    fn = smpl.skin_transform if fused else smpl.framework_transform
    with torch.set_grad_enabled(backward):
        wm, wq = fn(t["means"], t["quats"], t["instances_quats"], t["smpl_quats"], t["instances_trans"], fv, FRAME, voxel_corr=t["voxel_corr"], **kw)
        if backward:
            ((wm * ws[0]).sum() + (wq * ws[1]).sum()).backward()
    return wm, wq


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/smpl_skin_time.json")
    ap.add_argument("--humans", type=int, default=8)
    ap.add_argument("--field", default="16,64,64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", choices=("fused", "framework"))
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    L.lib()
    dhw = tuple(int(x) for x in a.field.split(","))
    t, kw, fv, ws = make(a.humans, dhw)
    if a.profile:
        for _ in range(a.steps):
            step(t, kw, fv, ws, a.profile == "fused", True)
        torch.cuda.synchronize()
        return
    # the two sides compute the same thing at the timed size (the field gradient's summation order differs)
    step(t, kw, fv, ws, False, True)
    ref = {k: t[k].grad.clone() for k in GRADS}
    step(t, kw, fv, ws, True, True)
    agree = {k: float((t[k].grad - ref[k]).abs().max() / ref[k].abs().max().clamp(min=1.0)) for k in GRADS}
    rows = []
    for backward in (True, False):
        for _ in range(5):
            step(t, kw, fv, ws, True, backward)
            step(t, kw, fv, ws, False, backward)
        torch.cuda.synchronize()
        tb, ta = [], []
        for _ in range(a.reps):
            tb.append(timed(lambda: step(t, kw, fv, ws, True, backward)))
            ta.append(timed(lambda: step(t, kw, fv, ws, False, backward)))
        mb, ma = statistics.median(tb), statistics.median(ta)
        row = dict(I=a.humans, V=V, field=list(dhw), mode="fwd+bwd" if backward else "fwd", fused_ms=round(mb, 4), framework_ms=round(ma, 4),
                   speedup=round(ma / mb, 2), fused_min_ms=round(min(tb), 4), framework_min_ms=round(min(ta), 4),
                   fused_max_ms=round(max(tb), 4), framework_max_ms=round(max(ta), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0), frames=F, reps=a.reps, rows=rows, gradient_agreement=agree,
               note="median of device-event times around one call (ms), A and B alternated; the backward includes the loss's own "
                    "reductions on both sides; gradient_agreement: largest difference over max(1, largest entry) per tensor")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
