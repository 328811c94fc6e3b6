#!/usr/bin/env python3
"""Golden vectors for the node classes' pose transform (bilateral_driving_amd/nodes.py, csrc/nodes.hip), produced by the
REFERENCE's own RigidNodes.transform_means / transform_quats / get_pts_valid_mask (models/nodes/rigid.py:28-32, 385-441) and
interpolate_quats (models/gaussians/basics.py:17-45), called on a bare object that holds only the attributes they read, then the
activations of get_gaussians (:467-471).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_node_pose.py        (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

rigid.py is loaded by path (models/nodes/__init__.py would pull trimesh in through the SMPL nodes); the remaining imports are
stubbed the way oracle/gen_golden_refine.py does it, with the drop-in gsplat on sys.path for quat_to_rotmat.

node_pose_train.npz: inputs (ids in shuffled order, instances 3 and 11 without points, fv = False rows) and, for cur_frame in
{0, 1, F-2, F-1}, the outputs and the autograd gradients of loss = sum(wm * w_m) + sum(wq * w_q) + sum(op * w_o).
node_pose_interp.npz: the same inputs with in_test_set = True (instance 0: a dot < 0 pair between frames f-1 and f+1, instance 1:
a near-identical pair, the lerp branch): the outputs for the same four frames (interpolation only where 1 < f < F-1)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
N, I, F = 2500, 16, 12
FRAMES = (0, 1, F - 2, F - 1)


class Bare:
    """The attributes RigidNodes' transform methods read."""

    def __init__(self, point_ids, iq, it, fv, cur_frame, in_test_set):
        self.point_ids, self.instances_quats, self.instances_trans, self.instances_fv = point_ids, iq, it, fv
        self.cur_frame, self.in_test_set = cur_frame, in_test_set

    @property
    def num_frames(self):
        return self.instances_fv.shape[0]

    def quat_act(self, x):
        return x / x.norm(dim=-1, keepdim=True)


def make_inputs():
    g = torch.Generator().manual_seed(1234)
    inst = torch.tensor([i for i in range(I) if i not in (3, 11)])
    ids = inst[torch.randint(0, len(inst), (N,), generator=g)]
    ids = torch.sort(ids).values[torch.randperm(N, generator=g)]          # shuffled order, as after densification and culling
    means = (torch.rand(N, 3, generator=g) - 0.5) * 6
    quats = torch.randn(N, 4, generator=g)
    logits = torch.randn(N, 1, generator=g) * 2
    iq = torch.randn(F, I, 4, generator=g)
    it = torch.randn(F, I, 3, generator=g) * 10
    fv = torch.rand(F, I, generator=g) > 0.25
    base = torch.tensor([0.8, 0.2, -0.4, 0.3])
    for k in range(F):
        ang = 0.15 * k
        qk = torch.tensor([np.cos(ang), 0.0, 0.0, np.sin(ang)], dtype=torch.float32)
        w1, x1, y1, z1 = base
        w2, x2, y2, z2 = qk
        prod = torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
        iq[k, 0] = prod * (1.3 if k % 4 < 2 else -1.3)                    # frames two apart have opposite signs: dot < 0
        iq[k, 1] = base * 2.0 + 1e-3 * torch.randn(4, generator=g)        # near-identical rows: dot > 0.9995
    fv[:, 0] = True
    fv[:, 1] = True
    w_m, w_q, w_o = torch.randn(N, 3, generator=g), torch.randn(N, 4, generator=g), torch.randn(N, 1, generator=g)
    return dict(point_ids=ids[:, None].clone(), means=means, quats=quats, logits=logits, instances_quats=iq, instances_trans=it,
                instances_fv=fv, w_m=w_m, w_q=w_q, w_o=w_o)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    import models   # the reference package that import_reference put on sys.path
    spec = importlib.util.spec_from_file_location("ref_rigid", os.path.join(os.path.dirname(models.__file__), "nodes", "rigid.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    RN = R.RigidNodes
    inp = make_inputs()

    def run(f, test, grad):
        ts = {k: inp[k].clone().requires_grad_(grad) for k in ("means", "quats", "logits", "instances_quats", "instances_trans")}
        b = Bare(inp["point_ids"], ts["instances_quats"], ts["instances_trans"], inp["instances_fv"], f, test)
        wm = RN.transform_means(b, ts["means"])
        wq = b.quat_act(RN.transform_quats(b, ts["quats"]))
        op = torch.sigmoid(ts["logits"]) * RN.get_pts_valid_mask(b).float().unsqueeze(-1)
        out = {"wm": wm.detach().numpy(), "wq": wq.detach().numpy(), "op": op.detach().numpy()}
        if grad:
            ((wm * inp["w_m"]).sum() + (wq * inp["w_q"]).sum() + (op * inp["w_o"]).sum()).backward()
            for k, t in ts.items():
                out["grad_" + k] = t.grad.numpy()
        return out

    base = {k: v.numpy() for k, v in inp.items()}
    train, interp = dict(base, frames=np.array(FRAMES)), dict(base, frames=np.array(FRAMES))
    for f in FRAMES:
        for k, v in run(f, False, True).items():
            train[f"f{f}_{k}"] = v
        with torch.no_grad():
            for k, v in run(f, True, False).items():
                interp[f"f{f}_{k}"] = v
    # the interpolation's two branches are both exercised at the interpolated frames
    q1, q2 = inp["instances_quats"][1], inp["instances_quats"][3]
    assert float((q1[0] / q1[0].norm() * q2[0] / q2[0].norm()).sum()) < 0
    assert float((q1[1] / q1[1].norm() * q2[1] / q2[1].norm()).sum()) > 0.9995
    np.savez_compressed(os.path.join(OUT, "node_pose_train.npz"), **train)
    np.savez_compressed(os.path.join(OUT, "node_pose_interp.npz"), **interp)
    print("wrote node_pose_train.npz, node_pose_interp.npz")


if __name__ == "__main__":
    main()
