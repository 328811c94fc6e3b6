#!/usr/bin/env python3
"""Golden vectors for the SMPL nodes' pose chain and skinning (bilateral_driving_amd/smpl.py, csrc/smpl.hip), produced by the
REFERENCE's own SMPLNodes.transform_means_and_quats / transform_means (models/nodes/smpl.py:203-341), SMPLTemplate.forward
(models/human_body.py:158-180) and VoxelDeformer.forward / normalize (models/modules.py:1168-1188), called unbound on bare objects that
hold only the attributes those methods read.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_smpl_skin.py        (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

models/human_body.py, models/nodes/rigid.py and models/nodes/smpl.py are loaded by path with an empty stub in place of trimesh;
matrix_to_quaternion / quaternion_to_matrix are bound to bilateral_driving_amd.p3d's (the import stubs leave them None).  No SMPL model
file is needed: J_canonical, A0_inv, the field and the standard 24-entry parent table are synthetic arrays stored in the fixture
(tests/smpl_skin_ref64.make_inputs).  The reference fixes V = 6890 and float32 on the quaternion path (the literal tensor of :339).

smpl_skin.npz: I = 2 humans, V = 6890, a (4,8,8) field, F = 5 frames.  Frame 1: training, both present; frame 2: training, instance 1
absent; frame 3: in_test_set, interpolated (instance 0 between frames 2 and 4, instance 1 keeps frame 3: frame 2 does not see it),
forward only.  Stored: the inputs, the full pose / translation / field gradients and every 8th row of the per-point outputs and
gradients of loss = sum(wm * w_m) + sum(wq * w_q)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "smpl_skin.npz")
I, V, DHW, F = 2, 6890, (4, 8, 8), 5
TRAIN, INTERP, STRIDE = (1, 2), 3, 8
MIN_GAP = 1e-6


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    from bilateral_driving_amd import p3d
    from tests import smpl_skin_ref64 as R64
    sys.modules["trimesh"] = types.ModuleType("trimesh")
    sys.modules["pytorch3d.transforms"].axis_angle_to_matrix = p3d.axis_angle_to_matrix
    import models
    import models.modules as MM
    base = os.path.dirname(models.__file__)
    HB = load("models.human_body", os.path.join(base, "human_body.py"))
    load("models.nodes.rigid", os.path.join(base, "nodes", "rigid.py"))
    SM = load("ref_smpl", os.path.join(base, "nodes", "smpl.py"))
    for m in (HB, SM):
        m.matrix_to_quaternion, m.quaternion_to_matrix = p3d.matrix_to_quaternion, p3d.quaternion_to_matrix

    class Deformer:
        """The attributes VoxelDeformer.forward / normalize / get_voxel_weight read."""
        get_voxel_weight = property(lambda s: MM.VoxelDeformer.get_voxel_weight.fget(s))
        normalize = MM.VoxelDeformer.normalize
        __call__ = MM.VoxelDeformer.forward

    class Template:
        """The attributes SMPLTemplate.forward reads."""
        __call__ = HB.SMPLTemplate.forward

    class Bare:
        """The attributes SMPLNodes' transform methods read."""
        smpl_points_num, use_voxel_deformer, device = V, True, torch.device("cpu")
        num_instances = property(lambda s: s.instances_fv.shape[1])
        num_frames = property(lambda s: s.instances_fv.shape[0])

        def quat_act(self, x):
            return x / x.norm(dim=-1, keepdim=True)

    d = R64.make_inputs(I, V, DHW, seed=20, F=F, frames=TRAIN + (INTERP,), compact=True)
    d["instances_fv"][2, 1] = False
    # the input conditions
    for f in TRAIN + (INTERP,):
        gap, real = R64.blend_margins(d, f, interpolate=f == INTERP)
        assert float(gap.min()) >= MIN_GAP and float(real.min()) >= MIN_GAP, (f, float(gap.min()), float(real.min()))
    n = R64.normalize_coords(d["means"].reshape(I, V, 3).double(), d["offset"].double(), d["scale"].double(), d["ratio"], d["ratio_dim"])
    assert float((n.abs() > 1).any(-1).float().mean()) >= 0.01 and int((n == 1).any(-1).sum()) >= 4

    def run(f, test, grad, ball=False):
        ts = {k: d[k].clone().requires_grad_(grad) for k in R64.INPUTS}
        vd = Deformer()
        vd.lbs_voxel_base, vd.voxel_w_correction, vd.offset, vd.scale = d["voxel_base"], ts["voxel_corr"], d["offset"], d["scale"]
        vd.ratio, vd.ratio_dim = torch.tensor(d["ratio"]), d["ratio_dim"]
        tp = Template()
        tp.J_canonical, tp.A0_inv, tp.use_voxel_deformer, tp.voxel_deformer = d["J_canonical"], d["A0_inv"], True, vd
        tp._template_layer = types.SimpleNamespace(parents=torch.tensor(d["parents"], dtype=torch.long))
        b = Bare()
        b.template, b.instances_fv, b.cur_frame, b.in_test_set = tp, d["instances_fv"], f, test
        b.point_ids = torch.arange(I).repeat_interleave(V)[:, None]
        b.instances_quats, b.smpl_qauts, b.instances_trans = ts["instances_quats"], ts["smpl_quats"], ts["instances_trans"]
        if ball:
            return {"wm_ball": SM.SMPLNodes.transform_means(b, ts["means"]).detach().numpy()[::STRIDE]}
        wm, wq = SM.SMPLNodes.transform_means_and_quats(b, ts["means"], ts["quats"])
        out = {"wm": wm.detach().numpy()[::STRIDE], "wq": wq.detach().numpy()[::STRIDE]}
        if grad:
            ((wm * d["w_m"]).sum() + (wq * d["w_q"]).sum()).backward()
            for k, t in ts.items():
                g = t.grad.numpy()
                out["grad_" + k] = g[::STRIDE] if k in ("means", "quats") else g
        return out

    rec = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in d.items() if v is not None}
    rec.update(train_frames=np.array(TRAIN), interp_frame=np.array(INTERP), stride=np.array(STRIDE))
    for k, t in (("quats", np.float16), ("voxel_base", np.float16), ("voxel_corr", np.float16), ("w_m", np.int8), ("w_q", np.int8)):
        assert (rec[k].astype(t).astype(np.float32) == rec[k]).all(), k         # (compact inputs: stored exactly in the narrow type)
        rec[k] = rec[k].astype(t)
    for f in TRAIN:
        for k, v in run(f, False, True).items():
            rec[f"f{f}_{k}"] = v
    with torch.no_grad():
        for k, v in run(INTERP, True, False).items():
            rec[f"f{INTERP}_{k}"] = v
        for k, v in run(TRAIN[0], False, False, ball=True).items():
            rec[f"f{TRAIN[0]}_{k}"] = v
    np.savez_compressed(OUT, **rec)
    cap = os.path.getsize(os.path.join(ROOT, "tests", "golden", "node_pose_train.npz"))
    assert os.path.getsize(OUT) <= cap, (os.path.getsize(OUT), cap)
    print(f"wrote smpl_skin.npz ({os.path.getsize(OUT)} bytes, cap {cap})")


if __name__ == "__main__":
    main()
