"""Float64 restatement of the node classes' pose transform (models/nodes/rigid.py:28-32, 385-471; test infrastructure): the expression
of ``bilateral_driving_amd.nodes.framework_transform`` evaluated in float64 with autograd, shared by tests/test_node_pose_cpu.py and
tests/test_gpu_36_node_pose.py."""
import numpy as np
import torch

from bilateral_driving_amd.nodes import framework_transform

INPUTS = ("means", "quats", "logits", "instances_quats", "instances_trans")


def rel(a, b) -> float:
    """Norm-wise relative error of b against a."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-30))


def tensors(z, dtype=torch.float64, device="cpu"):
    """The npz (or dict of arrays) inputs as tensors: float ones in `dtype`, ids int64 [N,1], fv bool."""
    t = {k: torch.as_tensor(np.asarray(z[k])).to(device=device, dtype=dtype) for k in INPUTS + ("w_m", "w_q", "w_o")}
    t["point_ids"] = torch.as_tensor(np.asarray(z["point_ids"])).to(device=device, dtype=torch.int64)
    t["instances_fv"] = torch.as_tensor(np.asarray(z["instances_fv"])).to(device=device, dtype=torch.bool)
    return t


def forward64(t, f, interpolate=False):
    return framework_transform(t["means"], t["quats"], t["logits"], t["point_ids"], t["instances_quats"], t["instances_trans"],
                               t["instances_fv"], f, interpolate)


def grads64(t, f):
    """Outputs and gradients {name: array} of loss = sum(wm w_m) + sum(wq w_q) + sum(op w_o) in float64."""
    ts = {k: t[k].detach().double().cpu().clone().requires_grad_(True) for k in INPUTS}
    d = dict(t, **ts)
    d["point_ids"], d["instances_fv"] = t["point_ids"].cpu(), t["instances_fv"].cpu()
    wm, wq, op = forward64(d, f)
    w = {k: t[k].detach().double().cpu() for k in ("w_m", "w_q", "w_o")}
    ((wm * w["w_m"]).sum() + (wq * w["w_q"]).sum() + (op * w["w_o"]).sum()).backward()
    return (wm.detach().numpy(), wq.detach().numpy(), op.detach().numpy()), {k: v.grad.numpy() for k, v in ts.items()}
