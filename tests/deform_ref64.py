"""Float64 restatement of the deformation networks, written from the contract (models/modules.py:874-1012): encoding
[v, sin(2^k v), cos(2^k v)] for k < 10, h0 = [emb(x) | emb(t) | cond], 8 x (Linear + ReLU) with the skip [h0 | h4] into layer 5,
heads warp / rotation / scaling.  Shared by tests/test_deform_network_cpu.py and tests/test_gpu_35_deform_network.py."""
import zlib

import numpy as np
import torch

HEADS = ("gaussian_warp", "gaussian_rotation", "gaussian_scaling")
EXP_W, EXP_B = 18, 20      # weights: int16 code x 2^-18 (|w| < 2^-3), biases: x 2^-20 (|b| < 2^-5); exact in float32


def hashed_codes(name, shape, seed):
    """int16 codes of one parameter from a fixed integer hash (splitmix64) of (seed, name, flat index): the same on every machine
    and torch / numpy version, so the golden files need not carry the 0.5 M weights."""
    n = int(np.prod(shape))
    salt = np.full(1, zlib.crc32(name.encode()) + (int(seed) << 32), dtype=np.uint64)
    z = np.arange(n, dtype=np.uint64) + salt * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(48)).astype(np.int64) - 32768).astype(np.int16).reshape(shape)


def hashed_state_dict(shapes, seed, dtype=torch.float32):
    """{name: shape} -> the state_dict of hashed codes x 2^-k."""
    return {k: torch.from_numpy(hashed_codes(k, sh, seed).astype(np.float64) * 2.0 ** -(EXP_W if k.endswith("weight") else EXP_B)).to(dtype)
            for k, sh in shapes.items()}


def golden_state_dict(z, dtype=torch.float32):
    """The state_dict a fixture was generated with (its keys, shapes and hash seed)."""
    return hashed_state_dict({str(k): tuple(int(d) for d in z["shape_" + str(k)]) for k in z["sd_keys"]}, int(z["seed"]), dtype)


def stored_grad(z, g, key):
    """(golden, ours) for a stored gradient: grad_<name> is the whole tensor, gradcols_<name> the columns cols_<name> of it."""
    if key.startswith("gradcols_"):
        name = key[len("gradcols_"):]
        return z[key], g[name][:, torch.as_tensor(z["cols_" + name]).to(g[name].device)]
    return z[key], g[key[len("grad_"):]]


def enc64(v, L=10):
    out = [v]
    for k in range(L):
        out += [torch.sin(v * 2.0 ** k), torch.cos(v * 2.0 ** k)]
    return torch.cat(out, -1)


def forward64(sd, x, t, cond=None):
    """(d_xyz, rotation or None, scaling or None) from a state_dict of float64 tensors (missing head = off)."""
    h0 = torch.cat([enc64(x), enc64(t)] + ([cond] if cond is not None else []), -1)
    h = h0
    for i in range(8):
        h = torch.relu(h @ sd[f"linear.{i}.weight"].T + sd[f"linear.{i}.bias"])
        if i == 4:
            h = torch.cat([h0, h], -1)
    return tuple((h @ sd[n + ".weight"].T + sd[n + ".bias"]) if n + ".weight" in sd else None for n in HEADS)



def grads64(sd, x, t, cond, ws):
    """Outputs and the gradients of sum(w * out) (ws: one weight tensor per head, None = head off) w.r.t. every parameter and
    x / t / cond, all float64.  Returns (outs, {name: grad})."""
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    ins = {"x": x.detach().double().clone().requires_grad_(True), "t": t.detach().double().clone().requires_grad_(True)}
    if cond is not None:
        ins["cond"] = cond.detach().double().clone().requires_grad_(True)
    outs = forward64(sd, ins["x"], ins["t"], ins.get("cond"))
    loss = sum((o * w.double()).sum() for o, w in zip(outs, ws) if o is not None)
    loss.backward()
    g = {k: v.grad for k, v in sd.items()}
    g.update({k: v.grad for k, v in ins.items()})
    return tuple(None if o is None else o.detach() for o in outs), g


def rel(a, b):
    """Norm-wise relative error of a against b."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
