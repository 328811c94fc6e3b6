#!/usr/bin/env python3
"""Golden vectors for the periodic-vibration Gaussians' time transform (bilateral_driving_amd/pvg.py, csrc/pvg.hip), produced by the
REFERENCE's own PeriodicVibrationGaussians properties get_marginal_t / temporal_means / temporal_opacities / get_scaling / get_quats
(models/gaussians/pvg.py:58-88, vanilla.py:122-146), read from a bare object that holds only the attributes they use, with the
filter of get_gaussians (:389, :410-416).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_pvg.py        (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

pvg_time.npz: the raw parameters, and for three settings s0..s2 of (frame, in_smooth, delta_t) on the shipped schedule (T = 0.2,
time_interval = 0.02, 40 timestamps: train_time_scale = 0.78) -- s0 frame 5 not smoothed, s1 frame 20 smoothed with delta_t < 0,
s2 frame 33 smoothed with delta_t > 0 -- the mask, the filtered outputs and the autograd gradients of
loss = sum(means * w_m) + sum(opacities * w_o) + sum(scales * w_s) + sum(quats * w_q) over the kept rows.
A row whose marginal lies within 1e-4 (relative, float64) of the 0.05 threshold at any setting gets a new tau: no row's keep decision
depends on the last bits of exp, so no row is excluded from any comparison.  SH colours are not part of the golden (the drop-in SH
has no CPU path); they are checked against oracle/gs_oracle.py."""
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
N, T, TIME_INTERVAL, NUM_T = 2000, 0.2, 0.02, 40
SCALE = TIME_INTERVAL / (1.0 / (NUM_T - 1))                 # train_time_scale (pvg.py:46-47)
SETTINGS = ((5, False, 0.0), (20, True, 0.017), (33, True, -0.023))     # frame, in_smooth, cur_time - scaled_train_t (|.| < bound = 0.03)
RAW = ("means", "velocity", "taus", "betas", "logits", "log_scales", "quats")
ATTR = dict(means="_means", velocity="_velocity", taus="_taus", betas="_betas", logits="_opacities", log_scales="_scales", quats="_quats")
BAND = 1e-4


def times(frame, smooth, offset):
    scaled = frame / (NUM_T - 1) * SCALE
    cur = scaled + offset if smooth else scaled
    return cur, (scaled - cur if smooth else 0.0)


def marg64(taus, betas, cur):
    return torch.exp(-0.5 * (taus.double() - cur) ** 2 / torch.exp(betas.double()) ** 2)


def make_inputs():
    g = torch.Generator().manual_seed(4321)
    r = lambda *s: torch.rand(*s, generator=g)
    p = dict(means=(r(N, 3) - 0.5) * 40, velocity=torch.randn(N, 3, generator=g) * 2, taus=r(N, 1) * SCALE,
             betas=torch.log(0.03 * (0.4 / 0.03) ** r(N, 1)), logits=torch.randn(N, 1, generator=g) * 2, log_scales=r(N, 3) * 4 - 4,
             quats=torch.randn(N, 4, generator=g))
    for _ in range(100):
        near = torch.zeros(N, dtype=torch.bool)
        for s in SETTINGS:
            near |= ((marg64(p["taus"], p["betas"], times(*s)[0]) / 0.05 - 1).abs() < BAND).reshape(-1)
        if not near.any():
            break
        p["taus"][near] = r(int(near.sum()), 1) * SCALE
    assert not near.any()
    w = dict(w_m=torch.randn(N, 3, generator=g), w_o=torch.randn(N, 1, generator=g), w_s=torch.randn(N, 3, generator=g),
             w_q=torch.randn(N, 4, generator=g))
    return p, w


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    from models.gaussians.pvg import PeriodicVibrationGaussians as PVG
    p, w = make_inputs()
    out = {k: v.numpy() for k, v in {**p, **w}.items()}
    out.update(T=np.float64(T), frames=np.array([s[0] for s in SETTINGS]))
    for i, s in enumerate(SETTINGS):
        cur, delta = times(*s)
        obj = PVG.__new__(PVG)
        nn.Module.__init__(obj)
        ts = {k: p[k].clone().requires_grad_(True) for k in RAW}
        for k, a in ATTR.items():
            setattr(obj, a, ts[k])
        obj.T, obj.cur_time, obj.delta_t, obj.in_smooth = T, cur, delta, s[1]
        obj.ball_gaussians = obj.gaussian_2d = False
        mask = (obj.get_marginal_t > 0.05).squeeze()
        frac = float(mask.float().mean())
        assert 0.4 <= frac <= 0.7, frac
        assert float(((marg64(p["taus"], p["betas"], cur) / 0.05 - 1).abs()).min()) >= BAND
        assert bool(((marg64(p["taus"], p["betas"], cur) > 0.05).reshape(-1) == mask).all())
        outs = dict(means=obj.temporal_means[mask], opacities=obj.temporal_opacities[mask], scales=obj.get_scaling[mask],
                    quats=obj.get_quats[mask])
        loss = sum((outs[k] * w[wk][mask]).sum() for k, wk in (("means", "w_m"), ("opacities", "w_o"), ("scales", "w_s"), ("quats", "w_q")))
        loss.backward()
        out.update({f"s{i}_cur_time": np.float64(cur), f"s{i}_delta_t": np.float64(delta), f"s{i}_in_smooth": np.bool_(s[1]),
                    f"s{i}_mask": mask.numpy()})
        out.update({f"s{i}_{k}": v.detach().numpy() for k, v in outs.items()})
        out.update({f"s{i}_grad_{k}": t.grad.numpy() for k, t in ts.items()})
        print(f"s{i}: frame {s[0]} smooth {s[1]} cur_time {cur:.6f} delta_t {delta:+.6f} kept {frac:.3f}")
    path = os.path.join(OUT, "pvg_time.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(OUT, "node_pose_train.npz")), os.path.getsize(path)
    print("wrote pvg_time.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
