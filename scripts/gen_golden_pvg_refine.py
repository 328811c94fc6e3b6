#!/usr/bin/env python3
"""Golden vectors for the periodic-vibration Gaussians' density control (bilateral_driving_amd/pvg_densify.py, csrc/refine.hip), produced
by the REFERENCE's own PeriodicVibrationGaussians.refinement_after (models/gaussians/pvg.py:148-265, with split_gaussians, dup_gaussians,
cull_gaussians and the optimiser surgery of models/gaussians/basics.py:162-206) on a real torch.optim.Adam with the class's nine named
groups (:135-146), and by its after_train (:100-133).

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_pvg_refine.py     (needs the reference tree that oracle/gen_golden_refine.py imports; CPU only)

Three patches let the reference run on the CPU and make its noise an input: ``torch.zeros(..., device="cuda")`` (:331) goes to the CPU,
``torch.randn`` is recorded, and ``torch.normal(mean, std)`` becomes ``mean + std * z`` with a recorded unit normal z -- the
``samples [rows, 4]`` of the drop-in: columns 0-2 the randn of :305, column 3 that z.

pvg_refine_<case>.npz: 640 rows, SH degree 2, scene_origin (3, -2, 1), T = 0.2, the ctrl keys of configs/pvg.yaml, at the step
regimes of the schedule -- 3300 densify + full cull, 1300 densify + cull by opacity, 16300 densify and cull without the screen tests
(pvg.yaml splits until step 20000), 20300 cull without densification, 3100 opacity reset --
the two densifying steps with no_time_split true (the shipped value, suffix _nts) and false (_ts), and step 3300 with
densify_until_num_points below N (_full: culls only).  pvg_refine_stats.npz: three consecutive after_train calls.
The inputs are built by tests/pvg_refine_ref64.py (``synthetic`` + ``settle``): every decision input, a child's cull decision included,
lies at least 1e-4 (relative, float64) from its threshold, so no row is excluded from any comparison."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
N, K, LAST_SIZE = 640, 9, 960
CASES = (("step3300_nts", 3300, {}), ("step3300_ts", 3300, dict(no_time_split=False)), ("step1300_nts", 1300, {}),
         ("step1300_ts", 1300, dict(no_time_split=False)), ("step16300", 16300, {}), ("step20300", 20300, {}), ("step3100", 3100, {}),
         ("step3300_full", 3300, dict(densify_until_num_points=500)))


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gen_golden_refine as G
    G.import_reference()
    from models.gaussians.pvg import PeriodicVibrationGaussians as PVG
    from tests import pvg_refine_ref64 as R
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("refine_"))
    real_randn, real_zeros, real_normal = torch.randn, torch.zeros, torch.normal
    for name, step, over in CASES:
        ctrl = dict(R.CTRL, sh_degree=2, **over)
        noise_fn = R.seeded_noise(step)
        P, stats = R.synthetic(N, seed=step + len(over), K=K)
        R.settle(P, stats, step, ctrl, noise_fn)
        assert float(R.margins(P, stats, step, ctrl, noise_fn).min()) >= R.BAND
        g = torch.Generator().manual_seed(step + 7)
        grads = {a: torch.randn(v.shape, generator=g) * 0.01 for a, v in P.items()}
        model = PVG(class_name="Background", ctrl=R.Cfg(ctrl), scene_scale=R.SCENE_SCALE, scene_origin=torch.tensor(R.ORIGIN),
                    num_train_images=R.NUM_TRAIN_IMAGES, device=torch.device("cpu"))
        for a in R.ATTRS:
            setattr(model, a, torch.nn.Parameter(P[a].clone()))
        groups = [{"params": v, "lr": 0.0, "eps": 1e-15, "weight_decay": 0, "name": k} for k, v in model.get_gaussian_param_groups().items()]
        assert [g_["name"] for g_ in groups] == [model.class_prefix + n for n in R.GROUPS]
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for a in R.ATTRS:
            getattr(model, a).grad = grads[a].clone()
        opt.step()                                                 # populates exp_avg / exp_avg_sq; lr 0 leaves the settled parameters
        rec = {"step": np.array(step), "N": np.array(N), "scene_scale": np.array(R.SCENE_SCALE), "scene_origin": np.array(R.ORIGIN, np.float32),
               "num_train_images": np.array(R.NUM_TRAIN_IMAGES)}
        for k, v in ctrl.items():
            rec["ctrl_" + k] = np.array(v)
        for a in R.ATTRS:
            prm = getattr(model, a)
            assert torch.equal(prm.detach(), P[a])
            rec["in" + a] = prm.detach().numpy().copy()
            rec["in_m" + a] = opt.state[prm]["exp_avg"].numpy().copy()
            rec["in_v" + a] = opt.state[prm]["exp_avg_sq"].numpy().copy()
        for k, v in stats.items():
            setattr(model, k, v.clone())
            rec["in_" + k] = v.numpy().copy()
        model.step = step
        noise, zs = [], []

        def recording_randn(*a, **k):
            t = real_randn(*a, **k)
            noise.append(t.clone())
            return t

        def cpu_zeros(*a, **k):
            k.pop("device", None)
            return real_zeros(*a, **k)

        def normal_from_z(mean, std):
            z = real_randn(std.shape)
            zs.append(z.clone())
            return mean + std * z
        torch.manual_seed(step)
        torch.randn, torch.zeros, torch.normal = recording_randn, cpu_zeros, normal_from_z
        try:
            model.refinement_after(step, opt)
        finally:
            torch.randn, torch.zeros, torch.normal = real_randn, real_zeros, real_normal
        rec["samples"] = (torch.cat([noise[0], zs[0]], 1) if noise else torch.zeros(0, 4)).numpy()
        if noise:
            assert torch.equal(torch.from_numpy(rec["samples"]), noise_fn(rec["samples"].shape[0]))     # the draw settle() judged
        for a, n in zip(R.ATTRS, R.GROUPS):
            prm = getattr(model, a)
            st = opt.state[prm]
            rec["out" + a] = prm.detach().numpy().copy()
            rec["out_m" + a] = st["exp_avg"].numpy().copy()
            rec["out_v" + a] = st["exp_avg_sq"].numpy().copy()
            grp = [g_ for g_ in opt.param_groups if g_["name"] == model.class_prefix + n][0]
            assert grp["params"][0] is prm
        assert model.xys_grad_norm is None and model.t_grad_accum is None and model.vis_counts is None and model.max_2Dsize is None
        pop = R.populations(P, stats, step, ctrl, noise_fn)
        path = os.path.join(OUT, f"pvg_refine_{name}.npz")
        np.savez_compressed(path, **rec)
        size = os.path.getsize(path)
        print(f"{name}: {N} -> {model.num_points} points, noise rows {rec['samples'].shape[0]}, {size} bytes, {pop}")
        assert size <= limit, (size, limit)

    # after_train: one initialising and two accumulating calls
    calls = R.stats_calls(N, seed=11)
    model = PVG(class_name="Background", ctrl=R.Cfg(dict(R.CTRL, sh_degree=2)), scene_scale=R.SCENE_SCALE, num_train_images=R.NUM_TRAIN_IMAGES,
                device=torch.device("cpu"))
    model._means = torch.nn.Parameter(torch.zeros(N, 3))
    model._taus = torch.nn.Parameter(torch.zeros(N, 1))
    rec = {"N": np.array(N), "last_size": np.array(LAST_SIZE)}
    for i, c in enumerate(calls):
        model.filter_mask = c["filter_mask"]
        model._taus.grad = c["taus_grad"].clone()
        model.after_train(c["radii"], c["xys_grad"], LAST_SIZE)
        assert 0 < int((c["radii"] == 0).sum()) < c["radii"].numel() < N
        for k, v in c.items():
            rec[f"c{i}_{k}"] = v.numpy().copy()
        for k in R.STATS:
            rec[f"c{i}_out_{k}"] = getattr(model, k).numpy().copy()
    np.savez_compressed(os.path.join(OUT, "pvg_refine_stats.npz"), **rec)
    print("wrote pvg_refine_stats.npz", os.path.getsize(os.path.join(OUT, "pvg_refine_stats.npz")))


if __name__ == "__main__":
    main()
