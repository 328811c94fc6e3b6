#!/usr/bin/env python3
"""Density control of the periodic-vibration Gaussians at 1 M rows (SH degree 3, the nine-group Adam state): the fused path
(bilateral_driving_amd.pvg_densify) against the reference's sequence restated as framework ops on the same device
(pvg_densify.framework_*: models/gaussians/pvg.py:100-133, :148-372, :430-435 with basics.py:162-206).

    python scripts/pvg_refine_time.py [--rows 1000000] [--out profiles/pvg_refine_time.json]        (on the GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/pvg_refine_time.py --profile        (the fused side alone, a run of its own)

Three parts, each timed with device events around the whole region (host waits inside it included), after a warm-up, A (framework
ops) and B (fused) alternating in one process; the JSON holds the median, the minimum and the maximum of the repeated regions in ms:
  after_train        one accumulating call (M ~ 0.6 N kept rows, 70 % of them visible)
  velocity_reg       forward + read-back of the count + backward
  refinement_after   one densifying step with the full cull (step 3300), inputs as tests/pvg_refine_ref64.synthetic builds them
                     (the split / dup / cull fractions of the golden vectors); the model and optimizer are rebuilt outside the region.
A's refinement works on plain dicts of tensors (no nn.Parameter wrapping, no optimizer bookkeeping), which favours A slightly."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bilateral_driving_amd import pvg_densify as PD
from tests import pvg_refine_ref64 as R

STEP, LAST = 3300, 1920


def region(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def alternate(make_a, make_b, warmup, repeats):
    """make_x() -> the region's callable (set-up outside the region).  Returns {A: [ms], B: [ms]} and the last results."""
    ms, last = {"A": [], "B": []}, {}
    for i in range(warmup + repeats):
        for name, make in (("A", make_a), ("B", make_b)):
            t, last[name] = region(make())
            if i >= warmup:
                ms[name].append(t)
    return ms, last


def summary(ms):
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "regions": len(v)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvg_refine_time.json"))
    ap.add_argument("--profile", action="store_true", help="run the fused side only, a few times, and write nothing")
    a = ap.parse_args()
    N, dev = a.rows, "cuda"
    ctrl = R.Cfg(dict(R.CTRL, sh_degree=3))
    P, stats = R.synthetic(N, seed=1, K=16, special=min(N // 9, 2000))
    M, V = R.moments(P, 2)
    cu = lambda d: {k: v.to(dev) for k, v in d.items()}
    Pd, Md, Vd, Sd = cu(P), cu(M), cu(V), cu(stats)
    origin = torch.tensor(R.ORIGIN, device=dev)
    res = {"rows": N, "sh_degree": 3, "step": STEP, "device": torch.cuda.get_device_name(0)}

    # ---- after_train: an accumulating call
    c = cu(R.stats_calls(N, seed=3, calls=1)[0])
    sa = {k: Sd[k].clone() for k in R.STATS}
    sb = tuple(Sd[k].clone() for k in R.STATS)
    alt = alternate
    if a.profile:       # B only
        alt = lambda make_a, make_b, warmup, repeats: (None, [region(make_b()) for _ in range(repeats)][-1])
    ms, _ = alt(lambda: lambda: PD.framework_after_train(sa, c["filter_mask"], c["radii"], c["xys_grad"], c["taus_grad"], LAST),
                      lambda: lambda: PD.densify_stats(sb, c["filter_mask"], c["radii"], c["xys_grad"], c["taus_grad"], LAST), 3, 20)
    res["after_train"] = None if a.profile else summary(ms)

    # ---- velocity_reg: forward, the count's read-back, backward
    vel, betas = Pd["_velocity"].clone().requires_grad_(True), Pd["_betas"].clone().requires_grad_(True)

    def reg_a():
        vel.grad = betas.grad = None
        loss = PD.framework_velocity_reg(vel, betas, c["filter_mask"], c["radii"], R.T)
        if loss is not None:
            (loss * 0.01).backward()
        return None if loss is None else float(loss.detach())

    def reg_b():
        vel.grad = betas.grad = None
        total, out = PD.velocity_reg(vel, betas, c["filter_mask"], c["radii"], R.T)
        _, count = out.tolist()
        if count:
            (total / count * 0.01).backward()
        return float(total.detach()) / count if count else None
    ms, last = alt(lambda: reg_a, lambda: reg_b, 3, 20)
    if not a.profile:
        res["velocity_reg"] = dict(summary(ms), value_A=last["A"], value_B=last["B"])

    # ---- refinement_after: one densifying step with the full cull
    d = PD.framework_decisions(Pd, Sd, PD.schedule(STEP, ctrl, R.NUM_TRAIN_IMAGES, N), ctrl, R.SCENE_SCALE, origin)
    n_split = int(d["splits"].sum())
    samples = torch.randn(2 * n_split, 4, device=dev)

    def make_a():
        p, m, v, s = ({k: t.clone() for k, t in x.items()} for x in (Pd, Md, Vd, Sd))
        return lambda: PD.framework_refinement(p, m, v, s, STEP, ctrl, R.SCENE_SCALE, origin, R.NUM_TRAIN_IMAGES, R.T, samples)[3]

    def make_b():
        model = types.SimpleNamespace(ctrl_cfg=ctrl, scene_scale=R.SCENE_SCALE, scene_origin=origin, num_train_images=R.NUM_TRAIN_IMAGES,
                                      step=STEP, class_prefix="Background#", T=R.T)
        groups = []
        for at, n in zip(R.ATTRS, R.GROUPS):
            prm = torch.nn.Parameter(Pd[at].clone())
            setattr(model, at, prm)
            groups.append({"params": [prm], "lr": 1e-3, "eps": 1e-15, "name": model.class_prefix + n})
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for at in R.ATTRS:
            opt.state[getattr(model, at)] = {"step": torch.tensor(1.0), "exp_avg": Md[at].clone(), "exp_avg_sq": Vd[at].clone()}
        for k in R.STATS:
            setattr(model, k, Sd[k].clone())

        def run():
            with contextlib.redirect_stdout(io.StringIO()):
                PD.refinement_after(model, STEP, opt, samples=samples)
            return model._means.shape[0]
        return run
    ms, last = alt(make_a, make_b, 1, 5)
    if a.profile:
        return
    counts = {k: last["A"][k] for k in ("split", "dup", "cull")}
    left = N + 2 * counts["split"] + counts["dup"] - counts["cull"]
    assert last["B"] == left, (last["B"], left)
    res["refinement_after"] = dict(summary(ms), rows_after=left, **counts)
    for k in ("after_train", "velocity_reg", "refinement_after"):
        r = res[k]
        print(f"{k:17s} A {r['A']['median_ms']:9.3f} ms [{r['A']['min_ms']:.3f}, {r['A']['max_ms']:.3f}]   B {r['B']['median_ms']:9.3f} ms "
              f"[{r['B']['min_ms']:.3f}, {r['B']['max_ms']:.3f}]   A / B {r['A']['median_ms'] / r['B']['median_ms']:.1f}")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
