#!/usr/bin/env python3
"""Time of the SMPL nodes' fused kNN and skinning-field regularisers (csrc/smpl_reg.hip through ``smpl_reg.knn_reg`` /
``smpl_reg.voxel_reg``, B) against the reference's expressions as framework ops (``smpl_reg.framework_knn_reg`` /
``framework_voxel_reg``, A: per group expand, gather, std, mean, with scatter_add backwards; three shifted differences with
abs().mean() and norm(dim=1).mean()), forward only and forward + backward, and the launches each side makes per step.

    python scripts/smpl_reg_time.py [--out profiles/smpl_reg_time.json] [--reps 30]
    python scripts/smpl_reg_time.py --profile fused|framework --term knn|field [--steps 5]
                                    (that side and term only, forward + backward at I = 8, degree 1, no warm-up: for a
                                     rocprofv3 --kernel-trace --stats run of its own; --steps 0 makes the inputs only)
    python scripts/smpl_reg_time.py --merge-stats knn:fused=<csv>,<csv of --steps 0> knn:framework=... field:fused=... field:framework=...
                                    (adds the dispatches per step, (kernel calls - the input-making run's) / steps, to the JSON; no GPU)

Sizes: I = 8 and 32 humans, V = 6890 points, K = 3 neighbours, SH degree 1 (the shipped config) and 3, the field [I,24,16,64,64].
Device events around each call after a warm-up, A and B alternated over the repeats; the median is reported (ms).  Both sides include
the weighted sum of the terms and its backward, and the gradient buffers autograd makes.  The reverse lists are built once, outside the
timed region (once per ``update_knn`` in training)."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import smpl_reg  # noqa: E402

V, K = 6890, 3
FLOOR = 2.3e-6       # tests/smpl_reg_ref64.FLOOR: the host shim's largest error against float64, measured by tests/test_smpl_reg_cpu.py


def make_knn(I, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = I * V
    t = dict(features_dc=torch.rand(N, 3, generator=g), features_rest=torch.randn(N, (degree + 1) ** 2 - 1, 3, generator=g) * 0.2,
             opacities=torch.randn(N, 1, generator=g), scales=torch.randn(N, 3, generator=g) * 0.3 - 3, quats=torch.randn(N, 4, generator=g))
    t = {k: v.cuda().requires_grad_(True) for k, v in t.items()}
    pts = torch.randn(I, V, 3, generator=g).cuda()
    nn = torch.stack([torch.cdist(p, p).topk(K, dim=1, largest=False).indices for p in pts])       # the query itself and its two nearest
    present = torch.ones(I, dtype=torch.bool).cuda()
    w = torch.tensor([1.0, 0.5, 2.0, 1.5, 0.75]).cuda()
    reverse = (*smpl_reg.reverse_lists(nn), nn.to(torch.int32).contiguous())
    return t, nn, present, w, reverse


def knn_step(t, nn, present, w, reverse, fused, backward):
    for v in t.values():
        v.grad = None
    with torch.set_grad_enabled(backward):
        terms = smpl_reg.knn_reg(nn, present, reverse=reverse, **t) if fused else smpl_reg.framework_knn_reg(nn, present, **t)
        if backward:
            (terms * w).sum().backward()
    return terms


def field_step(x, w, fused, backward):
    x.grad = None
    with torch.set_grad_enabled(backward):
        terms = smpl_reg.voxel_reg(x) if fused else smpl_reg.framework_voxel_reg(x)
        if backward:
            (terms * w).sum().backward()
    return terms


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def merge_stats(out, specs, steps):
    """Kernel calls per step of rocprofv3's kernel-stats CSVs (``term:side=path``) into the JSON."""
    with open(out) as fh:
        doc = json.load(fh)
    table = doc.setdefault("dispatches_per_step", {"note": "dispatches (kernels, fills, copies) of rocprofv3 --kernel-trace --stats runs of forward "
                                                           "+ backward at I = 8, degree 1 (--profile), less those of a run that only makes "
                                                           "the inputs (--steps 0), over the steps"})

    def calls(path):
        with open(path) as fh:
            return sum(int(r["Calls"]) for r in csv.DictReader(fh))
    for spec in specs:
        key, paths = spec.split("=", 1)
        run, base = paths.split(",")
        table[key] = round((calls(run) - calls(base)) / steps, 2)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)


def measure(name, size, step, reps):
    rows = []
    for backward in (True, False):
        for _ in range(5):
            step(True, backward)
            step(False, backward)
        torch.cuda.synchronize()
        tb, ta = [], []
        for _ in range(reps):
            tb.append(timed(lambda: step(True, backward)))
            ta.append(timed(lambda: step(False, backward)))
        mb, ma = statistics.median(tb), statistics.median(ta)
        row = dict(term=name, **size, mode="fwd+bwd" if backward else "fwd", fused_ms=round(mb, 4), framework_ms=round(ma, 4),
                   speedup=round(ma / mb, 2), fused_min_ms=round(min(tb), 4), framework_min_ms=round(min(ta), 4), fused_max_ms=round(max(tb), 4),
                   framework_max_ms=round(max(ta), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/smpl_reg_time.json")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", choices=("fused", "framework"))
    ap.add_argument("--term", choices=("knn", "field"), default="knn")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--merge-stats", nargs="+")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.out, a.merge_stats, a.steps)
    L.lib()
    if a.profile:
        if a.term == "knn":
            knn = make_knn(8, 1)
            torch.cuda.synchronize()
            for _ in range(a.steps):
                knn_step(*knn, a.profile == "fused", True)
        else:
            x, wf = (torch.randn(8, 24, 16, 64, 64) * 0.01).cuda().requires_grad_(True), torch.tensor([1.0, 0.5]).cuda()
            for _ in range(a.steps):
                field_step(x, wf, a.profile == "fused", True)
        torch.cuda.synchronize()
        return
    rows, agree = [], {}
    for I in (8, 32):
        for degree in (1, 3):
            knn = make_knn(I, degree)
            t = knn[0]
            knn_step(*knn, False, True)
            ref = {k: v.grad.clone() for k, v in t.items()}
            knn_step(*knn, True, True)
            agree[f"knn I={I} degree={degree}"] = {k: float((v.grad - ref[k]).abs().max() / ref[k].abs().max()) for k, v in t.items()}
            rows += measure("knn_reg", dict(I=I, V=V, K=K, sh_degree=degree), lambda fused, backward: knn_step(*knn, fused, backward), a.reps)
            del knn, t, ref
        x, wf = (torch.randn(I, 24, 16, 64, 64) * 0.01).cuda().requires_grad_(True), torch.tensor([1.0, 0.5]).cuda()
        field_step(x, wf, False, True)
        ref = x.grad.clone()
        field_step(x, wf, True, True)
        agree[f"field I={I}"] = float((x.grad - ref).abs().max() / ref.abs().max())
        rows += measure("voxel_deformer_reg", dict(I=I, field=[I, 24, 16, 64, 64]), lambda fused, backward: field_step(x, wf, fused, backward), a.reps)
        del x, ref
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, rows=rows, gradient_agreement=agree, floor=FLOOR,
               note="median of device-event times around one call (ms), A and B alternated; both sides include the weighted sum of the "
                    "terms and its backward; gradient_agreement: largest difference over the largest entry per tensor, fused against framework; floor: the "
                    "host shim's largest error against float64 over the test cases (tests/test_smpl_reg_cpu.py), the additive part of the "
                    "GPU test's bound")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
