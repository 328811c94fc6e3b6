#!/usr/bin/env python3
"""One forward + backward of every one-view node (N = 20 000, 256x160, SH degree 3, 3 grid levels), for comparing two trees:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/view_backward_share.py trace    (kernels of each case, fenced by a roll)
    python scripts/view_backward_share.py kernels DIR OUT.json       ordered (kernel, grid, workgroup) per case from the trace's CSV
    python scripts/view_backward_share.py run OUT.pt RUNS            images + gradients of RUNS runs of each case
    python scripts/view_backward_share.py kernels-compare PARENT.json CHANGE.json OUT.json       profiles/view_backward_share_trace.json
    python scripts/view_backward_share.py compare PARENT1.pt PARENT2.pt CHANGE.pt OUT.json [NOTES.json]      (12 runs each; NOTES: what
                                          was not measured, merged in as it is) -> profiles/view_backward_share_ab.json
"""
import csv, glob, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

N, W, H = 20_000, 256, 160
CASES = ("train_view", "frame_graph", "raw_ed", "raw_ed_aa", "act_rgb", "act_ed")


def cases():
    from bilateral_driving_amd import harness as Hn, marshalling as Marsh
    from bilateral_driving_amd.graph_view import FrameGraph
    from bilateral_driving_amd.rendering import rasterization
    dev = torch.device("cuda", 0)
    cams = Hn.ring_cameras(W, H, yaws_deg=(0.0, 125.0), device=dev)
    for c in cams:
        c.viewmat.requires_grad_(True)
    p = {k: v.requires_grad_(True) for k, v in Hn.synthetic_scene(N, seed=0, device=dev).items()}
    grids = [g.requires_grad_(True) for g in Hn.make_grids(3, device=dev)]
    gen = torch.Generator().manual_seed(7)
    skies = [torch.rand(H, W, 3, generator=gen).to(dev).requires_grad_(True) for _ in cams]
    targets = [torch.rand(H, W, 3, generator=gen).to(dev) for _ in cams]
    wt, wa = torch.randn(1, H, W, 4, generator=gen).to(dev), torch.randn(1, H, W, 1, generator=gen).to(dev)
    leaves = list(p.values()) + grids + skies + [c.viewmat for c in cams]

    def grads(extra=()):
        out = {f"grad_{k}": v.grad.clone() for k, v in p.items() if v.grad is not None}
        out.update({f"grad_viewmat{i}": c.viewmat.grad.clone() for i, c in enumerate(cams) if c.viewmat.grad is not None})
        out.update({f"grad_{k}": v.grad.clone() for k, v in extra})
        return out

    def train_view():
        o = Hn.train_view(p, cams[0], grids, 1, skies[0], targets[0])
        return dict(rgb=o["rgb"], depth=o["depth"], opacity=o["opacity"], **grads())

    def frame_graph():      # (the constructor's eager calibration visit + capture, then one replay)
        fr = FrameGraph(p, cams, grids, skies, targets, img_indices=[1, 2])
        assert fr.step() is True
        imgs = {f"{k}{i}": getattr(v, k).clone() for i, v in enumerate(fr.views) for k in ("rgb", "depth", "opacity")}
        return dict(imgs, **grads())

    def dropin(raw, mode, aa):
        model = Hn.VanillaModel(p)
        if raw:
            Marsh.install(Hn.VanillaModel)
        try:
            gs = model.get_gaussians(Hn.reference_camera(cams[0]))
            r, a, meta = rasterization(gs["_means"], gs["_quats"], gs["_scales"], gs["_opacities"].squeeze(), gs["_rgbs"], cams[0].viewmat[None],
                                       cams[0].K[None], W, H, packed=False, absgrad=True, near_plane=0.1, render_mode=mode,
                                       rasterize_mode="antialiased" if aa else "classic")
            meta["means2d"].retain_grad()
            ((r * wt[..., :r.shape[-1]]).sum() + (a * wa).sum() + 1e-5 * (meta["means2d"] ** 2).sum()).backward()
        finally:
            if raw:
                Marsh.uninstall(Hn.VanillaModel)
        names = ("means", "quats", "log_scales", "logits", "dc", "rest")
        m2 = meta["means2d"]
        return dict(rgb=r[..., :3].detach(), depth=r[..., 3:].detach(), alphas=a.detach(), **grads(zip(names, model.parameters())),
                    means2d_grad=m2.grad.clone(), means2d_absgrad=m2.absgrad.clone())

    fns = dict(train_view=train_view, frame_graph=frame_graph, raw_ed=lambda: dropin(True, "RGB+ED", False),
               raw_ed_aa=lambda: dropin(True, "RGB+ED", True), act_rgb=lambda: dropin(False, "RGB", False),
               act_ed=lambda: dropin(False, "RGB+ED", False))
    for name in CASES:
        for t in leaves:
            t.grad = None
        yield name, fns[name]


def main():
    mode = sys.argv[1]
    if mode == "trace":
        fence = torch.zeros(64, device="cuda")
        for _, fn in cases():
            torch.cuda.synchronize(); torch.roll(fence, 1); torch.cuda.synchronize()
            fn()
        torch.cuda.synchronize()
    elif mode == "kernels":
        rows = [r for f in glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(f))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        out, cur = {}, None
        for r in rows:
            if "roll_cuda_kernel" in r["Kernel_Name"]:
                cur = out.setdefault(CASES[len(out)], [])
            elif cur is not None:
                cur.append([r["Kernel_Name"], [int(r[f"Grid_Size_{a}"]) for a in "XYZ"], [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]])
        assert len(out) == len(CASES), (len(out), len(rows))
        json.dump(out, open(sys.argv[3], "w"))
    elif mode == "run":
        res = {}
        for _ in range(int(sys.argv[3])):
            for name, fn in cases():
                res.setdefault(name, []).append({k: v.detach().cpu() for k, v in fn().items()})
        torch.save(res, sys.argv[2])
    elif mode == "kernels-compare":      # PARENT.json CHANGE.json OUT.json: both lists (names through one index table) + the comparison
        par, chg = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        names = sorted({k[0] for d in (par, chg) for v in d.values() for k in v})
        enc = lambda d: {c: [[names.index(k[0]), k[1], k[2]] for k in v] for c, v in d.items()}
        same = {c: dict(launches=[len(par[c]), len(chg[c])], ordered_identical=par[c] == chg[c]) for c in CASES}
        json.dump(dict(what="per case the launches in start order as [index into kernel_names, grid xyz, workgroup xyz], parent and change",
                       comparison=same, kernel_names=names, parent=enc(par), change=enc(chg)), open(sys.argv[4], "w"), separators=(",", ":"))
        print(same)
    elif mode == "compare":      # PARENT1.pt PARENT2.pt CHANGE.pt OUT.json: three processes of 12 runs each, compared half by half
        p1, p2, chg = (torch.load(f) for f in sys.argv[2:5])
        out, worst = {}, (0.0, None)
        for name in CASES:
            for k in (k for k in p1[name][0] if p1[name][0][k].numel()):
                e = out.setdefault(name, {})[k] = {}
                if "grad" not in k:
                    e["bit_identical"] = all(torch.equal(x[k], p1[name][0][k]) for x in p1[name] + p2[name] + chg[name])
                    continue
                diff = lambda xs, ys: max(float((x[k] - y[k]).abs().max()) for x in xs for y in ys)
                for half, sl in (("runs_1_6", slice(0, 6)), ("runs_7_12", slice(6, 12))):
                    cp, pp = diff(chg[name][sl], p1[name][sl]), diff(p2[name][sl], p1[name][sl])
                    e[half] = dict(change_vs_parent=cp, parent_vs_parent=pp, inside_2x=cp <= 2.0 * pp)
                    worst = max(worst, (cp / pp if pp else float(cp > 0) * 1e30, [name, k, half]))
                e["runs_7_12_vs_runs_1_6_parent"] = diff(p1[name][6:12], p1[name][:6])
        ok = all(e.get("bit_identical", True) and all(h["inside_2x"] for h in e.values() if isinstance(h, dict)) for d in out.values() for e in d.values())
        json.dump(dict(what="largest absolute difference over all pairs of runs, per case and tensor: three processes (parent, parent, change) of 12 "
                            "runs each; runs 1-6 and runs 7-12 compared separately, change vs first parent against second parent vs first parent",
                       criterion="images bit-identical over all 36 runs; every gradient tensor and half: change_vs_parent <= 2 x parent_vs_parent",
                       summary=dict(all_inside=ok, largest_ratio=worst[0], largest_ratio_at=worst[1]),
                       **(json.load(open(sys.argv[6])) if len(sys.argv) > 6 else {}), cases=out), open(sys.argv[5], "w"), indent=1)
        print("all inside:", ok, worst)


if __name__ == "__main__":
    main()
