#!/usr/bin/env python3
"""Time of one training view of a SCENE GRAPH through the reference's call sequence (``marshalling.collect_gaussians`` ->
``render_gaussians`` -> the fused colour transform and loss, forward + backward) with the background class's placeholders kept lazy
through the concatenation (``marshalling.install(cls, scene=True)``: ``rendering._RasterizeSceneView``, B) against the same sequence
without the flag (every placeholder materialises at the ``torch.cat``: dense activations, the concatenation of the two SH parameters,
a dense SH pass in each direction, ``rendering._RasterizeView``, A).

    python scripts/scene_view_time.py [--out profiles/scene_view_time.json] [--rows 2000000] [--dense 150000,50000] [--reps 30]
    python scripts/scene_view_time.py --profile a|b [--steps 5]      (that side only, for rocprofv3 --kernel-trace --stats: its
                                                                      launches per step = kernel calls / steps)

The scene: a background class of 2 M rows (``harness.synthetic_scene`` in spatial order, K = 16, degree 3) and two classes of 150 k and
50 k rows that hand over activated tensors (the eager mirror: what the node classes do), one 1920 x 1080 camera.  Device events around
each step after a warm-up; every repeat runs A, B and A again, so the spread of A against A comes from the same call: the medians of
the first and the second A are reported next to B's (ms)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import harness as Hn  # noqa: E402
from bilateral_driving_amd import marshalling as M  # noqa: E402
from bilateral_driving_amd.bilagrid import bilagrid_transform  # noqa: E402

W, H = 1920, 1080


class NodeLike(Hn.VanillaModel):
    """A class that hands over activated tensors, as the node classes do (its own ``get_gaussians``: ``install`` does not reach it)."""

    def get_gaussians(self, cam):
        return M.get_gaussians(self, cam)


def make(rows, dense, dev="cuda"):
    p = Hn.synthetic_scene(rows, seed=0, device=dev)
    p = Hn.reorder_params(p, Hn.spatial_order(p["means"]))
    models = {"Background": Hn.VanillaModel(p)}
    for i, n in enumerate(dense):
        models[f"Nodes{i}"] = NodeLike(Hn.synthetic_scene(n, seed=1 + i, device=dev))
    cam = Hn.ring_cameras(W, H, yaws_deg=(0.0,), device=dev)[0]
    cam.viewmat.requires_grad_(True)
    grids = [g.requires_grad_(True) for g in Hn.make_grids(1, device=dev)]
    gen = torch.Generator().manual_seed(5)
    sky, target = torch.rand(H, W, 3, generator=gen).to(dev), torch.rand(H, W, 3, generator=gen).to(dev)
    return models, cam, grids, sky, target


def leaves(models, cam, grids):
    return [t for m in models.values() for t in m.parameters()] + [cam.viewmat] + grids


def step(models, cam, grids, sky, target, scene):
    for t in leaves(models, cam, grids):
        t.grad = None
    camera = M.process_camera({"camera_to_world": torch.linalg.inv(cam.viewmat), "intrinsics": cam.K, "height": H, "width": W}, torch.tensor([0]))
    M.install(Hn.VanillaModel, scene=scene)
    try:
        gs, _ = M.collect_gaussians(models, {k: i for i, k in enumerate(models)}, camera)
        res, _, info = M.render_gaussians(gs, camera, near_plane=0.1, far_plane=1e10, render_mode="RGB+ED", radius_clip=0.0)
    finally:
        M.uninstall(Hn.VanillaModel)
    rgb = bilagrid_transform(res["rgb_gaussians"], [g[0:1] for g in grids], Hn.FACTORS_3, alpha=res["opacity"], sky=sky)
    out = dict(rgb=rgb, depth=res["depth"], opacity=res["opacity"])
    loss = Hn.training_loss(out, target, grids) + 0.1 * out["depth"].mean() + 0.1 * out["opacity"].mean()
    loss.backward()
    return out, loss, info


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/scene_view_time.json")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--dense", default="150000,50000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", choices=("a", "b"))
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    L.lib()
    dense = [int(x) for x in a.dense.split(",") if x]
    args = make(a.rows, dense)
    if a.profile:
        for _ in range(a.steps):
            step(*args, scene=a.profile == "b")
        torch.cuda.synchronize()
        return
    # the two sides compute the same thing at the timed size
    out_a, loss_a, info_a = step(*args, scene=False)
    ref = [t.grad.clone() for t in leaves(*args[:3])]
    img_a = out_a["rgb"].detach().clone()
    out_b, loss_b, info_b = step(*args, scene=True)
    # (B normalises the raw quaternion once, inside the projection; A normalises it in the class and again in the projection: among
    #  millions of rows a few radii -- ceil(3 sigma) -- land on the other side of an integer)
    d_radii = (info_a["radii"] - info_b["radii"]).abs()
    d_img = (out_b["rgb"].detach() - img_a).abs()
    agree = dict(image=float(d_img.max()), image_mean=float(d_img.mean()), pixels_above_2e5=int((d_img.amax(-1) > 2e-5).sum()),
                 loss=abs(float(loss_b.detach()) - float(loss_a.detach())), radii_differ=int((d_radii > 0).sum()),
                 radii_largest_difference=int(d_radii.max()),
                 visibility_differs=int(((info_a["radii"] > 0) != (info_b["radii"] > 0)).sum()),
                 gradients=max(float((t.grad - r).abs().max() / r.abs().max().clamp(min=1e-30)) for t, r in zip(leaves(*args[:3]), ref)))
    visible = int((info_b["radii"] > 0).sum())
    for _ in range(4):
        step(*args, scene=False)
        step(*args, scene=True)
    torch.cuda.synchronize()
    ta1, tb, ta2 = [], [], []
    for _ in range(a.reps):
        ta1.append(timed(lambda: step(*args, scene=False)))
        tb.append(timed(lambda: step(*args, scene=True)))
        ta2.append(timed(lambda: step(*args, scene=False)))
    ma1, mb, ma2 = statistics.median(ta1), statistics.median(tb), statistics.median(ta2)
    ma = statistics.median(ta1 + ta2)
    row = dict(rows=a.rows, dense=dense, width=W, height=H, visible=visible, a_ms=round(ma, 4), b_ms=round(mb, 4),
               a_first_ms=round(ma1, 4), a_second_ms=round(ma2, 4), a_spread_ms=round(abs(ma1 - ma2), 4), speedup=round(ma / mb, 3),
               a_min_ms=round(min(ta1 + ta2), 4), a_max_ms=round(max(ta1 + ta2), 4), b_min_ms=round(min(tb), 4), b_max_ms=round(max(tb), 4),
               b_faster_than_the_spread=bool(ma - mb > abs(ma1 - ma2)))
    print(json.dumps(row), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, row=row, agreement=agree,
               note="median of device-event times around one forward + backward step (ms); every repeat runs A, B, A; a_spread_ms = "
                    "|median of the first A - median of the second A|; agreement: largest image / loss difference and the largest "
                    "gradient difference over the tensor's largest entry, B against A at the timed size")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
