#!/usr/bin/env python3
"""Benchmark of the hot path: train iterations/sec (forward + backward of one view) of the differentiable
Gaussian-splat rasterizer + fused multi-scale bilateral-grid colour transform.

    python bench.py --gpus N --steps K --warmup W [--workload headline|c2|c3|c5] [--dump-outputs DIR] [--full]

One STEP = one FRAME: every rank renders the views of its rig once (BASELINE.json: "2M Gaussians x 6 views x 1920x1080 fwd+bwd",
"6 cams x 8 timesteps sharded across 8 GPUs"): per view SH -> projection -> tile intersection + ordering -> alpha compositing
(RGB + expected depth) -> clamp + sky blend + bilateral slice + affine -> L1 + TV loss -> full backward incl. the camera-pose
gradient; the views' gradients are summed into ONE flat gradient buffer (the visible rows only), and at N > 1 also over the ranks
(dist.FrameExchange: per-view compact all-reduce over RCCL, overlapped with the next view).  Rank r's rig sits 1.5 m x r further
along the road (its own timestep), so the ranks see different -- overlapping -- parts of the scene.
`value` = views (iterations) processed by all ranks per second ("weak" scaling: one frame per GPU per step).

Prints ONE JSON line on rank 0: the headline (`value`, `ms_per_step` = milliseconds of one timed step, the workload in `config`).
A plain run sets up, warms up, times exactly --steps steps once, and prints that line.  --full adds what takes runs of its own:
the median of --repeats (default 5) timed regions, `roofline` (dominant kernel, HIP-event timed on the launch stream inside the
timed region), the per-operator table, `selfcheck` (the timed frame against the eager frame; exit status 3 when they differ),
the replayable-frame / other-row-order / drop-in-path / training-cadence figures, the exchange probe and `cpu_baseline` (the
oracle/ port of the same pipeline on the host cores, bounded sample, rank 0 at N=1 only).

--dump-outputs DIR writes what the last timed step computed, rank 0's view of it, as DIR/<name>.npy (float32; the losses
float64): per view the loss, a fixed seeded sample of the pixels of the image / expected depth / opacity and of the sky
colour's gradient, the camera-pose gradients, a fixed seeded sample of the rows of every per-Gaussian gradient and the grids'
gradients in full -- at most 64 MB.  The inputs are seeded: equal arguments give equal inputs, so two builds can be compared
output for output.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)

# BASELINE.json configs: name -> (Gaussians, yaws, W, H, grid levels (gx, gy, L), guidance factors)
WORKLOADS = {
    "headline": dict(gaussians=2_000_000, rig="six", width=1920, height=1080, levels=((2, 2, 1), (4, 4, 2), (8, 8, 4)), factors=(4, 4, 2),
                     text="BASELINE.json metric: 2M Gaussians, 6-cam ring 1920x1080, SH deg 3, 3-level bilateral grid"),
    "c2": dict(gaussians=500_000, rig="one", width=1920, height=1080, levels=((16, 16, 8),), factors=(1,),
               text="configs[1]: 500k Gaussians, single 1920x1080 view, SH deg 3, single-scale 16x16x8 bilateral grid"),
    "c3": dict(gaussians=2_000_000, rig="six", width=1600, height=900, levels=((2, 2, 1), (4, 4, 2), (8, 8, 4)), factors=(4, 4, 2),
               text="configs[2]: 2M Gaussians, nuScenes 6-cam frame at 1600x900, 3-level multi-scale bilateral grid"),
    "c5": dict(gaussians=5_000_000, rig="five", width=1920, height=1280, levels=((2, 2, 1), (4, 4, 2), (8, 8, 4), (16, 16, 8)),
               factors=(8, 4, 4, 2),
               text="configs[4]: 5M Gaussians, Waymo 5-cam 1920x1280, SH deg 3, 4-level bilateral grid (guidance factors 8,4,4,2)"),
}


def _physical_cores() -> int:
    """Physical cores of the host (distinct (package, core) pairs of /proc/cpuinfo; psutil or half the logical count as fall-backs)."""
    try:
        seen, pkg = set(), None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pkg = line.split(":")[1].strip()
            elif line.startswith("core id"):
                seen.add((pkg, line.split(":")[1].strip()))
        if seen:
            return len(seen)
    except OSError:
        pass
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return int(n)
    except Exception:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps; one step = one frame (all views of the rig) per rank")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="headline")
    ap.add_argument("--scene", choices=("ring", "lidar"), default="ring",
                    help="ring: SURVEY.md 8(d)'s synthetic scene (BASELINE.json's metric is quoted on it).  lidar: a lidar-INITIALISED street "
                         "scene as the reference seeds its Background class (harness.lidar_scene: 0.8 N points on road / facades / clutter + "
                         "0.1 N near + 0.1 N far randoms, isotropic scales = mean 3-NN distance; default N = 1 M) -- the other end of the "
                         "splat-size distribution, same rig, same line")
    ap.add_argument("--lidar-opacity", choices=("trained", "init"), default="trained")
    ap.add_argument("--gaussians", type=int, default=None)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--views-per-step", type=int, default=None, help="views of the rig rendered per step (default: all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pair-stats", action="store_true")
    ap.add_argument("--no-api-path", action="store_true", help="skip the short measurement of the reference-signature operator chain")
    ap.add_argument("--cpu-sample-gaussians", type=int, default=100000)
    ap.add_argument("--cpu-sample-width", type=int, default=960)
    ap.add_argument("--cpu-sample-height", type=int, default=540)
    ap.add_argument("--cpu-threads", type=int, default=_physical_cores(),
                    help="threads of the CPU baseline: the host's PHYSICAL cores by default (SURVEY.md 8d), stated in the line")
    ap.add_argument("--cpu-timeout", type=float, default=170.0)
    ap.add_argument("--cpu-baseline-only", action="store_true")
    ap.add_argument("--exchange-probe-only", action="store_true", help="(child process of the default run) see exchange_probe_worker")
    ap.add_argument("--no-exchange-probe", action="store_true",
                    help="N = 1: skip the child process that runs the frame with the multi-GPU exchange's collectives really issued over "
                         "RCCL at world size 1 (config.exchange_world1: ms per frame without an exchange, per view, per frame)")
    ap.add_argument("--probe-timeout", type=float, default=150.0)
    ap.add_argument("--no-train-cadence", action="store_true",
                    help="N = 1: skip config.train_cadence (one view per step; + optimizer step and densification statistics: the reference's loop)")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the timed region of --steps steps is run this many times (barrier + synchronize around each); the MEDIAN "
                         "repeat is reported (a 0.2 s window on a shared host can swing 10-20 %), min / max beside it.  Default: 1, "
                         "with --full 5")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline (module docstring); a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (module docstring)")
    ap.add_argument("--no-graph", action="store_true",
                    help="N = 1: drive the frame through the eager host-count loop (one host wait per view, ~40 launches from Python) "
                         "instead of replaying the captured hipGraphs of graph_view.FrameGraph (default: same kernels, same order, "
                         "device-side list counts, one launch per view)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="graph replay: one graph per view on one stream instead of forward / backward graphs on two streams (view v + 1's "
                         "forward next to view v's backward)")
    ap.add_argument("--row-order", choices=("spatial", "given"), default=os.environ.get("BDS_BENCH_ROW_ORDER", "spatial"),
                    help="order of the scene's rows in memory: spatial = Morton order of the centres (densify.spatial_order, the framework's "
                         "layout: applied once at load, outside the timed region), given = the generator's own order")
    ap.add_argument("--exchange", choices=("auto", "view", "frame"), default="auto",
                    help="N > 1: sum the gradients over the ranks per view (compact union rows, overlapped with the next view), once per "
                         "frame (one dense all-reduce), or whichever dist.plan_exchange prices cheaper from the measured unions, the "
                         "measured compute time of a frame and the measured all-reduce bandwidth of the fabric (default)")
    ap.add_argument("--no-random-views", dest="random_views", action="store_false",
                    help="skip the measurement of the REPLAYABLE frame.  Default at N = 1: also time the replayable frame (graph_view.FrameGraph(dynamic=True)) -- every step each view slot gets "
                         "a random camera of a pool, a new target / sky and a random image index written into its static inputs before "
                         "the replay, as the reference's loop draws a random image per step (tools/train.py:250-283); reported as "
                         "config.random_views_iters_per_sec next to the fixed-frame value")
    ap.add_argument("--dense-grads", action="store_true",
                    help="N = 1 only: fresh dense gradient tensors per view (zero fill of all N rows, autograd accumulation) instead of "
                         "the flat gradient buffer whose rows are cleared / written through the visible-id lists")
    return ap.parse_args()


def _cpu_iter_fn(N, W, H):
    """One fwd+bwd of the oracle/ port (the checker; here only as the timed CPU baseline)."""
    from bilateral_driving_amd import harness as Hn
    from oracle import bilagrid_oracle as BO
    from oracle import gs_oracle as G

    cam = Hn.ring_cameras(W, H, yaws_deg=(0.0,))[0]
    p = Hn.synthetic_scene(N, seed=0)
    if N <= 2000:
        p["means"] = p["means"] * torch.tensor([0.25, 0.25, 1.0])
    grids = Hn.make_grids(1)
    gen = torch.Generator().manual_seed(3)
    sky = torch.rand(H, W, 3, generator=gen)
    target = torch.rand(H, W, 3, generator=gen)

    def one():
        q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        g = [x.clone().requires_grad_(True) for x in grids]
        dirs = q["means"].detach() - torch.linalg.inv(cam.viewmat)[:3, 3]
        col = torch.clamp(G.spherical_harmonics(3, dirs, q["sh"]) + 0.5, 0.0, 1.0)
        r, a, _ = G.rasterization(q["means"], q["quats"] / q["quats"].norm(dim=-1, keepdim=True), torch.exp(q["log_scales"]),
                                  torch.sigmoid(q["opacity_logits"]), col, cam.viewmat[None], cam.K[None], W, H,
                                  near_plane=0.1, render_mode="RGB+ED")
        rgb = BO.multiscale_transform([x[0] for x in g], BO.sky_blend(r[0, ..., :3], a[0], sky), list(Hn.FACTORS_3))
        loss = (rgb - target).abs().mean() + 0.01 * BO.multiscale_tv(g)
        loss.backward()

    return one


def cpu_baseline_worker(args):
    """Runs in a child process (so that a pathological host cannot hang the benchmark): times the oracle/ port -- best of 3 -- at
    configs[0] (1k Gaussians, 256x256) and on a bounded sample of the GPU workload, and prints one JSON object."""
    threads = args.cpu_threads
    torch.set_num_threads(threads)

    def best_of(fn, reps, budget):
        fn()   # warm-up (allocator, thread pool)
        best, t_all = None, time.perf_counter()
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            if time.perf_counter() - t_all + dt > budget:
                break
        return best

    t_c1 = best_of(_cpu_iter_fn(1000, 256, 256), 3, 20.0)
    # the port is a chain of small framework operators: on a many-core host it can be SLOWER with every physical core than with a
    # few (measured on the 128-core GPU box: configs[0] 0.76 it/s at 128 threads, 5.2 at 16).  Both are timed at configs[0]; the
    # faster setting runs the sample and is the `cores` of the line, the other figure is kept beside it.
    alt, c1_alt = (16 if threads > 16 else None), None
    if alt:
        torch.set_num_threads(alt)
        t_alt = best_of(_cpu_iter_fn(1000, 256, 256), 3, 20.0)
        c1_alt = {"threads": alt, "c1_value": 1.0 / t_alt}
        if t_alt < t_c1:
            c1_alt = {"threads": threads, "c1_value": 1.0 / t_c1}
            threads, t_c1 = alt, t_alt
        else:
            torch.set_num_threads(threads)
    small = (20000, 480, 270)
    big = (args.cpu_sample_gaussians, args.cpu_sample_width, args.cpu_sample_height)
    t_small = best_of(_cpu_iter_fn(*small), 1, 30.0)
    sample, dt = small, t_small
    # the big sample costs ~15x the small one (measured); only run it if best-of-3 fits the budget
    if t_small * 15.0 * 4 < 110.0:
        dt = best_of(_cpu_iter_fn(*big), 3, 90.0)
        sample = big
    print(json.dumps({
        "value": 1.0 / dt, "unit": "iters/sec", "cores": threads, "kind": "port",
        "sample": f"{sample[0]} Gaussians, one {sample[1]}x{sample[2]} view, SH3 + 3-level bilateral grid, fwd+bwd, fp32 "
                  f"pure-PyTorch CPU port (oracle/), best of 3; NOT the GPU workload size "
                  f"(host: {_physical_cores()} physical cores / {os.cpu_count()} logical CPUs; {threads} torch threads used)",
        "c1_value": 1.0 / t_c1, "c1_sample": "configs[0]: 1000 Gaussians, one 256x256 view, same pipeline, best of 3",
        "physical_cores": _physical_cores(), "other_thread_count": c1_alt,
    }))


def cpu_baseline(args):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--cpu-threads", str(args.cpu_threads),
           "--cpu-sample-gaussians", str(args.cpu_sample_gaussians), "--cpu-sample-width", str(args.cpu_sample_width),
           "--cpu-sample-height", str(args.cpu_sample_height)]
    env = dict(os.environ, OMP_NUM_THREADS=str(args.cpu_threads), MKL_NUM_THREADS=str(args.cpu_threads))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.cpu_timeout)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        return json.loads(line)
    except Exception as e:  # timeout or failure: report it, never hang the benchmark
        return {"value": None, "unit": "iters/sec", "cores": args.cpu_threads, "kind": "port",
                "sample": f"not measured: {type(e).__name__} (limit {args.cpu_timeout}s)"}


def _newest_profile(suffix, kernel_substr, field, workload="headline"):
    """Value `field` of the kernel in the newest committed rocprofv3 summary profiles/*<suffix> of this workload (files of the other
    BASELINE workloads carry `_c2_` / `_c3_` / `_c5_` in their names; bench.py cannot collect counters itself: gfx950 counter
    passes are separate rocprofv3 runs of this same command, scripts/gpu_round.sh)."""
    import glob
    others = ("_c2_", "_c3_", "_c5_", "_lidar_")
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*" + suffix)), reverse=True):
        base = os.path.basename(f)
        if (workload == "headline" and any(o in base for o in others)) or (workload != "headline" and f"_{workload}_" not in base):
            continue
        try:
            d = json.load(open(f))["kernels"]
        except Exception:
            continue
        for k, v in d.items():
            if kernel_substr in k and field in v:
                return v[field], os.path.basename(f)
    return None, None


# kernels of ONE replayed view of the headline frame (name substring, launches per view): what `frame_valu_issue_frac` sums
_FRAME_KERNELS = (("project_view_fwd_kernel<true>", 1), ("visible_compact_kernel", 1), ("short_hist_kernel", 3), ("short_scatter_kernel", 4),
                  ("isect_count_rows_kernel", 1), ("finish_counts_kernel", 1), ("isect_emit_rows_kernel", 1), ("radix_hist_wide_kernel", 1),
                  ("radix_scatter_keys_wide_kernel", 1), ("tile_stage_persistent_kernel", 1), ("splat_pack_sh_kernel", 1),
                  ("rasterize_fwd_wave_kernel<4, true, true>", 1), ("ms_tile_fwd_kernel<3, true>", 1), ("ms_apply_bwd_x_kernel", 1),
                  ("ms_tile_bwd_kernel", 1), ("cell_bwd_kernel<false>", 1), ("ms_guidance_blend_bwd_kernel", 1), ("rasterize_bwd_wave_kernel<4, true, true, false>", 1),
                  ("sh_view_bwd_list_kernel<3, true, true>", 1), ("project_view_bwd_list_kernel<true, true, true>", 1),
                  ("view_grads_clear_list_kernel", 1))


def _frame_valu_issue(ms_per_view, workload="headline", clock_ghz=2.4):
    """Vector-issue time of one view's kernels / the measured time per view.  A wave64 vector instruction occupies its SIMD's issue
    port for 4 cycles: the committed SQ counter pass (profiles/*_sq_counters.json, SQ_ACTIVE_INST_VALU per launch) summed over the
    frame's kernels x 4 / (1024 SIMDs x clock) is the time the view would take if every SIMD issued a vector instruction every
    cycle it could -- the floor of this instruction mix; the fraction says how much of the frame's time the issue ports are busy."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_sq_counters.json")), reverse=True):
        base = os.path.basename(f)
        if any(o in base for o in ("_c2_", "_c3_", "_c5_")) != (workload != "headline") or (workload != "headline" and f"_{workload}_" not in base):
            continue
        try:
            ks = json.load(open(f))["kernels"]
        except Exception:
            continue
        busy, used = 0.0, []
        for pat, mult in _FRAME_KERNELS:
            hit = [v for k, v in ks.items() if pat in k and "SQ_ACTIVE_INST_VALU" in v]
            if hit:
                busy += mult * 4.0 * hit[0]["SQ_ACTIVE_INST_VALU"]
                used.append(pat)
        if not used:
            continue
        issue_ms = busy / 1024.0 / (clock_ghz * 1e9) * 1e3
        return {"value": issue_ms / ms_per_view, "issue_ms_per_view": issue_ms, "ms_per_view": ms_per_view, "counter_source": base,
                "kernels_found": len(used), "clock_ghz_assumed": clock_ghz,
                "note": "sum over the view's kernels of 4 x SQ_ACTIVE_INST_VALU / (1024 SIMDs x clock) from the committed counter pass, "
                        "divided by the measured time per view: the share of the frame in which the vector issue ports are busy"}
    return None


def _pair_stats(N, W, H, params=None):
    spec = importlib.util.spec_from_file_location("pair_stats", os.path.join(ROOT, "scripts", "pair_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pair_stats(N, W, H, view=0, params=params)


def build_scene(args, dev, rank):
    """SURVEY.md 8(d)'s synthetic scene of the workload on ``dev`` (rank r's rig sits 1.5 m x r further along the road)."""
    from bilateral_driving_amd import harness as Hn
    wl = dict(WORKLOADS[args.workload])
    N = args.gaussians or (1_000_000 if args.scene == "lidar" else wl["gaussians"])
    W, H = args.width or wl["width"], args.height or wl["height"]
    yaws = {"six": Hn.SIX_CAM_YAWS, "five": Hn.FIVE_CAM_YAWS, "one": (0.0,)}[wl["rig"]]
    cams = Hn.ring_cameras(W, H, yaws_deg=yaws, device=dev, origin=(1.5 * rank, 0.0, 0.0))   # this rank's timestep of the drive
    for cam in cams:   # the camera pose is learnable in the reference (trainers/base.py:328-329,399): its gradient stays live
        cam.viewmat.requires_grad_(os.environ.get("BDS_BENCH_NO_POSE") != "1")   # (diagnostic switch)
    params = Hn.synthetic_scene(N, seed=0, device=dev) if args.scene == "ring" else Hn.lidar_scene(N, seed=0, device=dev, opacity=args.lidar_opacity)
    # the scene's rows in Morton order of the centres (densify.spatial_order, applied ONCE at load as a trainer would -- and again after
    # densification steps: refinement_after(reorder=True)): the ~15 % of the rows a camera sees then form runs, and every list-driven
    # kernel of a view moves whole cache lines.  --row-order given keeps the generator's own (random) order: the figure of rounds 1-4
    if args.row_order == "spatial":
        perm = Hn.spatial_order(params["means"])
        params = {k: v[perm].contiguous() for k, v in params.items()}
    for v in params.values():
        v.requires_grad_(True)
    grids = [g.requires_grad_(True) for g in Hn.make_grids(len(cams), levels=wl["levels"], device=dev)]
    gen = torch.Generator().manual_seed(7)
    # the sky colour comes from a trainable sky model in the reference: its gradient path stays live
    skies = [torch.rand(H, W, 3, generator=gen).to(dev).requires_grad_(True) for _ in cams]
    targets = [torch.rand(H, W, 3, generator=gen).to(dev) for _ in cams]
    return wl, N, W, H, yaws, cams, params, grids, skies, targets


def train_cadence(args, params, cams, grids, skies, targets, factors, V, dev):
    """The reference's TRAINING cadence at this workload's size (what `value` -- fwd + bwd of a frame of views, gradients accumulated,
    view v + 1's forward next to view v's backward -- leaves out):

      one_view_step         a frame of ONE view per step, nothing to overlap with (tools/train.py:252-283: one image per iteration);
      train_step            that + the optimizer step over EVERY parameter + the densification statistics of the view
                            (models/trainers/base.py:502-516 step, :222-226 one dense Adam over all groups, :279-297 statistics),
                            with the dense one-pass FusedAdam and with optim.DeferredRowAdam (the SH rows step through the view's
                            visible-id list, missed zero-gradient steps replayed in the next forward that sees the row: same numbers);
      train_frame           the frame of all views + ONE optimizer step + the statistics of every view.

    Every variant starts from a copy of the same parameters; the reference's learning rates (configs/omnire_ms_bilateral_extended.yaml
    :39-52); a random camera of the rig per step where the frame has one view."""
    from bilateral_driving_amd import _lib as L
    from bilateral_driving_amd.graph_view import FrameGraph
    from bilateral_driving_amd.optim import DeferredRowAdam, FusedAdam
    steps = max(6, min(args.steps, 30))
    N = params["means"].shape[0]
    W, H = cams[0].width, cams[0].height
    lrs = dict(means=1.6e-4, quats=1e-3, log_scales=5e-3, opacity_logits=5e-2)
    gen = torch.Generator().manual_seed(11)
    picks = torch.randint(0, len(cams), (steps + 3,), generator=gen).tolist()
    out = {"steps": steps}

    def variant(n_views, optim):
        p = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        g = [x.detach().clone().requires_grad_(True) for x in grids]
        sk = [s.detach().clone().requires_grad_(True) for s in skies[:n_views]]
        opt = None
        if optim is not None:
            groups = [{"params": [p[k]], "lr": lr, "eps": 1e-15} for k, lr in lrs.items()] + [{"params": [x], "lr": 2e-3, "eps": 1e-15} for x in g]
            if optim == "deferred":
                groups.append({"params": [p["sh"]], "lr": 2.5e-3, "lr_b": 1.25e-4, "col_split": 3, "deferred_rows": True, "eps": 1e-15})
                opt = DeferredRowAdam(groups, lr=0.0, eps=1e-15, consume_grads=True)
            else:
                groups.append({"params": [p["sh"]], "lr": 2.5e-3, "eps": 1e-15})
                opt = FusedAdam(groups, lr=0.0, eps=1e-15, consume_grads=True)
        dyn = n_views == 1
        fr = FrameGraph(p, cams[:n_views], g, sk, targets[:n_views], factors=factors, img_indices=list(range(n_views)), dynamic=dyn,
                        calib_cams=cams if dyn else None, clear_grads=opt is None,
                        row_catchup=opt.catchup if optim == "deferred" else None)
        stats = [torch.zeros(N, device=dev) for _ in range(3)]
        lib, t_opt = L.lib(), []

        def one(i):
            if dyn:
                k = picks[i]
                fr.set_view(0, cams[k], targets[k], skies[k].detach(), k)
            fr.step(wait=False)
            if opt is None:
                return
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if optim == "deferred":
                opt.step(lists=fr.row_lists())
            else:
                opt.step()
            for v in range(n_views):    # trainers/base.py:279-297 + gaussians/vanilla.py:163-191 for the view's absgrad
                L.check(lib.bds_densify_stats(N, L.ptr(fr.g2d[v][1]), L.ptr(fr.views[v].out["radii"]), W, H, 1, max(W, H), 0, L.ptr(stats[0]),
                                              L.ptr(stats[1]), L.ptr(stats[2]), L.stream()), "bds_densify_stats")
            e1.record()
            t_opt.append((e0, e1))
        for i in range(3):
            one(i)
        torch.cuda.synchronize()
        assert fr.valid()
        t_opt.clear()
        t0 = time.perf_counter()
        for i in range(steps):
            one(3 + i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ok = fr.valid()
        res = {"iters_per_sec": n_views * steps / dt, "ms_per_step": dt / steps * 1e3, "valid": bool(ok)}
        if t_opt:
            res["optimizer_and_stats_ms_per_step"] = sum(a.elapsed_time(b) for a, b in t_opt) / len(t_opt)
        if optim == "deferred":
            res["sh_rows_behind"] = int((opt.state[p["sh"]]["last_step"] < opt._t).sum())
        del fr, opt, p, g
        torch.cuda.empty_cache()
        return res

    for name, (nv, optim) in (("one_view_step", (1, None)), ("train_step_dense_adam", (1, "dense")), ("train_step_deferred_adam", (1, "deferred")),
                              ("train_frame_dense_adam", (V, "dense")), ("train_frame_deferred_adam", (V, "deferred"))):
        try:
            out[name] = variant(nv, optim)
        except Exception as e:   # measurement tooling must never take the bench line down
            out[name] = {"error": f"{type(e).__name__}: {e}"}
    return out


def _free_port():
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def exchange_probe_worker(args):
    """Child process of the default N = 1 run: ONE rank, backend "nccl" (= RCCL), ``dist.force_collectives``: the workload's frame
    without an exchange, with the per-view exchange (mask MAX + compact-row SUM all-reduce between every view's graphs) and with the
    per-frame dense all-reduce -- every collective really issued.  A one-rank all-reduce moves nothing over xGMI: what this measures is
    the exchange's OVERHEAD on a rank (enqueue, union-slot kernels, compact stores + row adds, RCCL's kernel launch), not a fabric."""
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(_free_port()))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
    from bilateral_driving_amd import dist as D
    from bilateral_driving_amd.graph_view import FrameGraph
    D.force_collectives(True)
    wl, N, W, H, yaws, cams, params, grids, skies, targets = build_scene(args, dev, 0)
    V = min(args.views_per_step or len(cams), len(cams))
    names = list(params.keys()) + [f"grid{i}" for i in range(len(grids))]
    out = {"backend": dist.get_backend(), "world": 1, "steps": args.steps}

    def timed(frame):
        for _ in range(3):
            assert frame.step() is True
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                frame.step(wait=False)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / args.steps * 1e3)
        assert frame.valid()
        return sorted(ts)[1]

    def flat_grad():
        return torch.cat([t.grad.reshape(-1) for t in list(params.values()) + grids]).clone()

    frame = FrameGraph(params, cams[:V], grids, skies[:V], targets[:V], factors=wl["factors"], img_indices=list(range(V)))
    out["plain_ms_per_frame"] = timed(frame)
    ref = flat_grad()
    del frame
    for mode, per_view in (("per_view", True), ("per_frame", False)):
        flat = D.FlatGradients(list(params.values()) + grids, sparse_rows=True)
        fx = D.FrameExchange(flat, names, per_view=per_view)
        frame = FrameGraph(params, cams[:V], grids, skies[:V], targets[:V], factors=wl["factors"], img_indices=list(range(V)), exchange=fx)
        ms = timed(frame)
        n1 = D.ISSUED["all_reduce"]
        assert frame.step() is True
        got = flat_grad()
        out[mode] = {"ms_per_frame": ms, "overhead_ms_per_frame": ms - out["plain_ms_per_frame"], "all_reduces_per_frame": D.ISSUED["all_reduce"] - n1,
                     "payload_bytes_per_frame": fx.payload_bytes, "grad_rel_vs_plain": float((got - ref).norm() / ref.norm()),
                     "exchange_rows_capacity": fx.cap}
        del frame, fx, flat
    out["all_reduces_issued"] = D.ISSUED["all_reduce"]
    out["note"] = ("RCCL executed at world size 1: a one-rank all-reduce is a device copy, so this is the exchange's per-rank overhead "
                   "(enqueue + union-slot kernels + compact stores / row adds + RCCL's launches); no xGMI number exists")
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps(out))


def exchange_probe(args):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--exchange-probe-only", "--workload", args.workload, "--scene", args.scene,
           "--steps", str(min(args.steps, 20)), "--row-order", args.row_order, "--lidar-opacity", args.lidar_opacity]
    for flag, val in (("--gaussians", args.gaussians), ("--width", args.width), ("--height", args.height), ("--views-per-step", args.views_per_step)):
        if val is not None:
            cmd += [flag, str(val)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "BDS_FORCE_COLLECTIVES"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.probe_timeout)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if not lines:
            return {"error": f"exit code {r.returncode}: " + (r.stderr.strip().splitlines() or ["no output"])[-1][:300]}
        return json.loads(lines[-1])
    except Exception as e:  # timeout or failure: report it, never hang the benchmark
        return {"error": f"{type(e).__name__} (limit {args.probe_timeout}s)"}


# --dump-outputs: fixed seeded samples of the per-Gaussian rows and of the pixels (2 M Gaussians, six views: ~42 MB in all)
DUMP_ROWS, DUMP_PIXELS, DUMP_LIMIT = 131072, 65536, 64 << 20


def _sample(n, k, seed):
    """``k`` of ``range(n)`` (all of them when n <= k), sorted, drawn by a seeded host generator: the same on every run."""
    if n <= k:
        return torch.arange(n)
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k].sort().values


def dump_outputs(path, views, params, grids, skies, cams):
    """What a caller of the timed step receives, after its last replay: ``views`` = per view (rgb, depth, opacity, loss)."""
    import numpy as np
    N, (H, W) = params["means"].shape[0], views[0][0].shape[:2]
    rows, pix = _sample(N, DUMP_ROWS, 0).to(params["means"].device), _sample(H * W, DUMP_PIXELS, 1).to(views[0][0].device)

    def pixels(t):
        return t.detach().reshape(H * W, -1)[pix]
    out = {"loss": torch.tensor([float(v[3]) for v in views], dtype=torch.float64)}
    for i, name in enumerate(("rgb", "depth", "opacity")):
        out[name] = torch.stack([pixels(v[i]) for v in views])
    out["grad_sky"] = torch.stack([pixels(s.grad) for s in skies])
    out["grad_viewmat"] = torch.stack([c.viewmat.grad.detach() for c in cams])
    for k, p in params.items():
        out[f"grad_{k}"] = p.grad.detach()[rows]
    for i, g in enumerate(grids):
        out[f"grad_grid{i}"] = g.grad.detach()
    arrays = {k: v.cpu().numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32) for k, v in out.items()}
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes"
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, f"{k}.npy"), a)


def main():

    args = parse()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.cpu_baseline_only:
        cpu_baseline_worker(args)
        return
    if args.exchange_probe_only:
        exchange_probe_worker(args)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU, torch.distributed.run on 127.0.0.1)
        import subprocess
        port = _free_port()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs the MI355X (there is no CPU path in the product)"
    # plumbing check on a ONE-GPU box only (scripts / CI): BDS_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and talks through
    # gloo (RCCL refuses two ranks on one device); the numbers of such a run mean nothing
    share = os.environ.get("BDS_BENCH_SHARE_GPU", "0") == "1"
    if share:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # BDS_FORCE_COLLECTIVES=1 at N = 1: a process group of ONE rank over RCCL whose collectives are really issued (dist.force_collectives)
    coll = world > 1 or os.environ.get("BDS_FORCE_COLLECTIVES", "0") == "1"
    if coll:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
        if share:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=dev)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    from bilateral_driving_amd import _lib as L
    from bilateral_driving_amd import harness as Hn
    from bilateral_driving_amd.dist import FlatGradients, FrameExchange

    L.lib()  # fail loudly if libbds.so is missing
    if os.environ.get("BDS_DEBUG_OPTION"):   # kernel A/B hooks (include/bds.h: option 3), measurement sessions only
        L.set_option(3, int(os.environ["BDS_DEBUG_OPTION"]))
    for env, which in (("BDS_PAD_BWD_KB", 1), ("BDS_PAD_FWD_KB", 2), ("BDS_CELLS", 7), ("BDS_SCHED_BINS", 8)):   # (tuning hooks: cap the compositors' resident waves)
        if os.environ.get(env):
            L.set_option(which, int(os.environ[env]))
    wl, N, W, H, yaws, cams, params, grids, skies, targets = build_scene(args, dev, rank)
    V = min(args.views_per_step or len(cams), len(cams))
    factors = wl["factors"]
    dense = bool(args.dense_grads) and not coll
    # param.grad = slices of ONE flat buffer: the backward kernels write the rows of the Gaussians a view sees straight into it,
    # zero_grad clears exactly the rows the previous frame wrote (a view sees ~15 % of the scene); at N > 1 the rows travel in compact
    # per-view exchange buffers (dist.FrameExchange)
    flat = FlatGradients(list(params.values()) + grids, sparse_rows=True)
    fx_names = list(params.keys()) + [f"grid{i}" for i in range(len(grids))]
    # (auto: the per-frame form is built first -- its step(local=True) is one rank's compute time without a second build)
    fx = FrameExchange(flat, fx_names, per_view=args.exchange == "view")

    # (16-px tile, Gaussian) pairs per view = the intersections of the reference's algorithm (SURVEY.md 8d counts bytes per such pair);
    # the fused view builds its lists for larger tiles (fused_view.LIST_TILE) and never materialises them, so they are counted once here
    from bilateral_driving_amd import fused_view as FV
    if args.full or coll:     # (--full: the roofline's pair counts; collectives: the ranks' visibility unions that price the exchange)
        with torch.no_grad():
            infos16 = [Hn.render_view(params, cams[v], grids, v, skies[v], factors=factors, list_tile=16)["info"] for v in range(V)]
            M16 = [i["n_isects"] for i in infos16]
            vis_masks = [(i["radii"].reshape(-1) > 0) for i in infos16] if coll else None
            del infos16
        torch.cuda.synchronize()

    stats = {}
    plan = None
    selfcheck = None
    use_graph = not args.no_graph and not dense
    frame = None
    if use_graph:
        # the views are captured with the roofline kernel bracketed by timing marks (event-record nodes: re-recorded by every replay)
        from bilateral_driving_amd.graph_view import FrameGraph
        L.enable_timers(os.environ.get("BDS_BENCH_NO_TIMERS") != "1", only=("rasterize_bwd",))
        def build_frame(exchange):
            if world > 1 and os.environ.get("BDS_BENCH_FAIL_GRAPH") == "1":     # (plumbing check of the last-resort fallback below)
                raise RuntimeError("forced by BDS_BENCH_FAIL_GRAPH")
            return FrameGraph(params, cams[:V], grids, skies[:V], targets[:V], factors=factors, img_indices=list(range(V)),
                              overlap=not args.no_overlap, exchange=exchange)
        try:
            frame = build_frame(fx)
        except Exception as e:
            # (the per-view exchange puts collectives between captured graphs; should the runtime refuse that on this fabric, the frame
            # that replays exactly as on one GPU + one dense all-reduce still measures the path)
            if not coll:
                raise
            if fx.per_view:
                print(f"bench.py: WARNING: per-view exchange failed to build ({type(e).__name__}: {e}); falling back to --exchange frame", file=sys.stderr)
                torch.cuda.synchronize()
                fx = FrameExchange(flat, fx_names, per_view=False)
                try:
                    frame = build_frame(fx)
                except Exception as e2:
                    e, frame = e2, None
            if frame is None:
                # last resort on a fabric no round could test (no multi-GPU box was ever available): the eager frame loop with the
                # exchange between the views -- slower (one host wait per view), but the N-GPU line exists
                print(f"bench.py: WARNING: the graph-replayed frame failed to build on {world} ranks ({type(e).__name__}: {e}); "
                      "timing the eager frame loop", file=sys.stderr)
                torch.cuda.synchronize()
                fx = FrameExchange(flat, fx_names, per_view=True)
        if coll and args.exchange == "auto" and frame is not None:
            # price the two exchanges from what this job measures: the ranks' unions per view, one rank's frame, the fabric
            from bilateral_driving_amd.dist import measure_busbw, plan_exchange, union_row_counts
            unions = union_row_counts(vis_masks)
            for _ in range(2):      # (the first replay of a captured graph uploads it)
                frame.step(wait=False, local=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                frame.step(wait=False, local=True)
            torch.cuda.synchronize()
            tt = torch.tensor([(time.perf_counter() - t0) / 3], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            busbw = measure_busbw(dev)
            if os.environ.get("BDS_BENCH_ASSUME_BUSBW_GBPS"):   # (plumbing checks on a box without the fabric: price with this instead)
                busbw = float(os.environ["BDS_BENCH_ASSUME_BUSBW_GBPS"]) * 1e9
            plan = plan_exchange(unions, N, fx.row_floats, flat.total - N * fx.row_floats, world, float(tt[0]), busbw)

            def timed_with_collectives(fr):     # ms per frame, max over the ranks: the exchange's enqueue / kernel overhead is in it
                for _ in range(3):                # (a frame that had to grow its lists re-captured itself: collective, every rank alike)
                    fr.step()
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(4):
                    fr.step(wait=False)
                torch.cuda.synchronize()
                t = torch.tensor([(time.perf_counter() - t0) / 4], device=dev, dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                fr.valid()
                return float(t[0]) * 1e3
            # the model prices the wire only; the per-view form also costs ~0.3 ms of enqueue + slot kernels per view on every rank
            # (config.exchange_world1) -- so both forms are built and TIMED with their collectives, and the faster one is kept
            frame_fx, frame_frame = fx, frame
            plan["per_frame_measured_ms"] = timed_with_collectives(frame_frame)
            try:
                fx = FrameExchange(flat, fx_names, per_view=True)
                frame = build_frame(fx)
                plan["per_view_measured_ms"] = timed_with_collectives(frame)
                if os.environ.get("BDS_BENCH_FAIL_PER_VIEW") == "1":   # (plumbing check of the fallback below)
                    raise RuntimeError("forced by BDS_BENCH_FAIL_PER_VIEW")
                plan["model_says_per_view"] = plan["per_view"]
                plan["per_view"] = bool(plan["per_view_measured_ms"] < plan["per_frame_measured_ms"])
                if not plan["per_view"]:
                    del frame
                    fx, frame = frame_fx, frame_frame
                    flat._dirty, flat._clean = None, False
                    for _ in range(2):      # (the gradient buffer's views belong to this frame again)
                        frame.step()
                else:
                    del frame_frame
            except Exception as e:   # (keep the form that already ran)
                print(f"bench.py: WARNING: per-view exchange failed ({type(e).__name__}: {e}); staying with the per-frame all-reduce",
                      file=sys.stderr)
                plan = dict(plan, per_view=False, per_view_failed=f"{type(e).__name__}: {e}")
                fx, frame = frame_fx, frame_frame
                flat._dirty, flat._clean = None, False
        L.enable_timers(False)

    last_views = [None] * V     # (eager driver, --dump-outputs: the outputs of the last step's views)

    def step(s):
        if frame is not None:
            frame.step(wait=False)     # (pipelined: validity is checked once, after the timed region)
            return
        if dense:
            for p in list(params.values()) + grids:
                p.grad = None
        else:
            fx.begin_frame()
        for v in range(V):
            skies[v].grad = None
            cams[v].viewmat.grad = None
            kw = {} if dense else fx.view_kwargs(v)
            # the reference-shaped step: forward, loss, loss.backward() through autograd
            out = Hn.render_view(params, cams[v], grids, v, skies[v], factors=factors, **kw)
            if not dense:
                fx.begin_view(out["info"])
            loss = Hn.training_loss(out, targets[v], grids, grid_grads=None if dense else fx.tail_grads())
            loss.backward()
            if args.dump_outputs:
                last_views[v] = (out["rgb"], out["depth"], out["opacity"], loss)
            if not dense:
                fx.end_view()
            stats.setdefault("M", []).append(out["info"]["n_isects"])
            stats.setdefault("n_vis", []).append(out["info"]["n_visible"])
        if not dense:
            fx.end_frame()

    for s in range(args.warmup):
        step(s)
    torch.cuda.synchronize()
    # inside the timed region only the dominant kernel is bracketed by HIP events (every pair is two more packets on the stream);
    # the per-operator table is taken from a few extra, untimed steps afterwards
    if frame is None:
        L.enable_timers(os.environ.get("BDS_BENCH_NO_TIMERS") != "1", only=("rasterize_bwd",))   # (diagnostic switch)
    # The timed region -- EXACTLY --steps steps between barrier + synchronize on both sides -- is repeated; the median repeat is the
    # reported one (max over ranks per repeat first)
    reps, dom_ms = [], []
    for r in range(max(args.repeats, 1)):
        stats.clear()
        torch.cuda.synchronize()
        if coll:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(args.steps):
            step(args.warmup + r * args.steps + s)
        torch.cuda.synchronize()
        if coll:
            dist.barrier()
        torch.cuda.synchronize()
        reps.append(time.perf_counter() - t0)
        if frame is not None:   # the marks of the repeat's last frame (one pair per view), recorded inside the timed region
            dom_ms += frame.mark_samples("rasterize_bwd")
    if coll:
        t = torch.tensor(reps, device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        reps = [float(x) for x in t.tolist()]
    elapsed = sorted(reps)[len(reps) // 2] if len(reps) % 2 else sorted(reps)[len(reps) // 2 - 1]   # (lower median for even counts)
    if frame is not None:
        assert frame.valid(), "a list outgrew its calibrated capacity during the timed region"
    if args.dump_outputs and rank == 0:
        views = [(vg.rgb, vg.depth, vg.opacity, vg.loss) for vg in frame.views] if frame is not None else last_views
        dump_outputs(args.dump_outputs, views, params, grids, skies[:V], cams[:V])
    last_views[:] = [None] * V
    ms_per_step = elapsed / args.steps * 1e3
    value = world * V * args.steps / elapsed
    result = {
        "metric": "train iters/sec (fwd+bwd) at 2M Gaussians, 6x1920x1080; HBM roofline %",
        "value": value, "unit": "iters/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "repeats": len(reps), "ms_per_step_min": min(reps) / args.steps * 1e3,
        "ms_per_step_max": max(reps) / args.steps * 1e3, "timing": "median of `repeats` timed regions of `steps` steps each",
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"{args.workload}{'' if args.scene == 'ring' else ' on the LIDAR-initialised street scene (harness.lidar_scene, opacity ' + args.lidar_opacity + '), NOT the scene the metric is quoted on'}: "
                               f"{wl['text']}; {N} Gaussians, {len(cams)}-cam ring {W}x{H}, RGB+ED, grids "
                               f"{[list(l) for l in wl['levels']]} factors {list(factors)}, L1+TV loss, camera-pose gradient live; one step = one "
                               f"frame of {V} views per GPU (1 iter = 1 view)",
                   "workload_name": args.workload, "scene": args.scene,
                   "row_order": args.row_order + (" (Morton order of the centres, densify.spatial_order: applied once at load, outside the timed "
                                                  "region; the set of Gaussians is the generator's)" if args.row_order == "spatial" else " (the generator's own order)"),
                   "gaussians": N, "width": W, "height": H, "views": len(cams), "views_per_step": V,
                   "frames_per_sec": value / V, "ms_per_view": ms_per_step / V, "parallelism": f"view-dp{world}",
                   "step_driver": ("hipGraph replay (graph_view.FrameGraph): per view " +
                                   ("two captured graphs (forward + L1/TV loss value | backward), the forwards on a second stream next to "
                                    "the previous view's backward" if not args.no_overlap else "ONE captured graph = forward + L1/TV loss + backward") +
                                   ", device-side list counts, no host wait") if frame is not None else
                                  "autograd (forward, loss, loss.backward())",
                   "gradient_buffer": "dense tensors (autograd accumulation)" if dense else "flat, visible rows only",
                   "allreduce_bytes_per_step": fx.payload_bytes if coll else 0, "allreduce_dense_bytes": flat.nbytes if coll else 0,
                   "exchanges_per_step": fx.n_exchanges if coll else 0,
                   "collectives_forced_at_world1": bool(coll and world == 1),
                   "exchange": None if not coll else dict(mode="view" if fx.per_view else "frame", chosen_by=args.exchange, plan=plan)},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(result))
        if coll:
            dist.destroy_process_group()
        return
    dom_in_situ = None
    if frame is not None:
        cnts = frame.counts()
        Ms, nvs = [c[0] for c in cnts], [c[1] for c in cnts]
        dom_in_situ = (len(dom_ms), sum(dom_ms) / max(len(dom_ms), 1)) if dom_ms else None
        # The same captured graphs once more on ONE stream: the kernel's own duration (in the timed region it shares the GPU with the
        # other stream's kernels; rocprofv3 serialises the streams and reports this figure)
        alone = []
        for _ in range(3):
            frame.step(serial=True)
            torch.cuda.synchronize()
            alone += frame.mark_samples("rasterize_bwd")
        tsum = {"rasterize_bwd": (len(alone), sum(alone) / max(len(alone), 1))} if alone else {}
        # the TIMED path checked at this size, every run: one more replayed frame against one eager frame on the same parameters
        if not coll and os.environ.get("BDS_BENCH_NO_SELFCHECK") != "1":
            from bilateral_driving_amd.selfcheck import frame_against_eager
            try:
                selfcheck = frame_against_eager(frame, params, cams[:V], grids, skies[:V], targets[:V], factors)
            except Exception as e:
                selfcheck = {"ok": False, "error": f"{type(e).__name__}: {e}"}
            if not selfcheck["ok"]:
                print(f"bench.py: ERROR: the replayed frame does not match the eager frame: {selfcheck}", file=sys.stderr)
    else:
        tsum = L.timer_summary()
        Ms, nvs = list(stats["M"]), list(stats["n_vis"])
    # per-operator table
    per_kernel_source = None
    tall = None
    if frame is not None and world == 1 and os.environ.get("BDS_BENCH_EAGER_TABLE") != "1":
        # the timed path itself: the same frame captured once more with timing marks around EVERY operator (event-record nodes; the
        # timed graphs carry them around the roofline kernel only), replayed on one stream
        try:
            L.enable_timers(True)
            marked = FrameGraph(params, cams[:V], grids, skies[:V], targets[:V], factors=factors, img_indices=list(range(V)),
                                overlap=not args.no_overlap)
            L.enable_timers(False)
            acc = {}
            for _ in range(3):
                marked.step(serial=True)
                torch.cuda.synchronize()
                for name in marked.marks:
                    acc.setdefault(name, []).extend(marked.mark_samples(name))
            tall = {k: (len(v), sum(v) / max(len(v), 1)) for k, v in acc.items() if v}
            if os.environ.get("BDS_BENCH_OVERLAP_TABLE") == "1":   # diagnostic: the same marks while the two streams share the GPU
                acc2 = {}
                for _ in range(4):
                    marked.step()
                    torch.cuda.synchronize()
                    for name in marked.marks:
                        acc2.setdefault(name, []).extend(marked.mark_samples(name))
                print("bench.py: operator ms, one stream vs the overlapped frame: " + json.dumps(
                    {k: [round(tall[k][1], 4), round(sum(v) / max(len(v), 1), 4)] for k, v in sorted(acc2.items()) if v and k in tall}), file=sys.stderr)
            per_kernel_source = ("timing marks (event-record nodes) around every operator inside a second capture of the timed frame graphs, "
                                 "replayed on ONE stream after the timed region: rasterize_fwd includes the record pack with the SH colours, "
                                 "bilagrid_fwd the L1 + TV loss; algorithmic bytes: SURVEY.md 8(d) rows at this run's N, n_visible, M, pixels")
            del marked
        except Exception as e:   # (the table is a by-product: never lose the bench line over it)
            L.enable_timers(False)
            print(f"bench.py: WARNING: marked capture failed ({type(e).__name__}: {e}); per-operator table from the eager loop", file=sys.stderr)
            tall = None
    if tall is None:
        # the eager host-count loop with HIP events around every operator (2 untimed frames)
        frame_graph, frame = frame, None
        L.enable_timers(True)
        for s in range(2):
            step(s)
        torch.cuda.synchronize()
        tall = L.timer_summary()
        L.enable_timers(False)
        frame = frame_graph
        per_kernel_source = ("HIP events around every operator of the eager host-count loop, 2 extra frames AFTER the timed region; "
                             "algorithmic bytes: SURVEY.md 8(d) rows at this run's N, n_visible, M, pixels")
    # the replayable frame: ONE capture, every step other cameras / targets / skies / image indices in the slots' static inputs (the
    # reference's loop: a random image per step, tools/train.py:250-283).  Same kernels; the extra work is the input copies (a data
    # loader would write the static tensors directly) and two launches per view that pick / return the image's grids.
    random_its = None
    if rank == 0 and world == 1 and args.random_views and frame is not None:
        try:
            from bilateral_driving_amd.graph_view import FrameGraph
            g2 = torch.Generator().manual_seed(5)
            pool = []
            for k in range(4):      # 4 rigs along the drive, jittered yaws: 4 x V cameras
                pool += Hn.ring_cameras(W, H, yaws_deg=[y + float(torch.rand(1, generator=g2)) * 20.0 - 10.0 for y in yaws], device=dev,
                                        origin=(1.5 * k, 0.0, 0.0))
            pool_t = [torch.rand(H, W, 3, generator=g2).to(dev) for _ in range(4)]
            pool_s = [torch.rand(H, W, 3, generator=g2).to(dev) for _ in range(4)]
            dyn = FrameGraph(params, cams[:V], grids, skies[:V], targets[:V], factors=factors, img_indices=list(range(V)),
                             overlap=not args.no_overlap, dynamic=True, calib_cams=pool)
            picks = torch.randint(0, len(pool), (args.steps + 3, V), generator=g2).tolist()

            def dyn_step(i):
                for v in range(V):
                    k = picks[i][v]
                    dyn.set_view(v, pool[k], pool_t[k % 4], pool_s[(k + 1) % 4], k % len(cams))
                dyn.step(wait=False)
            for i in range(3):
                dyn_step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                dyn_step(3 + i)
            torch.cuda.synchronize()
            random_its = V * args.steps / (time.perf_counter() - t0)
            assert dyn.valid(), "a list outgrew the capacities of the calibration sweep"
            frame = dyn     # (keeps `frame is not None` for the step_driver text below)
        except Exception as e:   # measurement tooling must never take the bench line down
            random_its = f"{type(e).__name__}: {e}"
    # the same frame with the scene's rows in the OTHER order (--row-order): same set of Gaussians, same kernels, same images
    other_order_its, other_order = None, ("given" if args.row_order == "spatial" else "spatial")
    if rank == 0 and world == 1 and args.random_views and frame is not None:
        try:
            from bilateral_driving_amd.graph_view import FrameGraph
            if other_order == "spatial":
                p2 = Hn.reorder_params(params, Hn.spatial_order(params["means"]))
            else:   # undo the Morton order with a fixed shuffle (the generator's own order is a random one)
                p2 = Hn.reorder_params(params, torch.randperm(N, generator=torch.Generator().manual_seed(1)).to(dev))
            fr2 = FrameGraph(p2, cams[:V], grids, skies[:V], targets[:V], factors=factors, img_indices=list(range(V)), overlap=not args.no_overlap)
            for _ in range(3):
                fr2.step(wait=False)
            t2 = []
            for _ in range(max(args.repeats, 1)):     # (timed as the headline is: the median of `repeats` regions of `steps` frames)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fr2.step(wait=False)
                torch.cuda.synchronize()
                t2.append(time.perf_counter() - t0)
            other_order_its = V * args.steps / sorted(t2)[(len(t2) - 1) // 2]
            assert fr2.valid()
            del fr2, p2
        except Exception as e:   # measurement tooling must never take the bench line down
            other_order_its = f"{type(e).__name__}: {e}"
    # the drop-in path (reference-signature operators chained by autograd: projection, SH, isect_tiles, rasterize_to_pixels,
    # bilagrid_transform -- what `gsplat.rasterization(...)` + the module `forward` cost a trainer that changes nothing else)
    # api_path_iters_per_sec: that sequence starting at the Gaussian class's own get_gaussians with marshalling.install (deferred
    # activations -> the raw one-view node); api_path_eager_iters_per_sec: with the class's eager activations + dense SH pass (the
    # figure of rounds 3-4)
    api_its = api_eager_its = None
    if rank == 0 and world == 1 and not args.no_api_path:
        def api_loop(view):
            for v in range(V):
                view(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for v in range(V):
                view(v)
            torch.cuda.synchronize()
            return V / (time.perf_counter() - t0)
        try:
            Hn.FUSED = False
            def api_view(v):
                for t in list(params.values()) + grids + [skies[v], cams[v].viewmat]:
                    t.grad = None
                Hn.training_loss(Hn.render_view(params, cams[v], grids, v, skies[v], factors=factors), targets[v], grids).backward()
            api_eager_its = api_loop(api_view)
        except Exception as e:   # measurement tooling must never take the bench line down
            api_eager_its = f"{type(e).__name__}: {e}"
        finally:
            Hn.FUSED = True
        try:
            from bilateral_driving_amd import marshalling as Marsh
            model = Hn.VanillaModel(params)
            Marsh.install(Hn.VanillaModel)
            def model_view(v):
                for t in model.parameters() + grids + [skies[v], cams[v].viewmat]:
                    t.grad = None
                Hn.training_loss(Hn.render_view_model(model, cams[v], grids, v, skies[v], factors=factors), targets[v], grids).backward()
            api_its = api_loop(model_view)
            del model
        except Exception as e:
            api_its = f"{type(e).__name__}: {e}"
        finally:
            Marsh.uninstall(Hn.VanillaModel)
    cadence = None
    if rank == 0 and world == 1 and not args.no_train_cadence and frame is not None:
        del frame
        frame = True     # (only `frame is not None` is read below)
        torch.cuda.empty_cache()
        try:
            cadence = train_cadence(args, params, cams, grids, skies, targets, factors, V, dev)
        except Exception as e:   # measurement tooling must never take the bench line down
            cadence = {"error": f"{type(e).__name__}: {e}"}

    # ---- roofline of the dominant kernel: composite backward (K8).  Algorithmic bytes per launch: 44 B/isect read +
    # 28 B/pixel read + 48 B/isect gradient write.
    list_pairs_mean = sum(Ms) / len(Ms)          # pairs the tile stage emitted and sorted (list tiles of FV.LIST_TILE px)
    M_mean, nv_mean, P = sum(M16) / len(M16), sum(nvs) / len(nvs), W * H
    dom = "rasterize_bwd"   # (the composite backward: its block is always reported, as `roofline_composite`)
    calls, mean_ms = tsum.get(dom, (0, float("nan")))
    alg_bytes = 92.0 * M_mean + 28.0 * P
    achieved = alg_bytes / (mean_ms * 1e-3) / 1e9 if calls else float("nan")
    kname = L.rasterize_kernel_name(True, 4, True, FV.LIST_TILE)   # the library names the kernel its launch switches select
    counters_apply = args.scene == "ring"     # (the committed counter passes are of the ring scene)
    traffic, traffic_src = _newest_profile("_pmc.json", kname, "hbm_bytes_per_launch_corrected", args.workload) if counters_apply else (None, None)
    traffic_error = None
    if traffic is None and counters_apply:   # loud, not silent: a renamed kernel or a missing counter pass must not pass as "no traffic figure"
        traffic_error = f"no profiles/*_pmc.json holds counters of `{kname}`: re-run scripts/gpu_round.sh <tag> and scripts/summarize_profile.py"
        print("bench.py: WARNING: " + traffic_error, file=sys.stderr)
    roofline = {"bound": "hbm", "binding_roof": "valu issue (see `valu`): the kernel moves 0.15x its algorithmic bytes through HBM",
                "operator": dom, "kernel": "bds::" + kname, "achieved": achieved, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
                "frac_traffic": None if traffic is None or not calls else traffic / (mean_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": mean_ms, "launches_timed": calls,
                "avg_launch_ms_in_timed_region": None if dom_in_situ is None else dom_in_situ[1],
                "note": "achieved = algorithmic bytes (92 B per (16-px tile, Gaussian) pair of the reference's lists + 28 B/pixel, SURVEY.md 8d) "
                        "/ the kernel's HIP-event launch time.  frac is that NOMINAL figure; frac_traffic = HBM bytes the counters saw / "
                        "time / peak -- the kernel is bound by VALU issue, not by HBM (SURVEY.md 7, hard part 2).  avg_launch_ms: timing "
                        "marks inside the captured graphs, replayed on one stream right after the timed region (what rocprofv3, which "
                        "serialises the streams, reports); avg_launch_ms_in_timed_region: the same marks during the timed steps, where "
                        "the kernel shares the GPU with the next view's forward on the second stream"}
    if traffic_error:
        roofline["traffic_error"] = traffic_error
    # the binding roof of K7/K8: vector instructions per visited (tile, Gaussian) pair
    valu = None
    ring_headline = args.scene == "ring" and N == wl["gaussians"]     # (the committed counter passes are of this scene)
    if rank == 0 and not args.no_pair_stats and args.workload == "headline" and (ring_headline or args.scene == "lidar"):
        try:
            ps = _pair_stats(N, W, H, params if args.scene == "lidar" else None)
            insts, src = _newest_profile("_sq_counters.json", kname, "SQ_INSTS_VALU") if ring_headline else (None, None)
            if insts is None and ring_headline:
                print(f"bench.py: WARNING: no profiles/*_sq_counters.json holds `{kname}`", file=sys.stderr)
            busy, _ = _newest_profile("_sq_counters.json", kname, "valu_busy_frac") if ring_headline else (None, None)
            valu = {"listed_pairs": ps["isects_listed"], "visited_pairs": ps["pairs_visited"], "pixel_blends": ps["pixel_blends"],
                    "visited_over_listed": ps["pairs_visited"] / max(ps["isects_listed"], 1),
                    "pixels_per_visited_pair": ps["mean_pixels_per_visited_pair"], "strips_per_visited_pair": ps["mean_strips_per_visited_pair"],
                    "pairs_view": 0, "valu_insts_per_launch": insts, "valu_insts_per_pair": None if insts is None else insts / ps["pairs_visited"],
                    "valu_frac": busy, "counter_source": src,
                    # per pair: ~35 vector ops per blending pixel (4 exp2, 4 rcp, fma-class rest); everything else is overhead
                    "useful_frac": None if insts is None else min(1.0, 35.0 * ps["pixel_blends"] / 64.0 / insts),
                    "note": "visited = (tile, Gaussian) pairs that some pixel blends (early termination + alpha cut leave ~1 in 10 of the "
                            "listed pairs); valu_frac = 4 * SQ_ACTIVE_INST_VALU / (1024 SIMDs * kernel cycles) from the committed rocprofv3 "
                            "counter pass: the kernel issues a vector instruction in (nearly) every issue slot it has"}
        except Exception as e:  # measurement tooling must never take the bench line down
            valu = {"error": f"{type(e).__name__}: {e}"}

    # ---- per-operator table: HIP-event time + algorithmic bytes of SURVEY.md 8(d) at this run's N, n_visible, M, pixels
    K = params["sh"].shape[1]
    alg = {
        "project_fwd": 96.0 * N,                                   # K2 + activations: 68 + 28 B/Gaussian
        "sh_fwd": 216.0 * nv_mean + 32.0 * N,                      # K1 on the visible rows + 32 B/Gaussian of radii / depth / colour rows
        "isect_prepare": 36.0 * N + 64.0 * nv_mean,                # K4 count + depth sort of the visible entries (4 x 16 B)
        "isect_build": (4.0 + 16.0 + 4.0 + 8.0) * M_mean,          # K4 emit + K5 tile sort (packed: 2 x 8 B) + list values + K6 offsets
        #                                                            (bytes of the reference's 16-px pairs; the coarse lists move fewer)
        "rasterize_fwd": 44.0 * M_mean + 24.0 * P + 96.0 * nv_mean,  # K7 (+ packing the visible splat records: 48 B gathered + 48 B written)
        "bilagrid_fwd": 44.0 * P,                                  # K9-K11: 40 B/pixel + 4 B/pixel expected depth
        "bilagrid_bwd": 72.0 * P,                                  # K12: 68 B/pixel + 4 B/pixel depth gradient
        "rasterize_bwd": alg_bytes,                                # K8
        "sh_bwd": (64.0 + 24.0 + K * 12.0) * nv_mean,              # K1 bwd, visible rows: gradient record + mean / colour rows + 192 B row
        "project_bwd": (64.0 + 44.0 + 44.0 + 16.0) * nv_mean,      # K3, visible rows: record + 11 parameter floats in + 11 out + 2-D gradients
    }
    if per_kernel_source.startswith("timing marks"):   # (what the marks of the device-count form bracket)
        alg["rasterize_fwd"] += 216.0 * nv_mean           # SH colours evaluated by the record pack (K1 on the visible rows)
        alg["bilagrid_fwd"] += 36.0 * P                   # L1 + TV loss on the launch: target in, loss gradient out
    # entries whose SURVEY 8(d) byte count describes the REFERENCE's formulation rather than what this kernel moves: their GB/s figure
    # is a speed-up over that formulation, not an achieved bandwidth
    nominal = {"isect_build": "bytes of the reference's 16-px (tile, Gaussian) pairs; the fused view lists 64-px pairs (config.list_pairs_mean)",
               "rasterize_fwd": "bytes of the reference's 16-px pairs; ~1 in 10 is ever reached by a pixel (valu.visited_over_listed) and the records stay in L2",
               "rasterize_bwd": "bytes of the reference's 16-px pairs (92 B each); the counters see 0.15x of them (roofline_composite.traffic)",
               "project_fwd": "counts all N rows; the outputs of the ~85 % culled Gaussians are never read again",
               "isect_prepare": "36 B x all N + 64 B x visible: the stage is launch-latency bound, not bandwidth bound",
               "sh_fwd": "32 B x all N of radii / depth / colour rows + the visible coefficient rows"}
    per_kernel = {}
    for k, (c, ms) in sorted(tall.items()):
        e = {"ms": round(ms, 4)}
        if k in alg and ms > 0:
            e["algorithmic_bytes"] = alg[k]
            e["algorithmic_GBps"] = round(alg[k] / (ms * 1e-3) / 1e9, 1)
            if k in nominal:
                e["nominal"], e["nominal_reason"] = True, nominal[k]
        per_kernel[k] = e
    # ---- the roofline block follows the workload's ACTUAL dominant operator: the longest entry of the per-operator table (the marked
    # capture of the timed frame).  The compositor's block stays as `roofline_composite`.
    roofline_composite = roofline
    timed_ops = {k: v["ms"] for k, v in per_kernel.items() if k in alg and v["ms"] > 0}
    dom_op = max(timed_ops, key=timed_ops.get) if timed_ops else dom
    if dom_op != dom:
        from bilateral_driving_amd.bilagrid import _levels_struct
        lv = _levels_struct([g[0:1] for g in grids], None, factors)
        op_kernels = {"bilagrid_bwd": lambda: L.bilagrid_kernel_names(lv, H, W, True),
                      "bilagrid_fwd": lambda: L.bilagrid_kernel_names(lv, H, W, False, per_kernel_source.startswith("timing marks")),
                      "rasterize_fwd": lambda: [L.rasterize_kernel_name(False, 4, True, FV.LIST_TILE)]}
        knames = op_kernels[dom_op]() if dom_op in op_kernels else []
        tr, srcs = 0.0, []
        for kn in knames:   # counter traffic of every kernel the operator launches (None as soon as one is missing)
            t_k, src_k = _newest_profile("_pmc.json", kn, "hbm_bytes_per_launch_corrected", args.workload) if counters_apply else (None, None)
            if t_k is None:
                tr = None
                print(f"bench.py: WARNING: no profiles/*_pmc.json of workload {args.workload} holds counters of `{kn}`", file=sys.stderr)
                break
            tr += t_k
            srcs.append(src_k)
        if not knames:
            tr = None
        ms_dom = timed_ops[dom_op]
        ach = alg[dom_op] / (ms_dom * 1e-3) / 1e9
        roofline = {"bound": "hbm", "operator": dom_op, "kernel": ", ".join("bds::" + k for k in knames) or None, "achieved": ach,
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": tr,
                    "traffic_source": sorted(set(srcs)) or None,
                    "frac_traffic": None if tr is None else tr / (ms_dom * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "algorithmic_bytes_per_launch": alg[dom_op], "avg_launch_ms": ms_dom,
                    "note": "the longest operator of this workload's per_kernel table (timing marks inside the captured frame); achieved = its "
                            "SURVEY.md 8(d) algorithmic bytes / that time; traffic = HBM bytes of all its kernels from the committed counter "
                            "passes of this workload.  The composite backward's block: `roofline_composite`"}

    result["config"].update({
        f"{other_order}_row_order_iters_per_sec": other_order_its, "api_path_iters_per_sec": api_its, "api_path_eager_iters_per_sec": api_eager_its,
        "n_visible_mean": nv_mean, "isects_mean": M_mean, "list_tile": FV.LIST_TILE, "list_pairs_mean": list_pairs_mean,
        "random_views_iters_per_sec": random_its,
        "train_cadence": cadence,
        "one_view_step_iters_per_sec": None if not cadence or "error" in cadence.get("one_view_step", {"error": 1}) else cadence["one_view_step"]["iters_per_sec"],
        "train_step_iters_per_sec": None if not cadence or "error" in cadence.get("train_step_deferred_adam", {"error": 1}) else cadence["train_step_deferred_adam"]["iters_per_sec"],
        "train_step_dense_adam_iters_per_sec": None if not cadence or "error" in cadence.get("train_step_dense_adam", {"error": 1}) else cadence["train_step_dense_adam"]["iters_per_sec"]})
    result.update({
        "frame_valu_issue_frac": _frame_valu_issue(ms_per_step / V, args.workload) if (counters_apply and args.workload == "headline" and N == wl["gaussians"]) else None,
        "roofline": roofline,
        "roofline_composite": roofline_composite,
        "valu": valu,
        "per_kernel": per_kernel,
        "per_kernel_source": per_kernel_source,
        "selfcheck": selfcheck,
    })
    if rank == 0 and not coll and not args.no_exchange_probe:
        torch.cuda.empty_cache()
        probe = exchange_probe(args)
        result["config"]["exchange_world1"] = probe
        # (per frame of this workload, on ONE rank, every collective issued over RCCL at world size 1: what the exchange costs before a
        #  byte crosses xGMI)
        result["config"]["exchange_overhead_ms"] = None if "error" in probe else {
            "per_view": probe["per_view"]["overhead_ms_per_frame"], "per_frame": probe["per_frame"]["overhead_ms_per_frame"]}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(args)
    if rank == 0:
        print(json.dumps(result))
    if coll:
        dist.destroy_process_group()
    if selfcheck is not None and not selfcheck["ok"]:
        sys.exit(3)      # a fast frame whose results differ from the eager frame's is not a result


if __name__ == "__main__":
    main()
