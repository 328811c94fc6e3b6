#!/usr/bin/env python3
"""Times the batched cross search (bds_cross_knn) on the MI355X at the reference's two shapes, each against the same result formed
by torch on the same card -- chunked coordinate differences, ``topk``, a gather: the only stand-in for pytorch3d that runs here.

    python scripts/knn_points_time.py [--out profiles/knn_points_time.json]
    python scripts/knn_points_time.py --step field_hip          (one step, e.g. under rocprofv3 --kernel-trace --stats)

  field      the skinning field's search with its blend: B = 8 humans, P1 = 16*64*64 voxel centres, P2 = 6890 vertices, K = 30,
             J = 24 (models/modules.py:1199-1206); peak device memory is recorded both ways
  knn_8/32   update_knn's search: B = 8 and 32 clouds of 6890 points against themselves, K = 3 (models/nodes/smpl.py:186)

Every step runs in a child process of its own under ``timeout -k 10``; the first one that fails ends the run."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STEPS = ("field_hip", "field_torch", "knn_8_hip", "knn_8_torch", "knn_32_hip", "knn_32_torch")
STEP_SECONDS = 150
CLAMP = (0.0001, 1.0)


def _clouds(B, P1, P2, J, self_search):
    import torch
    g = torch.Generator().manual_seed(B)
    verts = torch.randn(B, P2, 3, generator=g) * torch.tensor([0.25, 0.5, 0.15])
    if self_search:
        return verts.cuda(), verts.cuda(), None
    side = (16, 64, 64)
    grid = torch.stack(torch.meshgrid(*[torch.linspace(-1, 1, s) for s in side], indexing="ij"), -1).flip(-1).reshape(1, -1, 3)
    x = grid * (1.2 * verts.abs().amax(1, keepdim=True))
    feat = torch.softmax(torch.randn(B, P2, J, generator=g) * 2, -1)
    assert x.shape[1] == P1
    return x.cuda(), verts.cuda(), feat.cuda()


def _torch_search(p1, p2, K, chunk):
    import torch
    d, i = [], []
    for s in range(0, p1.shape[1], chunk):
        diff = p1[:, s:s + chunk, None, :] - p2[:, None, :, :]
        d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        v, j = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
        d.append(v)
        i.append(j)
    return torch.cat(d, 1), torch.cat(i, 1)


def _torch_field(x, verts, feat, K, chunk):
    import torch
    out = []
    for s in range(0, x.shape[1], chunk):
        d2, idx = _torch_search(x[:, s:s + chunk], verts, K, chunk)
        w = 1.0 / d2.sqrt().clamp_(*CLAMP)
        w = w / w.sum(-1, keepdim=True)
        near = feat.unsqueeze(2).expand(-1, -1, K, -1).gather(1, idx.unsqueeze(-1).expand(-1, -1, -1, feat.shape[-1]))
        out.append((w[..., None] * near).sum(-2))
    return torch.cat(out, 1)


def step(name, reps=5, warmup=2):
    import torch
    from bilateral_driving_amd import p3d
    which, how = name.rsplit("_", 1)
    if which == "field":
        B, P1, P2, K, J = 8, 16 * 64 * 64, 6890, 30, 24
        x, verts, feat = _clouds(B, P1, P2, J, False)
        fn = (lambda: p3d.knn_blend(x, verts, feat, K, CLAMP)) if how == "hip" else (lambda: _torch_field(x, verts, feat, K, 4096))
    else:
        B, P1, P2, K, J = int(which.split("_")[1]), 6890, 6890, 3, 0
        x, verts, _ = _clouds(B, P1, P2, J, True)
        fn = (lambda: p3d.knn_points(x, verts, K=K, return_nn=False)[:2]) if how == "hip" else (lambda: _torch_search(x, verts, K, 1024))
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    marks[0].record()
    for r in range(reps):
        out = fn()
        marks[r + 1].record()
    torch.cuda.synchronize()
    ms = sorted(marks[r].elapsed_time(marks[r + 1]) for r in range(reps))
    first = out if torch.is_tensor(out) else out[0]
    rec = {"step": name, "B": B, "P1": P1, "P2": P2, "K": K, "J": J, "ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1],
           "reps": reps, "peak_bytes_above_inputs": int(torch.cuda.max_memory_allocated() - base),
           "checksum": float(first.double().sum()), "device": torch.cuda.get_device_name()}
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.step:
        step(a.step)
        return 0
    results = []
    for name in STEPS:
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name],
                           capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            print(f"{name}: exit status {r.returncode} after {time.time() - t0:.0f} s; nothing more is started\n{r.stderr[-2000:]}", flush=True)
            return r.returncode or 1
        results.append(json.loads(lines[-1][len("RESULT "):]))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
