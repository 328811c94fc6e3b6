#!/usr/bin/env python3
"""Time of the fused deformation network (csrc/deform.hip) against the same module run as framework ops (the hook off:
``deform.framework_forward`` over the module's own parameters, the expression of models/modules.py:925-1012), for
ConditionalDeformNetwork (embed 16, quat on, scale off: DeformableNodes) and DeformNetwork (all heads), forward only and
forward + backward (gradients of the parameters and of cond, as the trainer needs them).

    python scripts/deform_time.py [--out profiles/deform_time.json] [--sizes 5000,50000,200000,1000000]
    python scripts/deform_time.py --profile N      (a few fused forward + backward calls, for rocprofv3 --kernel-trace --stats)

Device events around each call, warm-up, A and B alternated over the repeats; the median of the repeats is reported.  Workspace
bytes from bds_deform_bwd_temp_bytes; FLOPs from the layer shapes (kernel share of the 157.3 TFLOP/s FP32 matrix peak)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import deform  # noqa: E402

PEAK_TFLOPS = 157.3


def macs_per_point(E, n_heads):
    K0 = 84 + E
    return K0 * 256 + 6 * 256 * 256 + (K0 + 256) * 256 + n_heads * 256


def make(kind):
    if kind == "cond":
        m = deform.ConditionalDeformNetwork(D=8, W=256, input_ch=3, embed_dim=16, x_multires=10, t_multires=10, deform_quat=True,
                                            deform_scale=False)
        return m.cuda(), 16, (m.gaussian_warp, m.gaussian_rotation, None)
    m = deform.DeformNetwork(D=8, W=256, input_ch=3, x_multires=10, t_multires=10)
    return m.cuda(), 0, (m.gaussian_warp, m.gaussian_rotation, m.gaussian_scaling)


def case(kind, N, backward):
    m, E, heads = make(kind)
    g = torch.Generator().manual_seed(N)
    x = (torch.rand(N, 3, generator=g) * 2 - 1).cuda()
    t = torch.full((N, 1), 0.3).cuda()
    c = (torch.randn(N, E, generator=g) * 0.5).cuda().requires_grad_(True) if E else None
    ws = [torch.randn(N, k, generator=g).cuda() for k in (3, 4, 3)]
    args = (x, t, c) if E else (x, t)

    def fused():
        m.zero_grad(set_to_none=True)
        if not backward:
            with torch.no_grad():
                return m(*args)
        outs = m(*args)
        sum((o * w).sum() for o, w in zip(outs, ws) if o is not None).backward()

    def framework():
        m.zero_grad(set_to_none=True)
        if not backward:
            with torch.no_grad():
                return deform.framework_forward(m.linear, heads, x, t, c, 10, 10)
        outs = deform.framework_forward(m.linear, heads, x, t, c, 10, 10)
        sum((o * w).sum() for o, w in zip(outs, ws) if o is not None).backward()
    return fused, framework, E, sum(h.out_features for h in heads if h is not None)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def measure(kind, N, backward, reps):
    fused, framework, E, head_rows = case(kind, N, backward)
    for _ in range(2):
        fused(); framework()
    torch.cuda.synchronize()
    tf, tw = [], []
    for r in range(reps):       # alternated: A B, B A, ...
        if r % 2 == 0:
            tf.append(event_ms(fused)); tw.append(event_ms(framework))
        else:
            tw.append(event_ms(framework)); tf.append(event_ms(fused))
    flop = 2.0 * macs_per_point(E, head_rows) * N * (3 if backward else 1)
    mf, mw = statistics.median(tf), statistics.median(tw)
    return {"net": kind, "N": N, "pass": "fwd+bwd" if backward else "fwd", "fused_ms": round(mf, 4), "framework_ms": round(mw, 4),
            "speedup": round(mw / mf, 3), "fused_ms_min": round(min(tf), 4), "framework_ms_min": round(min(tw), 4),
            "flop": flop, "fused_tflops": round(flop / mf / 1e9, 2), "fused_share_of_peak": round(flop / mf / 1e9 / PEAK_TFLOPS, 3),
            "bwd_temp_bytes": int(L.lib().bds_deform_bwd_temp_bytes(N, E)) if backward else 0, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="5000,50000,200000,1000000")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    if a.profile:
        for kind in ("cond", "plain"):
            fused, _, _, _ = case(kind, a.profile, True)
            for _ in range(5):
                fused()
        torch.cuda.synchronize()
        return
    rows = []
    for kind in ("cond", "plain"):
        for N in [int(s) for s in a.sizes.split(",")]:
            for backward in (False, True):
                r = measure(kind, N, backward, a.reps)
                rows.append(r)
                print(json.dumps(r), flush=True)
    res = {"device": torch.cuda.get_device_name(), "peak_fp32_matrix_tflops": PEAK_TFLOPS,
           "macs_per_point": {"cond": macs_per_point(16, 7), "plain": macs_per_point(0, 10)}, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
