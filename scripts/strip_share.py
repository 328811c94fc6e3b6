#!/usr/bin/env python3
"""Price of a per-strip early exit in the compositors (measurement tooling): lane pixel q of the one-wave-per-tile kernels is the 16 x 4
strip of rows 4q..4q+3, and a strip is finished for good behind its own deepest blended entry, `strip_last[q]` = max of last_ids over the
strip.  Per tile the walk covers the entries [start, tile_last]; the (entry, strip) combinations a scalar `gidx > strip_last[q]` test
could skip are sum_q (tile_last - max(strip_last[q], start - 1)), out of 4 x (tile_last - start + 1).  16-px lists: the entries a tile
walks behind the candidate filter.  Runs on the GPU with torch ops only.

    python scripts/strip_share.py [--scene ring|lidar] [--view 0]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bilateral_driving_amd import _lib as L  # noqa: E402
from bilateral_driving_amd import gs_ops as ops  # noqa: E402
from bilateral_driving_amd import harness as Hn  # noqa: E402


def strip_share(p, W, H, view=0):
    dev = p["means"].device
    cam = Hn.ring_cameras(W, H, device=dev)[view]
    N = p["means"].shape[0]
    with torch.no_grad():
        radii, m2, dep, con, _ = ops.fully_fused_projection(p["means"], p["quats"], torch.exp(p["log_scales"]), cam.viewmat[None], cam.K[None],
                                                            W, H, near_plane=0.1)
        op = torch.sigmoid(p["opacity_logits"])[None].contiguous()
        tw, th = math.ceil(W / 16), math.ceil(H / 16)
        _, _, fids, offs = ops.isect_tiles(m2, radii, dep, 16, tw, th, want_isect_ids=False, conics=con, opacities=op)
        M = fids.numel()
        col = torch.rand(1, N, 3, device=dev)
        render, alphas = torch.empty(1, H, W, 3, device=dev), torch.empty(1, H, W, 1, device=dev)
        last = torch.zeros(1, H, W, dtype=torch.int32, device=dev)
        rec = torch.empty(N, L.SPLAT_RECORD_FLOATS, device=dev)
        L.check(L.lib().bds_splat_pack(N, None, 3, None, L.ptr(m2), L.ptr(con), L.ptr(col), L.ptr(op), None, L.ptr(rec), None, None, 0, None,
                                       L.stream()), "pack")
        L.check(L.lib().bds_rasterize_fwd(1, N, M, None, 3, L.ptr(rec), None, W, H, 16, 16, tw, th, L.ptr(offs), L.ptr(fids), L.ptr(render),
                                          L.ptr(alphas), None, L.ptr(last), None, 0, 0, 0, L.stream()), "fwd")
        torch.cuda.synchronize()
        n_tiles = tw * th
        start = offs.reshape(-1).long()
        end = torch.cat([start[1:], torch.tensor([M], device=dev)])
        Hp, Wp = th * 16, tw * 16
        lid = torch.full((Hp, Wp), -1, dtype=torch.long, device=dev)
        lid[:H, :W] = last[0].long()
        # [tile, strip q, 64 pixels of the strip]
        lid_s = lid.reshape(th, 4, 4, tw, 16).permute(0, 3, 1, 2, 4).reshape(n_tiles, 4, 64)
        s_last = lid_s.max(dim=2).values                                   # [tile, 4]
        t_last = s_last.max(dim=1).values
        live = (end > start) & (t_last >= start)
        walked = torch.where(live, t_last - start + 1, torch.zeros_like(t_last))
        s_walk = torch.where(live[:, None], (s_last - start[:, None] + 1).clamp(min=0), torch.zeros_like(s_last))
        skippable = (walked[:, None] - s_walk).clamp(min=0)
        tot, skip = int(walked.sum()) * 4, int(skippable.sum())
        return dict(width=W, height=H, view=view, gaussians=N, isects_listed=M, tiles=n_tiles, tiles_live=int(live.sum()),
                    entries_walked=int(walked.sum()), walked_mean=float(walked.float().mean()), walked_max=int(walked.max()),
                    entry_strips=tot, entry_strips_skippable=skip, share=skip / max(tot, 1),
                    strips_never_blending=int(((s_walk == 0) & live[:, None]).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("ring", "lidar"), default="ring")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--view", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    p = Hn.lidar_scene(1_000_000, seed=0, device=dev) if a.scene == "lidar" else Hn.synthetic_scene(2_000_000, seed=0, device=dev)
    out = strip_share({k: v.detach() for k, v in p.items()}, a.width, a.height, a.view)
    out["scene"] = a.scene
    print(json.dumps(out))


if __name__ == "__main__":
    main()
