#!/usr/bin/env python3
"""Golden vectors for the SMPL nodes' skinning-weight field by IMPORTING THE REFERENCE: models/modules.py
VoxelDeformer._query_weights_smpl (:1197-1226), called unbound on a stand-in ``self`` that carries only ``resolution_dhw``.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_voxel_weights.py        (build machine only: needs the reference tree)

pytorch3d has no build for this machine either, so ``modules.knn_points`` is bound to the brute force below: float32 coordinate
differences, ``(dx*dx + dy*dy) + dz*dz``, a stable sort (equal values keep the order of their rows).  Everything after the search
-- the clamp, the inverse-distance blend through the [B,N,K,J] gather, the thirty relaxation steps -- is the reference's own code in
float32.  The blend before the relaxation is the same method's return with the module's ``range`` bound to an empty one.

Inputs: B = 2 humans, a 4 x 8 x 8 grid of voxel centres (x fastest, as VoxelDeformer.__init__ lays them) over a box 1.2 x the
vertices', V = 97 vertices, J = 5 weights per vertex that sum to 1.  The file holds arrays only."""
import builtins
import collections
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.gen_golden_neural_modules import import_reference  # noqa: E402  (the stubbing of tensorly / pytorch3d / nvdiffrast)

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "knn_points")
B, V, J, DHW, K = 2, 97, 5, (4, 8, 8), 30
_KNN = collections.namedtuple("KNN", "dists idx knn")


def brute_force_knn_points(p1, p2, K=1, **_):
    diff = p1[:, :, None, :] - p2[:, None, :, :]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    v, i = torch.sort(d2, dim=-1, stable=True)
    return _KNN(v[..., :K].contiguous(), i[..., :K].contiguous(), None)


def main():
    M = import_reference()
    M.knn_points = brute_force_knn_points
    g = torch.Generator().manual_seed(53)
    verts = torch.randn(B, V, 3, generator=g) * torch.tensor([0.25, 0.45, 0.15]) + torch.randn(B, 1, 3, generator=g)
    weights = torch.softmax(torch.randn(B, V, J, generator=g) * 2.0, dim=-1)
    d, h, w = DHW
    lo, hi = verts.min(1).values, verts.max(1).values
    centre, half = 0.5 * (lo + hi), 0.5 * 1.2 * (hi - lo)
    unit = torch.stack(torch.meshgrid(torch.linspace(-1, 1, d), torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij"), -1)
    unit = unit.flip(-1).reshape(1, -1, 3)                                  # (x, y, z) per voxel, x fastest
    x = centre[:, None, :] + unit * half[:, None, :]
    stand_in = types.SimpleNamespace(resolution_dhw=DHW)
    fn = M.VoxelDeformer._query_weights_smpl
    field = fn(stand_in, x.clone(), verts.clone(), weights.clone())
    M.range = lambda *_: builtins.range(0)
    try:
        blend = fn(stand_in, x.clone(), verts.clone(), weights.clone())
    finally:
        del M.range
    blend = blend.reshape(B, J, -1).permute(0, 2, 1).contiguous()           # back to [B, d*h*w, J]
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "voxel_weights_f32.npz")
    np.savez_compressed(path, x=x.numpy(), verts=verts.numpy(), weights=weights.numpy(), resolution_dhw=np.array(DHW, dtype=np.int64),
                        K=np.array(K, dtype=np.int64), blend=blend.numpy(), field=field.numpy())
    print(path, os.path.getsize(path), "bytes; field", tuple(field.shape), "sum over J", float(field.sum(1).min()), float(field.sum(1).max()))


if __name__ == "__main__":
    main()
