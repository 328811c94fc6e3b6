"""Numpy restatement of the batched cross search (csrc/knn_cross.hip, bilateral_driving_amd/p3d.py) and of the skinning field made
from it: brute force, once in float64 and once in float32 with the kernel's roundings, a stable argsort on the value so that equal
values keep the order of their rows, pytorch3d's padding, the inverse-distance blend and the relaxation in float64, and the named
clouds of the tests as functions of a seed.  Test infrastructure only."""
import functools

import numpy as np


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def values(p1, p2, norm, dtype):
    """[P1,P2] values of one cloud pair in ``dtype``: float32 rounds every operation on its own, in the kernel's order (numpy neither
    fuses nor reorders elementwise operations); float64 is the reference the bounds are stated against."""
    a, b = np.asarray(p1, dtype=dtype), np.asarray(p2, dtype=dtype)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    if norm == 2:
        return (dx * dx + dy * dy) + dz * dz
    return (np.abs(dx) + np.abs(dy)) + np.abs(dz)


def search(p1, p2, K, norm=2, len1=None, len2=None, dtype=np.float32):
    """p1 [B,P1,3], p2 [B,P2,3] -> (dists [B,P1,K] ``dtype``, idx [B,P1,K] int64): ascending by (value, row), the first len2[b] rows of
    p2[b] only; rows at or beyond len1[b] and slots at or beyond len2[b] hold zeros."""
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dists, idx = np.zeros((B, P1, K), dtype=dtype), np.zeros((B, P1, K), dtype=np.int64)
    for b in range(B):
        n1 = P1 if len1 is None else int(min(max(len1[b], 0), P1))
        n2 = P2 if len2 is None else int(min(max(len2[b], 0), P2))
        k = min(K, n2)
        if n1 == 0 or k == 0:
            continue
        v = values(p1[b, :n1], p2[b, :n2], norm, dtype)
        order = np.argsort(v, axis=1, kind="stable")[:, :k]
        dists[b, :n1, :k] = np.take_along_axis(v, order, axis=1)
        idx[b, :n1, :k] = order
    return dists, idx


def search_fast(p1, p2, K, norm=2, len1=None, len2=None, dtype=np.float32):
    """``search`` without sorting whole rows, for the GPU tests' many cases: the K smallest of the keys (value bits, row) by a
    partition, then sorted.  A non-negative float orders as its bit pattern does, so for float32 the 64-bit key (bits << 32 | row)
    carries the (value, row) order exactly; for float64 only the sorted VALUES are formed (idx is returned as None) -- that is all
    the float64 bound needs.  tests/test_knn_points_cpu.py holds it equal to ``search`` on every named cloud."""
    B, P1, P2 = p1.shape[0], p1.shape[1], p2.shape[1]
    dists = np.zeros((B, P1, K), dtype=dtype)
    idx = np.zeros((B, P1, K), dtype=np.int64) if dtype == np.float32 else None
    for b in range(B):
        n1 = P1 if len1 is None else int(min(max(len1[b], 0), P1))
        n2 = P2 if len2 is None else int(min(max(len2[b], 0), P2))
        k = min(K, n2)
        if n1 == 0 or k == 0:
            continue
        v = values(p1[b, :n1], p2[b, :n2], norm, dtype)
        if dtype == np.float32:
            key = (v.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n2, dtype=np.uint64)[None, :]
            key = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
            dists[b, :n1, :k] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
            idx[b, :n1, :k] = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        else:
            dists[b, :n1, :k] = np.sort(np.partition(v, k - 1, axis=1)[:, :k], axis=1)
    return dists, idx


def slots(B, P1, P2, K, len1=None, len2=None):
    """[B,P1,K] bool: the slots that hold a neighbour."""
    n1 = np.full(B, P1) if len1 is None else np.clip(np.asarray(len1), 0, P1)
    n2 = np.full(B, P2) if len2 is None else np.clip(np.asarray(len2), 0, P2)
    return (np.arange(P1)[None, :, None] < n1[:, None, None]) & (np.arange(K)[None, None, :] < n2[:, None, None])


# ---- the blend and the field -----------------------------------------------------------------------------------------------------------
def blend(p1, p2, feat, idx, valid, clamp):
    """float64 [B,P1,J]: sum_k (w_k / sum w) feat[idx_k] over the valid slots, w_k = 1 / clip(distance_k), the distances taken again in
    float64 from the float32 coordinates for the rows ``idx`` (the float32 search's choice: the blend is a function of the chosen
    rows, and a float64 search may choose others where two candidates are within rounding of each other)."""
    p1, p2, feat = np.asarray(p1, np.float64), np.asarray(p2, np.float64), np.asarray(feat, np.float64)
    B, P1, K = idx.shape
    out = np.zeros((B, P1, feat.shape[2]))
    for b in range(B):
        if p2.shape[1] == 0:
            continue
        nn = p2[b][idx[b]]                                        # [P1,K,3]
        d = np.sqrt(((p1[b][:, None, :] - nn) ** 2).sum(-1))
        w = np.where(valid[b], 1.0 / np.clip(d, clamp[0], clamp[1]), 0.0)
        s = w.sum(-1, keepdims=True)
        w = np.divide(w, s, out=np.zeros_like(w), where=s > 0)
        out[b] = (w[:, :, None] * feat[b][idx[b]]).sum(1)
    return out


def relax(weights, iters=30, keep=0.7):
    """models/modules.py:1212-1225 in float64 on [B,J,d,h,w]."""
    w = np.array(weights, dtype=np.float64)
    for _ in range(iters):
        mean = (w[:, :, 2:, 1:-1, 1:-1] + w[:, :, :-2, 1:-1, 1:-1] + w[:, :, 1:-1, 2:, 1:-1] + w[:, :, 1:-1, :-2, 1:-1]
                + w[:, :, 1:-1, 1:-1, 2:] + w[:, :, 1:-1, 1:-1, :-2]) / 6.0
        w[:, :, 1:-1, 1:-1, 1:-1] = (w[:, :, 1:-1, 1:-1, 1:-1] - mean) * keep + mean
        w = w / w.sum(1, keepdims=True)
    return w


def field(x, verts, weights, dhw, K=30, clamp=(0.0001, 1.0), iters=30):
    """-> (blend [B,P1,J], field [B,J,d,h,w]) in float64, from the float32 search's rows."""
    _, idx = search(x, verts, K, 2, dtype=np.float32)
    bl = blend(x, verts, weights, idx, slots(x.shape[0], x.shape[1], verts.shape[1], K), clamp)
    B, J = x.shape[0], weights.shape[2]
    return bl, relax(bl.transpose(0, 2, 1).reshape(B, J, *dhw), iters)


# ---- the named clouds -------------------------------------------------------------------------------------------------------------------
def uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def lattice(n, seed):
    """The first n of 11^3 lattice points at pitch 0.25, shuffled: every d2 is exact in float32 and every list is full of ties."""
    g = np.arange(11, dtype=np.float32) * np.float32(0.25)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return pts[np.random.default_rng(seed).permutation(len(pts))[:n]].copy()


def duplicates(n, seed):
    """Every point of a small cloud several times over."""
    rng = np.random.default_rng(seed)
    base = rng.random((max(n // 5, 1), 3), dtype=np.float32)
    return base[rng.integers(0, len(base), n)].copy()


def planar(n, seed):
    p = uniform(n, seed)
    p[:, 2] = np.float32(0.5)
    return p


def far_offset(n, seed):
    """Coordinates near 2000 with spacing 0.01: the differences cancel eleven bits."""
    rng = np.random.default_rng(seed)
    return (np.float32(2000.0) + rng.integers(0, 64, (n, 3)).astype(np.float32) * np.float32(0.01)).astype(np.float32)


def distinct(n, seed):
    """A cloud without duplicates (for a search against itself): a shuffled lattice, jittered by less than half its pitch."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    g = np.arange(side, dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)[:n]]
    return (pts + rng.random((n, 3), dtype=np.float32) * np.float32(0.4)).astype(np.float32)


CLOUDS = {"uniform": uniform, "lattice": lattice, "duplicates": duplicates, "planar": planar, "far_offset": far_offset}


@functools.lru_cache(maxsize=None)
def cloud(name, n, seed):
    """[n,3] float32, read-only (shared among the tests)."""
    out = (distinct if name == "distinct" else CLOUDS[name])(n, seed)
    out.setflags(write=False)
    return out


def batch(name, B, P1, P2, seed=0):
    """p1 [B,P1,3], p2 [B,P2,3] of the named cloud, every batch entry its own draw."""
    p1 = np.stack([cloud(name, P1, seed + 2 * b) for b in range(B)]) if P1 else np.zeros((B, 0, 3), np.float32)
    p2 = np.stack([cloud(name, P2, seed + 2 * b + 1) for b in range(B)]) if P2 else np.zeros((B, 0, 3), np.float32)
    return p1, p2


def within(got, ref64, rel):
    """Largest |got - ref64| / ref64 over the non-zero reference entries, and whether ``got`` is exactly 0 where the reference is."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    zero = ref64 == 0
    err = float((np.abs(got - ref64)[~zero] / ref64[~zero]).max(initial=0.0))
    return err, bool(np.all(got[zero] == 0)), err <= rel
