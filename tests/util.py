"""Shared helpers for the tests: synthetic scenes, error metrics, the host-math shim loader, hipcc's kernel resource report and the
header's declarations."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import torch

from bilateral_driving_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_scene(N, W, H, seed=0, dtype=torch.float32, device="cpu", fov_deg=70.0, spread=1.0):
    """Small synthetic scene in front of one camera (OpenCV convention, z forward)."""
    g = torch.Generator().manual_seed(seed)
    fx = 0.5 * W / np.tan(np.deg2rad(fov_deg) / 2)
    z = torch.rand(N, generator=g, dtype=torch.float64) * 8 + 2.0
    x = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * 1.4 * z * (W / fx) * spread
    y = (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * 1.4 * z * (H / fx) * spread
    means = torch.stack([x, y, z], -1)
    quats = torch.randn(N, 4, generator=g, dtype=torch.float64)
    # per-axis pixel-space sigma log-uniform in [0.7, W/8] px -> world scale at depth z
    spx = torch.exp(torch.rand(N, 3, generator=g, dtype=torch.float64) * np.log((W / 8) / 0.7) + np.log(0.7))
    scales = spx * z[:, None] / fx
    opac = torch.sigmoid(torch.randn(N, generator=g, dtype=torch.float64) * 1.5)
    colors = torch.rand(N, 3, generator=g, dtype=torch.float64)
    # camera: small rotation + translation so that viewmat is not the identity
    ang = 0.1
    Rz = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=torch.float64)
    Ry = torch.tensor([[np.cos(0.05), 0, np.sin(0.05)], [0, 1, 0], [-np.sin(0.05), 0, np.cos(0.05)]], dtype=torch.float64)
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, :3] = Rz @ Ry
    vm[:3, 3] = torch.tensor([0.1, -0.05, 0.2], dtype=torch.float64)
    # move the Gaussians into world space so that they land in front of the camera
    means = (means - vm[:3, 3]) @ vm[:3, :3]
    K = torch.tensor([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=torch.float64)
    out = dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors, viewmats=vm[None], Ks=K[None])
    return {k: v.to(dtype).to(device) for k, v in out.items()}


def aa_oracle(p, viewmats, Ks, W, H, mode, backgrounds=None, sh_degree=None, near_plane=0.01, probes=None):
    """float64 (or float32) antialiased rasterization, camera by camera, from the oracle's stages -> render, alphas, unstable, radii,
    compensations ([C,N] each)."""
    import math
    from oracle import gs_oracle as _G
    C = viewmats.shape[0]
    tw, th = math.ceil(W / 16), math.ceil(H / 16)
    rs, als, uns, rad, cps = [], [], [], [], []
    for c in range(C):
        radii, m2, dep, con, comp = _G.project(p["means"], p["quats"], p["scales"], viewmats[c], Ks[c], W, H, near_plane=near_plane,
                                              calc_compensations=True)
        if sh_degree is None:
            col = p["colors"]
        else:
            cam_pos = torch.linalg.inv(viewmats[c])[:3, 3]
            col = _G.spherical_harmonics(sh_degree, p["means"] - cam_pos, p["colors"], masks=radii > 0)
            col = torch.clamp_min(col + 0.5, 0.0)
        if mode in ("RGB+D", "RGB+ED"):
            col = torch.cat([col, dep[:, None]], -1)
        tpg, iids, fids = _G.isect_tiles(m2, radii, dep, 16, tw, th)
        offs = _G.isect_offset_encode(iids, tw, th)
        bg = None if backgrounds is None else torch.cat([backgrounds[c], backgrounds.new_zeros(col.shape[-1] - 3)])
        probe = None
        if probes is not None:
            probe = []
            probes.append(probe)
        r, a, _, un = _G.rasterize_to_pixels(m2, con, col, p["opacities"] * comp, W, H, 16, offs, fids, bg, return_unstable=True,
                                            absgrad_probe=probe)
        if mode == "RGB+ED":
            r = torch.cat([r[..., :-1], r[..., -1:] / a.clamp(min=1e-10)], -1)
        rs.append(r)
        als.append(a)
        uns.append(un)
        rad.append(radii)
        cps.append(comp.detach())
    return torch.stack(rs), torch.stack(als), torch.stack(uns), torch.stack(rad), torch.stack(cps)


def grad_errors(got, ref, floor=1e-3):
    """(norm-relative error, largest and 99th-percentile ELEMENT-wise relative error over the elements whose reference magnitude is
    above `floor` x the largest one -- below that a gradient entry is a sum of cancelling terms and its relative error says nothing)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    nrm = float((got - ref).norm() / ref.norm().clamp(min=1e-300))
    big = ref.abs() > floor * ref.abs().max()
    if not bool(big.any()):
        return nrm, 0.0, 0.0
    e = ((got - ref).abs() / ref.abs().clamp(min=1e-300))[big]
    return nrm, float(e.max()), float(torch.quantile(e, 0.99)) if e.numel() < 16_000_000 else float(e.kthvalue(int(0.99 * e.numel())).values)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp(min=1e-12))


def build_shim(stem=""):
    """Build (hipcc, host side only) and load tests/hostmath_<stem>_shim.hip, a test-only shim around the kernels' HD math; rebuilt
    when the shim or one of the kernels' headers is newer than the library."""
    name = f"hostmath_{stem}_shim" if stem else "hostmath_shim"
    src = os.path.join(ROOT, "tests", name + ".hip")
    so = os.path.join(ROOT, "tests", "_build", f"lib{name}.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    deps = [src] + [os.path.join(B.CSRC, f) for f in os.listdir(B.CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call([B._hipcc(), f"--offload-arch={B.ARCH}", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", tmp])
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@functools.lru_cache(maxsize=None)
def hostmath():
    """The shim around the projection's and the bilateral grid's HD math (tests/hostmath_shim.hip)."""
    return build_shim()


@functools.lru_cache(maxsize=None)
def kernel_resources(src):
    """hipcc's resource report (-Rpass-analysis=kernel-resource-usage) of csrc/<src> under the product's build flags:
    {mangled kernel name after _ZN3bds<digits>: {remark: int}}.  Cross-compiles, needs no GPU; one compile per file and session."""
    cmd = [B._hipcc(), f"--offload-arch={B.ARCH}", *B.FLAGS, *B.EXTRA_FLAGS.get(src, []), "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(B.CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: _ZN3bds\d+(\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def short_name(mangled):
    """``lidar_boxes_kernelILi2EEvl...`` -> ``lidar_boxes_kernel<2>``: the kernel's name with its first template argument where that
    is a bool or a one-digit int, without its parameter types."""
    m = re.match(r"(\w+?kernel)(?:IL[bi](\d)E)?", mangled)
    return m.group(1) + (f"<{m.group(2)}>" if m.group(2) is not None else "")


_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


@functools.lru_cache(maxsize=None)
def header():
    """include/bds.h without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bds.h")).read(), flags=re.S)


@functools.lru_cache(maxsize=None)
def declared_signatures():
    """{entry: (return ctype, [argument ctypes])} of every function include/bds.h declares.  Scalars are their ctypes type; every
    pointer and ``bds_stream_t`` is ``c_void_p`` (a ``const char *`` result: ``c_char_p``)."""
    def ctype(a):
        if "*" in a or a.startswith("bds_stream_t"):
            return ctypes.c_void_p
        return _SCALARS[a.split()[0]]
    out = {}
    for m in re.finditer(r"\n((?:const\s+)?\w+\s*\*?)\s*(bds_\w+)\s*\(([^)]*)\)\s*;", header()):
        ret, args = " ".join(m.group(1).split()), [a.strip() for a in m.group(3).split(",")]
        out[m.group(2)] = (ctypes.c_char_p if ret == "const char *" else ctype(ret), [] if args == ["void"] else [ctype(a) for a in args])
    return out


def fptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)
