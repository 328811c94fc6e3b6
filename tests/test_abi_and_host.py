"""CPU-only checks of the boundary: libbds.so builds for gfx950, loads, and exports every symbol that
include/bds.h declares; the product refuses to run without a GPU (no CPU fallback); host-side logic."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.util import declared_signatures, header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libpath():
    from bilateral_driving_amd import build
    return build.build()


def _declared_symbols():
    return sorted(set(re.findall(r"\b(bds_[a-z0-9_]+)\s*\(", header())))


def test_header_and_library_symbols_match_abi_7(libpath):
    names = _declared_symbols()
    assert len(names) >= 19
    h = ctypes.CDLL(libpath)
    for n in names:
        assert hasattr(h, n), f"{n} declared in include/bds.h but not exported by libbds.so"
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "-W", libpath], capture_output=True, text=True, check=True).stdout
    rows = [line.split() for line in out.splitlines()]    # Num: Value Size Type Bind Vis Ndx Name
    exported = {r[7] for r in rows if len(r) >= 8 and r[7].startswith("bds_") and r[6] != "UND"}
    assert len(exported) >= 19
    assert not exported - set(names), f"exported by libbds.so but not declared in include/bds.h: {sorted(exported - set(names))}"
    h.bds_abi_version.restype = ctypes.c_int
    from bilateral_driving_amd import _lib as _L
    assert h.bds_abi_version() == _L.ABI_VERSION == 7
    h.bds_strerror.restype = ctypes.c_char_p
    assert b"workspace" in h.bds_strerror(-2)


def test_binding_table_matches_header(libpath):
    from bilateral_driving_amd import _lib
    assert sorted(_lib.EXPORTS) == _declared_symbols()
    _lib.lib()  # sets argtypes for every symbol; raises if one is missing


def test_every_binding_signature_matches_the_header(libpath):
    """Every entry of the hand-written table against include/bds.h: result and scalar arguments exactly; a pointer or a
    ``bds_stream_t`` of the header is any ctypes pointer type (device addresses go as ``c_void_p``, host arrays as ``POINTER(...)``)."""
    from bilateral_driving_amd import _lib

    def is_pointer(t):
        return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)
    decl, lib = declared_signatures(), _lib.lib()
    assert sorted(decl) == sorted(_lib._SIGS) and len(decl) >= 127
    for name, (res, argtypes) in _lib._SIGS.items():
        ret, args = decl[name]
        assert res is ret, (name, res, ret)
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        for i, (got, want) in enumerate(zip(argtypes, args)):
            assert is_pointer(got) if want is ctypes.c_void_p else got is want, (name, i, got, want)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(argtypes), name


def test_library_is_gfx950_only(libpath):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", libpath], capture_output=True, text=True).stdout
    blob = open(libpath, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_80", b"sm_90"):
        assert other not in blob, other


def test_argument_validation_without_gpu(libpath):
    """EINVAL paths return before any launch, so they can be exercised on a CPU-only box."""
    from bilateral_driving_amd import _lib
    h = _lib.lib()
    assert h.bds_sh_fwd(10, 16, 7, None, None, None, None, None) == -1        # degree > 3
    assert h.bds_sh_fwd(0, 16, 3, None, None, None, None, None) == 0          # empty input is fine
    fwd_tail = (None, None, None, None, None, None, None, 0, 0, 0, None)   # isect_offsets .. last_ids, tile_order, split_*, stream
    assert h.bds_rasterize_fwd(1, 10, 0, None, 5, None, None, 64, 64, 16, 16, 4, 4, *fwd_tail) == -1    # CH = 5
    assert h.bds_rasterize_fwd(1, 10, 0, None, 3, None, None, 64, 64, 8, 8, 8, 8, *fwd_tail) == -1     # tile size 8
    assert h.bds_rasterize_fwd(1, 10, 0, None, 3, None, None, 64, 64, 16, 24, 4, 4, *fwd_tail) == -1   # list tile not a multiple of 16
    assert h.bds_splat_pack(0, None, 4, None, None, None, None, None, None, None, None, None, 0, None, None) == 0
    assert h.bds_splat_pack(5, None, 2, None, None, None, None, None, None, None, None, None, 0, None, None) == -1
    assert h.bds_sh_view_bwd_list(0, None, None, 16, 3, None, None, None, 0, None, None, None, None, 0, None) == 0
    assert h.bds_sh_view_bwd_list(4, None, None, 16, 3, None, None, None, 0, None, None, None, None, 0, None) == -1               # null list
    pack_sh_tail = (None,) * 11 + (0, None, None)    # coeffs .. zero_tail, zero_tail_floats, schedule, stream
    assert h.bds_splat_pack_sh(0, None, None, 16, 3, None, None, *pack_sh_tail) == 0
    assert h.bds_splat_pack_sh(4, None, None, 16, 3, None, None, *pack_sh_tail) == -1   # null list
    assert h.bds_splat_pack_sh(4, None, None, 15, 3, None, None, *pack_sh_tail) == -1   # K < 16 bases
    # combinations the merged entries refuse (every other argument acceptable: p stands for any 16-byte aligned device address)
    p = 4096
    img = (64, 64, 16, 16, 4, 4, p, p, p, p, p, p)     # W .. tile_h, isect_offsets, flatten, render, alphas, t_final, last_ids
    assert h.bds_rasterize_fwd(1, 10, 0, p, 3, p, None, *img, None, 0, 0, 0, None) == -1        # M_dev with capacity 0
    assert h.bds_rasterize_fwd(1, 10, 5, None, 3, p, None, *img, p, 0, 0, 0, None) == -1        # host count with a tile_order
    assert h.bds_rasterize_fwd(1, 10, 5, None, 4, p, None, *img, None, 64, 8, 0, None) == -1    # host count with split_len
    grad = (64, 64, 16, 16, 4, 4, p, p, p, p, p, p, p, p, 0)   # W .. tile_h, isect_offsets .. last_ids, v_render, v_alphas, v_records, absgrad
    assert h.bds_rasterize_bwd(1, 10, 0, p, 3, p, None, *grad, None, 0, 0, 0, None) == -1       # M_dev with capacity 0
    assert h.bds_rasterize_bwd(1, 10, 5, None, 4, p, None, *grad, p, 64, 8, 0, None) == -1      # host count with split_len
    assert h.bds_sh_view_bwd_list(4, None, p, 16, 3, p, p, p, 0, p, p, p, p, 0, None) == -1     # v_coeffs_rest together with row_map
    # the tile stage's folded entries: mixed modes, and the requirements of each mode that are checked before any launch
    cnt = (ctypes.c_int64 * 3)()
    prep = (1, 1000, p, p, p, p, p, 16, 4, 4, p, p, 1 << 30)    # C, N, means2d .. opacities, tile_size, tile_w, tile_h, tiles_per_gauss, ws, ws_bytes
    assert h.bds_isect_prepare(*prep, 100, 100, cnt, p, 1, None) == -1      # an event together with capacities
    assert h.bds_isect_prepare(*prep, 100, -1, cnt, None, 1, None) == -1    # exactly one capacity negative
    assert h.bds_isect_prepare(*prep, -1, 100, cnt, None, 1, None) == -1
    assert h.bds_isect_prepare(*prep, -1, -1, None, p, 1, None) == -1       # asynchronous form without counts
    assert h.bds_isect_prepare(*prep, -1, -1, None, None, 1, None) == -1    # synchronous form without counts
    assert h.bds_isect_prepare(1, 0, *prep[2:], 100, 100, cnt, None, 1, None) == -1    # device-count form with C*N == 0
    assert h.bds_isect_prepare(1, 0, *prep[2:], -1, -1, cnt, None, 1, None) == 0 and list(cnt[:2]) == [0, 0]     # (host counts: empty input is fine)
    build = (p, p, p, p, p, 16, 4, 4, p, 1 << 30, p, 1 << 30)   # means2d .. opacities, tile_size, tile_w, tile_h, ws, ws_bytes, ws2, ws2_bytes
    assert h.bds_isect_build(1, 1000, 0, 100, *build, None, p, p, None, 1, 1, None) == -1      # device counts with capacity 0
    assert h.bds_isect_build(1, 1000, 100, 0, *build, None, p, p, None, 1, 1, None) == -1
    assert h.bds_isect_build(1, 1000, 100, 100, *build, p, p, p, None, 1, 0, None) == -1       # isect_ids with device counts
    assert h.bds_isect_build(1, 1000, 100, 100, *build, None, p, p, p, 1, 1, None) == -1       # visible_ids with device counts
    assert h.bds_isect_prepare_workspace_bytes(1, 1000) > 5 * 4000
    assert h.bds_isect_build_workspace_bytes(1, 1000, 50000) > 3 * 4 * 50000
    lv = (_lib.BdsLevel * 1)()
    lv[0].gx, lv[0].gy, lv[0].gl, lv[0].factor, lv[0].n_avg = 8, 8, 4, 2, 1
    assert h.bds_bilagrid_ms_workspace_bytes(1, lv, 64, 64) >= 2 * 32 * 32 * 48  # low-res maps + their gradients
    assert h.bds_bilagrid_ms_workspace_bytes(0, lv, 64, 64) == 0
    # the colour transform's folded entries: `channels` selects the form, and every mix of the forms is refused
    lv[0].grid = p
    ms, bufs = (1, lv, 64, 64), (p, 1 << 30)     # nlevels .. W; ws, ws_bytes
    no_loss = (None, 0, None, None, 0.0, None, 0, None)     # target, tv_nlevels, tv_levels, tv_weights, v_loss, loss_out, loss_slots, v_rgb_out
    maps = (ctypes.c_void_p * 1)(p)
    fwd = h.bds_bilagrid_ms_fwd       # .., channels, in, alpha, sky, ws, ws_bytes, rgb_out, depth_out, affine_out, <loss>, stream
    assert fwd(*ms, 5, p, p, None, *bufs, p, p, None, *no_loss, None) == -1          # channels 5
    assert fwd(*ms, 3, p, None, None, *bufs, p, p, None, *no_loss, None) == -1       # channels 3 with depth_out
    assert fwd(*ms, 3, p, None, None, *bufs, p, None, None, p, 0, None, None, 1.0, p, 64, p, None) == -1     # channels 3 with target
    assert fwd(*ms, 4, p, None, None, *bufs, p, p, None, *no_loss, None) == -1       # channels 4 without alpha
    assert fwd(*ms, 4, p, p, None, *bufs, p, None, None, *no_loss, None) == -1       # channels 4 without depth_out
    assert fwd(*ms, 4, p, p, None, *bufs, p, p, maps, *no_loss, None) == -1          # channels 4 with affine_out
    assert fwd(*ms, 4, p, p, None, *bufs, p, p, None, p, 0, None, None, 1.0, None, 64, p, None) == -1        # target without loss_out
    assert fwd(*ms, 4, p, p, None, *bufs, p, p, None, p, 0, None, None, 1.0, p, 64, None, None) == -1        # target without v_rgb_out
    assert fwd(*ms, 4, p, p, None, *bufs, p, p, None, p, 0, None, None, 1.0, p, 48, p, None) == -1           # loss_slots not a power of two
    assert fwd(*ms, 4, p, p, None, *bufs, p, p, None, p + 4, 0, None, None, 1.0, p, 64, p, None) == -1       # misaligned target
    bwd = h.bds_bilagrid_ms_bwd       # .., channels, in, alpha, sky, ws, ws_bytes, v_rgb_out, v_depth, v_opacity, v_in, v_alpha, v_sky, defer, stream
    assert bwd(*ms, 5, p, p, None, *bufs, p, None, None, p, p, None, 0, None) == -1          # channels 5
    assert bwd(*ms, 3, p, None, None, *bufs, p, p, None, p, None, None, 0, None) == -1       # channels 3 with v_depth
    assert bwd(*ms, 3, p, None, None, *bufs, p, None, p, p, None, None, 0, None) == -1       # channels 3 with v_opacity
    assert bwd(*ms, 3, p, None, None, *bufs, p, None, None, p, None, None, 1, None) == -1    # channels 3 with defer
    assert bwd(*ms, 4, p, None, None, *bufs, p, None, None, p, p, None, 0, None) == -1       # channels 4 without alpha
    assert bwd(*ms, 4, p, p, None, *bufs, p, None, None, p, None, None, 0, None) == -1       # channels 4 without v_alpha
    assert bwd(*ms, 4, p, p, None, *bufs, p, None, None, p, p, None, 1, None) == -1          # defer with v_alpha
    assert bwd(*ms, 4, p, p, p, *bufs, p, None, None, p, None, p, 1, None) == -1             # defer with v_sky
    assert bwd(*ms, 4, p, p, None, *bufs, p, p, None, p, None, None, 1, None) == -1          # defer with v_depth
    assert h.bds_bilagrid_ms_bwd_deferrable(0, lv, 64, 64) == 0                              # (the query answers 0, not an error)
    lv[0].n_avg = 2      # a level averaged over two grids is not deferrable
    assert h.bds_bilagrid_ms_bwd_deferrable(*ms) == 0
    assert bwd(*ms, 4, p, p, None, *bufs, p, None, None, p, None, None, 1, None) == -1
    # Adam's one entry: n_rows, width, grad_stride, param .. exp_avg_sq, lr .. weight_decay, step, consume, stream
    adam = (p, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    assert h.bds_adam_step(10, -1, 0, *adam, 0, None) == -1      # width -1
    assert h.bds_adam_step(10, 4, 3, *adam, 0, None) == -1       # grad_stride < width
    assert h.bds_adam_step(0, 0, 0, *adam, 1, None) == 0         # empty tensors are fine, contiguous and by rows
    assert h.bds_adam_step(0, 4, 16, *adam, 0, None) == 0


def test_no_cpu_fallback():
    from bilateral_driving_amd import _lib
    import bilateral_driving_amd.gs_ops as ops
    import bilateral_driving_amd.bilagrid as B
    with pytest.raises(_lib.BdsError):
        ops.spherical_harmonics(3, torch.randn(4, 3), torch.randn(4, 16, 3))
    with pytest.raises(_lib.BdsError):
        ops.fully_fused_projection(torch.randn(4, 3), torch.randn(4, 4), torch.rand(4, 3), torch.eye(4)[None], torch.eye(3)[None], 8, 8)
    with pytest.raises(_lib.BdsError):
        B.bilagrid_transform(torch.rand(8, 8, 3), [torch.zeros(12, 1, 2, 2)], [1])
    with pytest.raises(_lib.BdsError):
        B.total_variation_loss(torch.zeros(1, 12, 2, 2, 2))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "bilateral_driving_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, os.path.join(dp, f)


def test_dropin_import_surfaces():
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "bilateral_driving_amd", "dropin") + os.pathsep + ROOT)
    code = ("from gsplat.rendering import rasterization\n"
            "from gsplat.cuda_legacy._wrapper import num_sh_bases\n"
            "from gsplat.cuda_legacy._torch_impl import quat_to_rotmat\n"
            "from gsplat.cuda._wrapper import spherical_harmonics\n"
            "from bilateral.lib_bilagrid import BilateralGrid, color_correct, slice, total_variation_loss, NeuralBilateralGrid, slice_feature\n"
            "import torch\n"
            "assert num_sh_bases(3) == 16\n"
            "R = quat_to_rotmat(torch.tensor([[2.0, 0, 0, 0]]))\n"
            "assert torch.allclose(R[0], torch.eye(3))\n"
            "g = BilateralGrid(3, 4, 5, 2)\n"
            "assert g.grids.shape == (3, 12, 2, 5, 4) and list(g.state_dict()) == ['grids', 'rgb2gray_weight']\n"
            "assert float(g.grids[1, 0].min()) == 1.0 and float(g.grids[1, 1].abs().max()) == 0.0 and float(g.grids[2, 5].min()) == 1.0\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_quat_to_rotmat_matches_oracle():
    sys.path.insert(0, os.path.join(ROOT, "bilateral_driving_amd", "dropin"))
    try:
        from gsplat.cuda_legacy._torch_impl import quat_to_rotmat
    finally:
        sys.path.pop(0)
    from oracle import gs_oracle as G
    q = torch.randn(50, 4, dtype=torch.float64)
    assert (quat_to_rotmat(q) - G.quat_to_rotmat(q)).abs().max() < 1e-14


def test_saved_input_tensor_identity_for_absgrad():
    """The .absgrad contract relies on autograd handing back the SAME tensor object that was passed in."""
    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.save_for_backward(x)
            return x * 2

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            x.absgrad = g.abs()
            return g * 2
    a = torch.randn(5, requires_grad=True)
    mid = a * 1.0
    meta = {"means2d": mid}
    F.apply(mid).sum().backward()
    assert hasattr(meta["means2d"], "absgrad")


def test_scene_generator_shapes():
    from bilateral_driving_amd import harness as Hn
    p = Hn.synthetic_scene(1000, seed=0)
    assert p["means"].shape == (1000, 3) and p["sh"].shape == (1000, 16, 3) and p["quats"].shape == (1000, 4)
    r = p["means"][:, :2].norm(dim=-1)
    assert float(r.min()) >= 2.0 - 1e-4 and float(r.max()) <= 80.0 + 1e-3
    cams = Hn.ring_cameras(1920, 1080)
    assert len(cams) == 6
    for c in cams:
        R = c.viewmat[:3, :3]
        assert torch.allclose(R @ R.T, torch.eye(3), atol=1e-6) and abs(float(torch.linalg.det(R)) - 1) < 1e-6
    # camera 0 looks down +x: a point on +x projects to the principal point
    pc = cams[0].viewmat[:3, :3] @ torch.tensor([10.0, 0, 0]) + cams[0].viewmat[:3, 3]
    assert torch.allclose(pc, torch.tensor([0.0, 0.0, 10.0]), atol=1e-6)
    g = Hn.make_grids(4)
    assert [tuple(x.shape) for x in g] == [(4, 12, 1, 2, 2), (4, 12, 2, 4, 4), (4, 12, 4, 8, 8)]


def test_reference_modules_import_against_the_dropin_packages():
    """The import surface that the reference's hot-path modules (models/gaussians/basics.py, vanilla.py, models/modules.py) take
    from `gsplat` / `bilateral` / `nvdiffrast` -- every import statement, pinned in tests/golden/reference_dropin_imports.json by
    oracle/gen_golden_reference_imports.py -- resolves against this repo's drop-in packages to the product's functions
    (SURVEY.md 8b)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bilateral_driving_amd", "dropin"), ROOT]))
    code = ("import importlib, json, sys\n"
            "fixture = json.load(open(sys.argv[1]))\n"
            "ns = {}\n"
            "for e in fixture['imports']:\n"
            "    mod, bound = importlib.import_module(e['module']), ns.setdefault(e['file'], {})\n"
            "    if 'alias' in e:\n"
            "        bound[e['alias']] = mod\n"
            "        assert e['attributes'] and all(hasattr(mod, a) for a in e['attributes']), e\n"
            "    else:\n"
            "        bound.update({n: getattr(mod, n) for n in e['names']})\n"
            "B, M = ns['models/gaussians/basics.py'], ns['models/modules.py']\n"
            "import bilateral_driving_amd.rendering as R, bilateral_driving_amd.gs_ops as O, bilateral_driving_amd.bilagrid as G\n"
            "assert B['rasterization'] is R.rasterization and B['spherical_harmonics'] is O.spherical_harmonics\n"
            "assert M['BilateralGrid'] is G.BilateralGrid and M['slice'] is G.slice and M['total_variation_loss'] is G.total_variation_loss\n"
            "import bilateral_driving_amd.envlight as E\n"
            "assert M['dr'].texture.__module__ == 'nvdiffrast.torch' and M['dr'].cubemap_sample is E.cubemap_sample\n"
            "print('ok')\n")
    fixture = os.path.join(ROOT, "tests", "golden", "reference_dropin_imports.json")
    r = subprocess.run([sys.executable, "-c", code, fixture], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_neural_modules_refuse_cpu_tensors():
    """No CPU fallback behind the module mirrors either: the feature slice underneath raises."""
    import torch
    from bilateral_driving_amd import _lib as L
    from bilateral_driving_amd.modules import NeuralBilateralAffineTransform
    mod = NeuralBilateralAffineTransform("Affine", 2, 4, 4, 2, feature_dim=8, hidden_dim=16, device="cpu")
    with pytest.raises(L.BdsError):
        mod(torch.rand(5, 6, 3), {"img_idx": 0})


def test_sky_and_colour_correct_refuse_cpu_tensors():
    import torch
    from bilateral_driving_amd import _lib as L
    from bilateral_driving_amd.colorcorrect import color_correct
    from bilateral_driving_amd.envlight import EnvLight, cubemap_sample
    with pytest.raises(L.BdsError):
        color_correct(torch.rand(4, 4, 3), torch.rand(4, 4, 3))
    with pytest.raises(L.BdsError):
        cubemap_sample(torch.rand(6, 4, 4, 3), torch.rand(5, 3))
    sky = EnvLight("Sky", resolution=4, device="cpu")
    assert list(sky.state_dict()) == ["base"] and sky.base.shape == (6, 4, 4, 3)
    with pytest.raises(L.BdsError):
        sky({"viewdirs": torch.rand(3, 5, 3)})
    with pytest.raises(ValueError):
        color_correct(torch.rand(4, 4, 3), torch.rand(4, 4, 4))


def test_dropin_lib_bilagrid_exports_the_product_functions():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "bilateral_driving_amd", "dropin"), ROOT]))
    code = ("import bilateral.lib_bilagrid as LB, bilateral_driving_amd.colorcorrect as C, bilateral_driving_amd.bilagrid as G\n"
            "assert LB.color_correct is C.color_correct and LB.slice_feature is G.slice_feature and LB.NeuralBilateralGrid is G.NeuralBilateralGrid\n"
            "import nvdiffrast.torch as dr, bilateral_driving_amd.envlight as E\n"
            "assert dr.cubemap_sample is E.cubemap_sample\n"
            "try:\n    LB.slice4d()\nexcept NotImplementedError:\n    print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_meta_dict_materialises_its_lazy_lists_through_every_accessor(monkeypatch):
    """rendering._Meta (the one-view fast path of rasterization()): gsplat's per-tile lists are built on first access -- through [],
    .get(), .items(), .values(), dict(meta) and ** alike (round-4 advisor finding: only [] did)."""
    import torch
    from bilateral_driving_amd import rendering as R
    calls = []

    def fake_isect_tiles(means2d, radii, depths, tile_size, tw, th, want_isect_ids=False, conics=None, opacities=None):
        calls.append(1)
        return torch.tensor([1]), None, torch.tensor([7, 8]), torch.tensor([0])
    monkeypatch.setattr(R, "isect_tiles", fake_isect_tiles)

    def fresh():
        return R._Meta({"means2d": 0, "radii": 0, "depths": torch.zeros(1, 9), "conics": 0, "opacities": torch.zeros(1, 9), "tile_size": 16,
                        "tile_width": 1, "tile_height": 1, "tiles_per_gauss": None, "isect_ids": None, "flatten_ids": None,
                        "isect_offsets": None, "_cull": False})
    for read in (lambda m: m["flatten_ids"], lambda m: m.get("flatten_ids"), lambda m: dict(m.items())["flatten_ids"],
                 lambda m: dict(m)["flatten_ids"], lambda m: (lambda **kw: kw["flatten_ids"])(**m),
                 lambda m: list(m.values())[list(m.keys()).index("flatten_ids")]):
        got = read(fresh())
        assert got is not None and got.tolist() == [7, 8]
    assert fresh().get("no_such_key", 5) == 5 and len(calls) >= 6
