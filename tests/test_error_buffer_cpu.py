"""The error-driven image sampler (bilateral_driving_amd/sampler.py, csrc/error_buffer.hip) on the CPU: the numpy restatement
(tests/error_buffer_ref64.py) against the reference's recorded results (tests/golden/error_buffer.npz,
scripts/gen_golden_error_buffer.py), the pixel formula on the host (tests/hostmath_error_buffer_shim.hip) against the restatement, the
draw table against the tensors the reference handed to ``torch.multinomial``, the control flow of ``propose_training_image``, the C
entries' signatures and argument checks, and the seam.

Bounds.  A map value is three subtractions, two additions and one division of non-negative terms, each rounded once, and the
multiplication by 5: at most (1 + 2^-24)^6 - 1 < 6 * 2^-24 relative from float64 -- and bit-equal to the restatement's float32 mode
where the golden's flag says that the reference's own maps are.  A float32 sum of n non-negative terms is within (n - 1) * 2^-24
relative of the exact one.  A draw weight is one float32 product in the reference and the float64 product of the same float32 factors
in the table: 2^-24 apart, held to 2^-23."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from bilateral_driving_amd import _lib as L
from bilateral_driving_amd import build as B
from bilateral_driving_amd import sampler as S
from tests import error_buffer_ref64 as R
from tests.util import build_shim, declared_signatures, kernel_resources, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = R.H * R.W


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. the restatement against the golden ------------------------------------------------------------------------------------------------
def test_restatement_equals_the_references_maps_and_buffer():
    z = R.golden()
    pred, gt, dyn = R.golden_inputs()
    assert same_bits(pred, z["pred"]) and same_bits(gt, z["gt"]) and same_bits(dyn, z["dyn"])
    assert z["maps"].shape == (R.CAMS, R.FRAMES, R.H, R.W) and z["buffer"].shape == (R.CAMS * R.FRAMES,)
    f32, f64 = R.error_map(pred, gt, dyn, np.float32), R.error_map(pred, gt, dyn, np.float64)
    if bool(z["maps_bit_equal"]):
        assert same_bits(f32, z["maps"])
    rel = float(np.max(np.abs(z["maps"].astype(np.float64) - f64) / f64))
    print(f"\nthe reference's maps: {rel:.2e} relative from float64 (bound {6 * R.EPS32:.2e}), bit-equal flag {bool(z['maps_bit_equal'])}")
    assert rel <= 6 * R.EPS32
    assert float(np.max(np.abs(f32.astype(np.float64) - f64) / f64)) <= 6 * R.EPS32
    # the boost is on exactly the pixels above 0.1f; the last camera has none
    boosted = dyn > R.DYN_THRESHOLD
    assert boosted[:-1, :, 0, 1].all() and not boosted[:-1, :, 0, 0].any() and not boosted[:, :, 0, 2].any() and not boosted[-1].any()
    plain = R.error_map(pred, gt, None, np.float32)
    assert same_bits(np.where(boosted, plain * np.float32(5), plain), z["maps"])
    # the means: image = frame * CAMS + cam
    for c in range(R.CAMS):
        for f in range(R.FRAMES):
            mean, lo, hi = R.map_stats(z["maps"][c, f])
            exact = z["maps"][c, f].astype(np.float64).mean()
            ref = float(z["buffer"][f * R.CAMS + c])
            assert abs(ref - exact) <= (N - 1) * R.EPS32 * exact, (c, f)
            assert abs(float(mean) - exact) <= R.EPS32 * exact and lo == z["maps"][c, f].min() and hi == z["maps"][c, f].max()
    assert float(z["mean_rel_distance"]) <= (N - 1) * R.EPS32


# ---- 2. the header on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    h = build_shim("error_buffer")
    vp = ctypes.c_void_p
    h.hm_eb_map.argtypes = [ctypes.c_int64, vp, vp, vp, vp]
    h.hm_eb_map.restype = None
    h.hm_eb_range.argtypes = [ctypes.c_int64, vp, vp, vp]
    h.hm_eb_range.restype = None
    return h


def shim_map(shim, pred, gt, dyn):
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    dyn = None if dyn is None else np.ascontiguousarray(dyn, np.float32)
    e = np.zeros(pred.shape[:-1], np.float32)
    shim.hm_eb_map(e.size, pred.ctypes.data, gt.ctypes.data, None if dyn is None else dyn.ctypes.data, e.ctypes.data)
    return e


def shim_range(shim, e):
    e = np.ascontiguousarray(e, np.float32)
    lo, hi = np.zeros(1, np.float32), np.zeros(1, np.float32)
    shim.hm_eb_range(e.size, e.ctypes.data, lo.ctypes.data, hi.ctypes.data)
    return lo[0], hi[0]


def test_host_formula_equals_the_restatement_bit_for_bit(shim):
    z = R.golden()
    pred, gt, dyn = z["pred"], z["gt"], z["dyn"]
    assert same_bits(shim_map(shim, pred, gt, dyn), R.error_map(pred, gt, dyn, np.float32))
    assert same_bits(shim_map(shim, pred, gt, None), R.error_map(pred, gt, None, np.float32))
    if bool(z["maps_bit_equal"]):
        assert same_bits(shim_map(shim, pred, gt, dyn), z["maps"])
    # the clamp's edges: below, at and above 0 and 1, next to them, far out; gt outside [0, 1] is not clamped
    one, zero = np.float32(1), np.float32(0)
    edge = np.array([-1e30, -0.2, -1e-45, -0.0, 0.0, 1e-45, 0.5, np.nextafter(one, zero), 1.0, np.nextafter(one, np.float32(2)), 1.3, 1e30,
                     np.inf, -np.inf], np.float32)
    p = np.stack(np.meshgrid(edge, edge[::-1], edge, indexing="ij"), -1).reshape(-1, 3)
    g = np.stack(np.meshgrid(edge[:12], np.float32([-0.5, 0.25, 1.5]), edge[:12][::-1], indexing="ij"), -1).reshape(-1, 3)
    g = np.resize(g, p.shape).astype(np.float32)
    got, want = shim_map(shim, p, g, None), R.error_map(p, g, None, np.float32)
    assert same_bits(got, want)
    clamped = shim_map(shim, np.float32([[-0.2, 1.3, 0.5]]), np.float32([[0.0, 1.0, 0.5]]), None)
    assert clamped[0] == 0.0                                  # the render is clamped ...
    assert shim_map(shim, np.float32([[0, 0, 0]]), np.float32([[1.5, -0.5, 0]]), None)[0] == np.float32(np.float32(2.0) / np.float32(3))   # ... gt is not
    # the strict > 0.1f at the three neighbouring values
    t = R.DYN_THRESHOLD
    d = np.float32([np.nextafter(t, zero), t, np.nextafter(t, one), 0.0, 1.0, -1.0, np.nan])
    pp, gg = np.tile(np.float32([[0.2, 0.4, 0.9]]), (len(d), 1)), np.tile(np.float32([[0.5, 0.1, 0.3]]), (len(d), 1))
    base = R.error_map(pp, gg, None, np.float32)
    got = shim_map(shim, pp, gg, d)
    assert same_bits(got, R.error_map(pp, gg, d, np.float32))
    assert [bool(x) for x in got != base] == [False, False, True, False, True, False, False]
    assert same_bits(got[2:3], base[2:3] * np.float32(5))
    # NaN: in any channel of pred or gt
    for k in range(3):
        for which in (0, 1):
            a, b = np.float32([[0.2, 0.4, 0.9]]), np.float32([[0.5, 0.1, 0.3]])
            (a, b)[which][0, k] = np.nan
            assert np.isnan(shim_map(shim, a, b, None)[0]) and np.isnan(R.error_map(a, b, None, np.float32)[0])
    # the running minimum and maximum propagate a NaN from anywhere, as torch's do
    e = np.float32([0.3, 0.1, 0.7, 0.2])
    assert shim_range(shim, e) == (np.float32(0.1), np.float32(0.7))
    for k in range(4):
        x = e.copy()
        x[k] = np.nan
        lo, hi = shim_range(shim, x)
        assert np.isnan(lo) and np.isnan(hi) and torch.from_numpy(x).min().isnan() and all(np.isnan(v) for v in R.map_stats(x))
    assert shim_range(shim, np.float32([np.inf, 0.5])) == (np.float32(0.5), np.float32(np.inf))


# ---- 3. the draw table ----------------------------------------------------------------------------------------------------------------
CASES = [(frames, weight, name) for frames in (R.FRAMES, R.SHORT_FRAMES) for weight in R.WEIGHTS for name in ("all", "strided")]


@pytest.mark.parametrize("frames,weight,name", CASES)
def test_draw_table_weights_equal_the_captured_multinomial_inputs(frames, weight, name):
    z = R.golden()
    num_imgs = frames * R.CAMS
    cands = R.candidate_lists(num_imgs)[name]
    table = S.DrawTable(z["buffer"][:num_imgs], cands, num_imgs, R.CAMS, weight)
    cap = z[f"mn_w{weight}_f{frames}_{name}"].astype(np.float64)
    assert table.weights.dtype == np.float64 and table.weights.shape == cap.shape == (len(cands),)
    rel = float(np.max(np.abs(table.weights - cap) / cap))
    print(f"\n{frames} frames, weight {weight}, {name}: weights {rel:.2e} relative from the reference's (bound {2.0 ** -23:.2e})")
    assert rel <= 2.0 ** -23
    want = R.draw_weights(z["buffer"][:num_imgs], cands, frames, R.CAMS, weight)
    assert float(np.max(np.abs(table.weights - want) / want)) <= 2.0 ** -23
    if weight == 3 and frames == R.FRAMES and name == "all":       # two boosted frames: 3 and 1 (linspace(3, 1, 2))
        assert np.allclose(table.weights[:R.CAMS] / z["buffer"][:R.CAMS], 3.0) and np.allclose(table.weights[R.CAMS:] / z["buffer"][R.CAMS:num_imgs], 1.0)
    if frames == R.SHORT_FRAMES:                                   # int(9 * 0.1) = 0 boosted frames
        assert np.array_equal(table.weights, z["buffer"][:num_imgs].astype(np.float64)[cands])
    assert np.array_equal(np.asarray(table.running), np.cumsum(table.weights)) and table.total == table.running[-1]
    # u at 0, just below and at every boundary of the running sum, and at the last float64 below 1
    us = [0.0, 1.0 - 2.0 ** -53]
    for r in table.running[:-1]:
        u = r / table.total
        us += [np.nextafter(u, 0.0), u, np.nextafter(u, 1.0)]
    for u in us:
        pos = R.draw(table.weights, u)
        assert table.position(u) == pos and table.draw(u) == cands[pos], u
        assert table.running[pos] > u * table.total and (pos == 0 or table.running[pos - 1] <= u * table.total)
    assert table.draw(0.0) == cands[0] and table.draw(1.0 - 2.0 ** -53) == cands[-1]


def test_draw_never_returns_a_zero_weight_candidate_and_raises_where_multinomial_does():
    buf = np.float32([0.0, 0.5, 0.0, 0.0, 0.25, 0.25, 0.0, 0.0])
    cands = list(range(8))
    table = S.DrawTable(buf, cands, 8, 1, 1)
    assert table.last == 5
    hits = {table.draw(u) for u in [0.0, 0.25, 0.4999999, 0.5, 0.5000001, 0.75, 0.7500001, 1.0 - 2.0 ** -53]
            + list(np.linspace(0.0, 1.0, 1001, endpoint=False))}
    assert hits == {1, 4, 5}
    for u in (0.0, 0.5, 0.75, 1.0 - 2.0 ** -53):
        assert table.position(u) == R.draw(buf.astype(np.float64), u)
    assert table.draw(0.0) == 1 and table.draw(0.5) == 4 and table.draw(0.75) == 5 and table.draw(1.0 - 2.0 ** -53) == 5
    assert S.DrawTable(buf, [7, 1, 6], 8, 1, 1).draw(1.0 - 2.0 ** -53) == 1       # a zero weight last in the list
    # a sum that rounds up: u * total can reach the total; the clamp keeps the draw on a non-zero weight
    tiny = S.DrawTable(np.float32([1.0, 1e-30, 0.0]), [0, 1, 2], 3, 1, 1)
    assert tiny.draw(1.0 - 2.0 ** -53) in (0, 1)
    for bad in ([0.0, 0.0, 0.0], [0.5, -0.1, 0.7], [0.5, np.nan, 0.7], [np.inf, 1.0, 1.0]):
        with pytest.raises(RuntimeError):
            S.DrawTable(np.float32(bad), [0, 1, 2], 3, 1, 1)
        if not np.isinf(bad[0]):
            with pytest.raises(RuntimeError):
                torch.multinomial(torch.tensor(bad, dtype=torch.float32), 1, replacement=False)
    with pytest.raises(RuntimeError):
        torch.multinomial(torch.tensor([np.inf, 1.0, 1.0]), 1, replacement=False)
    # the distribution: the frequency of each candidate over a fine grid of u is its weight's share
    z = R.golden()
    table = S.DrawTable(z["buffer"], list(range(75)), 75, R.CAMS, 3)
    grid = (np.arange(20000) + 0.5) / 20000
    freq = np.bincount([table.position(u) for u in grid], minlength=75) / len(grid)
    assert np.max(np.abs(freq - table.weights / table.total)) <= 1.0 / len(grid) + 1e-12


# ---- 4. propose_training_image ---------------------------------------------------------------------------------------------------------
class Randoms:
    """``random.random`` and ``random.choice`` replaced: scripted values, every call recorded."""

    def __init__(self, monkeypatch, values):
        self.values, self.calls = list(values), []
        monkeypatch.setattr(random, "random", self.random)
        monkeypatch.setattr(random, "choice", self.choice)

    def random(self):
        self.calls.append("random")
        return self.values.pop(0)

    def choice(self, seq):
        self.calls.append("choice")
        return seq[-1]


def filled_source(ratio, weight=None):
    z = R.golden()
    s = R.bare_pixel_source("cpu", buffer_ratio=ratio, start_enhance_weight=weight)
    s.image_error_buffer, s.image_error_buffered = torch.from_numpy(z["buffer"].copy()), True
    return s


def test_propose_training_image_keeps_the_references_control_flow(monkeypatch):
    z = R.golden()
    cands = R.candidate_lists(75)["strided"]
    # buffer_ratio 0: random.choice, one random.random()
    r = Randoms(monkeypatch, [0.0])
    assert S.propose_training_image(filled_source(0.0), cands) == cands[-1] and r.calls == ["random", "choice"]
    # buffer_ratio 1: the table, a second random.random() for u
    s = filled_source(1.0, 3)
    r = Randoms(monkeypatch, [0.999, 0.37])
    got = S.propose_training_image(s, cands)
    want = cands[R.draw(R.draw_weights(z["buffer"], cands, R.FRAMES, R.CAMS, 3), 0.37)]
    assert got == want and r.calls == ["random", "random"]
    # not yet buffered: random.choice whatever the ratio
    s2 = R.bare_pixel_source("cpu", buffer_ratio=1.0)
    r = Randoms(monkeypatch, [0.0])
    assert S.propose_training_image(s2, cands) == cands[-1] and r.calls == ["random", "choice"] and not hasattr(s2, "_bds_draw_tables")
    # the reference's comparison is strict: random.random() == buffer_ratio takes random.choice
    r = Randoms(monkeypatch, [0.5])
    assert S.propose_training_image(filled_source(0.5), cands) == cands[-1] and r.calls == ["random", "choice"]
    # the table is reused across calls ...
    table = S.draw_table(s, cands)
    r = Randoms(monkeypatch, [0.0, 0.0, 0.0, 1.0 - 2.0 ** -53])
    assert S.propose_training_image(s, list(cands)) == cands[0] and S.propose_training_image(s, tuple(cands)) == cands[-1]
    assert S.draw_table(s, cands) is table and len(s._bds_draw_tables) == 1
    # ... rebuilt for another candidate list (the first stays cached) ...
    every = R.candidate_lists(75)["all"]
    other = S.draw_table(s, every)
    assert other is not table and len(other.weights) == 75 and S.draw_table(s, cands) is table and S.draw_table(s, every) is other
    # ... and after a buffer update
    s.image_error_buffer = torch.from_numpy(z["buffer"][::-1].copy())
    fresh = S.draw_table(s, cands)
    assert fresh is not table and np.allclose(fresh.weights, R.draw_weights(z["buffer"][::-1], cands, R.FRAMES, R.CAMS, 3), rtol=2.0 ** -23, atol=0)
    assert S.draw_table(s, cands) is fresh
    # start_enhance_weight absent: 1, as ``sampler.get('start_enhance_weight', 1)``
    plain = S.draw_table(filled_source(1.0), every)
    assert np.array_equal(plain.weights, z["buffer"].astype(np.float64))


# ---- 5. the C entries -----------------------------------------------------------------------------------------------------------------
def test_entries_resolve_with_the_declared_signatures():
    full = open(os.path.join(ROOT, "include", "bds.h")).read()
    decl = {k: v for k, v in declared_signatures().items() if k.startswith("bds_error_maps")}
    assert sorted(decl) == ["bds_error_maps", "bds_error_maps_workspace_bytes"]
    lib = L.lib()
    for name, (ret, args) in decl.items():
        assert L._SIGS[name] == (ret, args) and ret in (ctypes.c_int, ctypes.c_size_t), name
        assert getattr(lib, name).argtypes == args, name
    assert len(decl["bds_error_maps"][1]) == 15 and len(decl["bds_error_maps_workspace_bytes"][1]) == 3
    assert "error_buffer.hip" in B.SOURCES
    assert lib.bds_abi_version() == L.ABI_VERSION == 7      # (what each version changed: include/bds.h)
    for cite in ("datasets/base/pixel_source.py:431-449", ":948-983", "models/video_utils.py:185-187"):
        assert cite in full, cite
    kernel = open(os.path.join(B.CSRC, "error_buffer.hip")).read()
    assert "atomic" not in kernel.split("namespace bds {", 1)[1]      # no atomics: bit-identical run to run
    assert len(re.findall(r"fabsf", kernel)) == 0 and "eb_pixel" in kernel      # the formula is stated in the header only
    assert len(re.findall(r"/ 3\.0f", open(os.path.join(B.CSRC, "error_buffer_math.h")).read())) == 1


def test_error_buffer_kernel_resources():
    res = {short_name(k): v for k, v in kernel_resources("error_buffer.hip").items()}
    assert sorted(res) == ["error_maps_kernel", "error_stats_kernel"], list(res)
    for k, v in res.items():
        print(f"\n{k}: occupancy {v['Occupancy']} waves/SIMD, {v['VGPRs']} VGPRs, static LDS {v['LDS Size']} bytes")
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 8, (k, v)      # a stream-bound pass: nothing spilled, every wave slot usable


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = L.lib()
    p = 1 << 20      # never dereferenced: every case fails its argument check first
    big = 1 << 40

    def call(B=3, h=5, w=7, pred=p, gt=p, dyn=p, slots=p, ids=p, maps=p, F=9, stats=p, num_imgs=12, ws=p, ws_bytes=big):
        return lib.bds_error_maps(B, h, w, pred, gt, dyn, slots, ids, maps, F, stats, num_imgs, ws, ws_bytes, None)
    # nothing to do: 0, whatever the pointers
    assert call(B=0) == 0 and lib.bds_error_maps(0, 0, 0, *([None] * 6), 0, None, 0, None, 0, None) == 0
    assert call(h=0, stats=None) == 0 and call(w=0, ids=None) == 0
    assert lib.bds_error_maps(2, 0, 7, *([None] * 6), 0, None, 0, None, 0, None) == 0
    need = lib.bds_error_maps_workspace_bytes(3, 5, 7)
    assert need >= 3 * 16 and need % 16 == 0
    assert lib.bds_error_maps_workspace_bytes(200, 135, 240) >= 200 * 32 * 16      # 8100 quads: 32 workgroups per view
    assert lib.bds_error_maps_workspace_bytes(1, 1080, 1920) >= 1024 * 16          # at most 1024 per view
    assert lib.bds_error_maps_workspace_bytes(0, 5, 7) > 0 and lib.bds_error_maps_workspace_bytes(3, 0, 7) > 0
    for kw in (dict(B=-1), dict(h=-1), dict(w=-2), dict(F=-1), dict(num_imgs=-1),
               dict(B=1 << 12, h=1 << 10, w=1 << 10), dict(B=1, h=1 << 16, w=1 << 15), dict(B=2, h=1 << 15, w=1 << 15),      # beyond 32-bit
               dict(pred=None), dict(gt=None), dict(slots=None), dict(ids=None), dict(maps=None), dict(stats=None), dict(ws=None),
               dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(pred=p + 2), dict(gt=p + 1), dict(dyn=p + 2), dict(maps=p + 3), dict(stats=p + 2), dict(slots=p + 4), dict(ids=p + 4),
               dict(ws=p + 8)):
        assert call(**kw) == L.BDS_EINVAL == -1, kw
    for args in ((-1, 5, 7), (3, -5, 7), (1 << 12, 1 << 10, 1 << 10)):
        assert lib.bds_error_maps_workspace_bytes(*args) == 0


def test_python_checks_arguments_and_refuses_cpu_tensors():
    import bilateral_driving_amd
    assert bilateral_driving_amd.sampler is S
    B_, h, w = 2, 5, 7
    pred, gt, dyn = torch.rand(B_, h, w, 3), torch.rand(B_, h, w, 3), torch.rand(B_, h, w)
    maps, stats, ids = torch.zeros(4, h, w), torch.zeros(6, 3), torch.arange(B_)
    with pytest.raises(L.BdsError):
        S.error_maps(pred, gt, dyn, maps, ids, stats, ids)
    with pytest.raises(L.BdsError):
        S.update_image_error_maps(R.bare_pixel_source("cpu"), R.render_results(*R.golden_inputs()))
    for kw in (dict(pred=pred[..., :2]), dict(gt=gt[:1]), dict(dyn=dyn[:, :4]), dict(maps=maps[:, :4]), dict(maps=maps.double()),
               dict(maps=torch.zeros(4, w, h).transpose(1, 2)), dict(stats=torch.zeros(6, 2)), dict(stats=stats.double()),
               dict(slots=ids.int()), dict(slots=torch.arange(3)), dict(ids=torch.arange(1)), dict(pred=pred[0, 0], gt=gt[0, 0])):
        a = {**dict(pred=pred, gt=gt, dyn=dyn, maps=maps, slots=ids, stats=stats, ids=ids), **kw}
        with pytest.raises(ValueError):
            S.error_maps(a["pred"], a["gt"], a["dyn"], a["maps"], a["slots"], a["stats"], a["ids"])


# ---- 6. the seam ----------------------------------------------------------------------------------------------------------------------
def test_install_and_uninstall_put_back_what_was_there():
    class Camera:
        def get_image_error_video(self):
            return "former video"

    class Source:
        def update_image_error_maps(self, render_results):
            return "former update"

        def propose_training_image(self, candidate_indices=None):
            return "former draw"
    former = {k: Source.__dict__[k] for k in ("update_image_error_maps", "propose_training_image")}
    former_cam = Camera.__dict__["get_image_error_video"]
    S.install(Camera, Source)
    S.install(Camera, Source)      # (twice: the former functions are still the ones remembered)
    assert Camera.get_image_error_video.__wrapped__ is S.get_image_error_video
    assert Source.update_image_error_maps.__wrapped__ is S.update_image_error_maps
    assert Source.propose_training_image.__wrapped__ is S.propose_training_image
    cam = Camera()
    cam.cam_to_worlds = torch.eye(4)[None]      # on the CPU: the class's own methods
    src = Source()
    src.camera_data = {0: cam}
    assert cam.get_image_error_video() == "former video" and src.update_image_error_maps({}) == "former update"
    assert src.propose_training_image([1, 2]) == "former draw"

    class Derived(Source):      # inherits: a CPU object still reaches the inherited method
        pass
    S.install(None, Derived)
    d = Derived()
    d.camera_data = {0: cam}
    assert "propose_training_image" in Derived.__dict__ and d.propose_training_image([1]) == "former draw"
    S.uninstall(Derived)
    assert "propose_training_image" not in Derived.__dict__ and d.propose_training_image([1]) == "former draw"

    class Bare:
        pass
    S.install(Bare, Bare)
    assert Bare.get_image_error_video.__wrapped__ is S.get_image_error_video
    from bilateral_driving_amd import pixels
    pixels.install(Camera)       # another module's seam on the same class is its own
    S.uninstall()
    assert Camera.__dict__["get_image_error_video"] is former_cam and all(Source.__dict__[k] is v for k, v in former.items())
    assert not any(k in Bare.__dict__ for k in ("get_image_error_video", "update_image_error_maps", "propose_training_image"))
    assert Camera.get_image.__wrapped__ is pixels.get_image
    pixels.uninstall(Camera)
    assert "get_image" not in Camera.__dict__
