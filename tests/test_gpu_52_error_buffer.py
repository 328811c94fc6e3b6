"""The error-driven image sampler on the MI355X (csrc/error_buffer.hip through bilateral_driving_amd/sampler.py) against the numpy
restatement (tests/error_buffer_ref64.py) and the reference's recorded results (tests/golden/error_buffer.npz), both pinned to the
reference by tests/test_error_buffer_cpu.py.  No test reads the reference tree.

Bounds.  The maps: bit-equal to the restatement's float32 mode where the golden's flag says that the reference's own maps are, else
6 * 2^-24 relative from float64 (six roundings of non-negative terms).  The mean: within 2^-23 relative of the float64 mean of the
RETURNED float32 map (one rounding to float32, 2^-24, plus the float64 sum's n * 2^-53).  Min and max: equal to the returned map's.
The shapes: one pixel, fewer pixels than a wave (35), a row length that is no multiple of 4 (17 x 23 = 391 pixels: three tail pixels,
two workgroups' worth of lanes only partly used), and the shipped 1080p / 8 (135 x 240: 32 workgroups per view).  Every case runs from
16-byte aligned bases and from bases one element off (the 4-byte path), with slots and image ids permuted and non-contiguous inside
larger buffers.

Figures measured on the MI355X (this file's own prints): the mean stands at most 4.4e-08 relative from the float64 mean of the returned
map over every shape (bound 1.19e-07); the maps are bit-equal to the restatement's float32 mode on every shape, from aligned and from
offset bases alike."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import error_buffer_ref64 as R
from tests.poison import holds_poison, poisoned_allocations

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (5, 7), (17, 23), (135, 240))
EXTRA_MAPS, EXTRA_STATS = 3, 4      # rows that no view names


@pytest.fixture(scope="module")
def S():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from bilateral_driving_amd import _lib
    _lib.lib()
    from bilateral_driving_amd import sampler
    return sampler


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()      # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().contiguous().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(h, w, B):
    """Random views and the restatement of them in both modes, computed once and left unchanged."""
    rng = np.random.default_rng(h * 1000 + w * 10 + B)
    pred = rng.uniform(-0.2, 1.3, (B, h, w, 3)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (B, h, w, 3)).astype(np.float32)
    dyn = rng.uniform(0.0, 0.2, (B, h, w)).astype(np.float32)
    dyn.reshape(-1)[0] = R.DYN_THRESHOLD
    ref = {with_dyn: (R.error_map(pred, gt, dyn if with_dyn else None, np.float32), R.error_map(pred, gt, dyn if with_dyn else None, np.float64))
           for with_dyn in (False, True)}
    for a in (pred, gt, dyn) + tuple(x for pair in ref.values() for x in pair):
        a.setflags(write=False)
    return pred, gt, dyn, ref


def offset_view(a, off):
    """``a`` on the device at a base ``off`` elements behind a fresh allocation's."""
    d = dev(a)
    flat = torch.zeros(d.numel() + off, dtype=d.dtype, device="cuda")
    flat[off:] = d.reshape(-1)
    return flat[off:].view(d.shape)


def ids_for(B, rows):
    """B distinct rows of ``rows``, out of order and with gaps."""
    return [(rows - 1 - 2 * b) % rows for b in range(B)] if B > 1 else [rows - 2]


def check_outputs(maps, stats, fill_maps, fill_stats, slots, ids, f32, f64, label):
    """``maps`` [F,h,w], ``stats`` [num_imgs,3] as numpy, after a call over the views whose restatement is ``f32`` / ``f64`` [B,h,w]."""
    flag = bool(R.golden()["maps_bit_equal"])
    worst = 0.0
    for b, (slot, i) in enumerate(zip(slots, ids)):
        m = maps[slot]
        if not np.isnan(f64[b]).any():
            if flag:
                assert same_bits(m, f32[b]), (label, b)
            assert float(np.max(np.abs(m.astype(np.float64) - f64[b]) / f64[b])) <= 6 * R.EPS32, (label, b)
            mean64 = m.astype(np.float64).mean()
            worst = max(worst, abs(float(stats[i, 0]) - mean64) / mean64)
            assert abs(float(stats[i, 0]) - mean64) <= 2.0 ** -23 * mean64, (label, b, stats[i, 0], mean64)
            assert stats[i, 1] == m.min() and stats[i, 2] == m.max(), (label, b)
        else:
            nan = np.isnan(f32[b])
            assert np.array_equal(np.isnan(m), nan) and np.array_equal(bits(m)[~nan], bits(f32[b])[~nan]), (label, b)
            assert np.isnan(stats[i]).all(), (label, b, stats[i])
    other_maps = [r for r in range(maps.shape[0]) if r not in slots]
    other_stats = [r for r in range(stats.shape[0]) if r not in ids]
    assert same_bits(maps[other_maps], fill_maps[other_maps]) and same_bits(stats[other_stats], fill_stats[other_stats]), label
    return worst


def run(S, h, w, B, with_dyn, off, nan_view=None):
    pred, gt, dyn, ref = case(h, w, B)
    f32, f64 = ref[with_dyn]
    if nan_view is not None:
        pred = pred.copy()
        pred[nan_view].reshape(-1)[min(4, pred[nan_view].size - 1)] = np.nan
        f32, f64 = (R.error_map(pred, gt, dyn if with_dyn else None, t) for t in (np.float32, np.float64))
    F, num_imgs = B + EXTRA_MAPS, B + EXTRA_STATS
    rng = np.random.default_rng(7)
    fill_maps, fill_stats = rng.uniform(-9, -1, (F, h, w)).astype(np.float32), rng.uniform(-9, -1, (num_imgs, 3)).astype(np.float32)
    maps, stats = offset_view(fill_maps, off), offset_view(fill_stats, off)
    slots, ids = ids_for(B, F), ids_for(B, num_imgs)
    S.error_maps(offset_view(pred, off), offset_view(gt, off), offset_view(dyn, off) if with_dyn else None, maps, dev(np.int64(slots)), stats,
                 dev(np.int64(ids)))
    return host(maps), host(stats), fill_maps, fill_stats, slots, ids, f32, f64


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dyn", [True, False], ids=["dyn", "nodyn"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_error_maps_equal_the_restatement(S, size, B, with_dyn):
    h, w = size
    label = f"{h}x{w} B={B} {'dyn' if with_dyn else 'no dyn'}"
    outs = {}
    for off in (0, 1):
        out = run(S, h, w, B, with_dyn, off)
        worst = check_outputs(*out, f"{label} offset {off}")
        print(f"\nerror_maps {label} offset {off}: mean at most {worst:.2e} relative from the float64 mean of the returned map (bound {2.0 ** -23:.2e})")
        outs[off] = out
    # the 16-byte and the 4-byte path give the same bits, statistics included
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), label
    # one NaN pixel: that image's mean, min and max are NaN, the others' are what they were
    nan_view = B - 1
    maps, stats, fill_maps, fill_stats, slots, ids, f32, f64 = run(S, h, w, B, with_dyn, 0, nan_view)
    check_outputs(maps, stats, fill_maps, fill_stats, slots, ids, f32, f64, f"{label} NaN")
    assert np.isnan(stats[ids[nan_view]]).all() and np.isnan(maps[slots[nan_view]]).sum() == 1
    for b in range(B):
        if b != nan_view:
            assert same_bits(stats[ids[b]], outs[0][1][ids[b]]) and same_bits(maps[slots[b]], outs[0][0][slots[b]])


def test_empty_views_and_empty_batches(S):
    stats = torch.full((4, 3), -2.0, device="cuda")
    S.error_maps(torch.zeros(2, 0, 7, 3, device="cuda"), torch.zeros(2, 0, 7, 3, device="cuda"), None, torch.zeros(3, 0, 7, device="cuda"),
                 dev(np.int64([0, 2])), stats, dev(np.int64([3, 1])))
    got = host(stats)
    assert np.isnan(got[[1, 3]]).all() and np.array_equal(got[[0, 2]], np.full((2, 3), -2.0, np.float32))      # the mean of nothing
    S.error_maps(torch.zeros(0, 5, 7, 3, device="cuda"), torch.zeros(0, 5, 7, 3, device="cuda"), None, torch.zeros(3, 5, 7, device="cuda"),
                 dev(np.int64([])), stats, dev(np.int64([])))
    assert same_bits(host(stats), got)
    # a slot or an id outside its buffer drops that view's map or statistics: nothing is written
    pred, gt, dyn, ref = case(5, 7, 3)
    maps, stats = torch.full((3, 5, 7), -2.0, device="cuda"), torch.full((3, 3), -2.0, device="cuda")
    S.error_maps(dev(pred), dev(gt), None, maps, dev(np.int64([3, 1, -1])), stats, dev(np.int64([0, -5, 3])))
    m, s = host(maps), host(stats)
    assert same_bits(m[1], ref[False][0][1]) and (m[[0, 2]] == -2.0).all() and (s[[1, 2]] == -2.0).all() and s[0, 1] == ref[False][0][0].min()


# ---- 2. repeatability ------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(S):
    a, b = run(S, 135, 240, 3, True, 0), run(S, 135, 240, 3, True, 0)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    a, b = run(S, 17, 23, 3, True, 1), run(S, 17, 23, 3, True, 1)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# ---- 3. poisoned memory ------------------------------------------------------------------------------------------------------------------
def test_error_maps_on_poisoned_memory(S):
    h, w, B = 17, 23, 3
    pred, gt, dyn, ref = case(h, w, B)
    F, num_imgs = B + EXTRA_MAPS, B + EXTRA_STATS
    slots, ids = ids_for(B, F), ids_for(B, num_imgs)
    p, g, d, sl, im = dev(pred), dev(gt), dev(dyn), dev(np.int64(slots)), dev(np.int64(ids))
    with poisoned_allocations(True, name="error_maps") as pz:
        maps = torch.empty(F, h, w, dtype=torch.float32, device="cuda")
        stats = torch.empty(num_imgs, 3, dtype=torch.float32, device="cuda")
        ws = S.error_maps(p, g, d, maps, sl, stats, im)          # (the workspace comes from torch.empty inside)
        assert len(pz.records) == 3 and ws.numel() >= 16 * B
        pz.check_guards()
        assert not bool(holds_poison(maps[slots]).any()) and not bool(holds_poison(stats[ids]).any())
        others_m, others_s = [r for r in range(F) if r not in slots], [r for r in range(num_imgs) if r not in ids]
        assert bool(holds_poison(maps[others_m]).all()) and bool(holds_poison(stats[others_s]).all())
        m, s = host(maps), host(stats)
    fill_m, fill_s = m.copy(), s.copy()
    check_outputs(m, s, fill_m, fill_s, slots, ids, *ref[True], "poisoned")


# ---- 4. the streaming and the batched update against the golden ---------------------------------------------------------------------------
def view_dicts(c, f, pred, gt, dyn, host_ids=False):
    """One view's tensors as the trainer and ``get_image`` hand them over: image ``f * CAMS + c``."""
    i = f * R.CAMS + c
    full = (lambda v: v) if host_ids else (lambda v: torch.full((R.H, R.W), v, dtype=torch.int64, device="cuda"))
    results = {"rgb": dev(pred[c, f]), "Dynamic_opacity": dev(dyn[c, f])[..., None]}
    image_infos = {"pixels": dev(gt[c, f]), "img_idx": full(i), "frame_idx": full(f)}
    cam_infos = {"cam_id": torch.full((R.H, R.W), c, dtype=torch.int64, device="cuda"), "cam_name": R.CAM_NAMES[c]}
    return results, image_infos, cam_infos


def sweep_all(S, source, skip=(), twice=()):
    z = R.golden()
    sweep = S.ErrorSweep(source)
    for f in range(R.FRAMES):
        for c in range(R.CAMS):
            if (c, f) in skip:
                continue
            for _ in range(2 if (c, f) in twice else 1):
                sweep.add(*view_dicts(c, f, z["pred"], z["gt"], z["dyn"], host_ids=(c == 2)))
    return sweep


@pytest.fixture(scope="module")
def swept(S):
    """The golden's 75 views through ``ErrorSweep``, once: the pixel source it filled."""
    source = R.bare_pixel_source("cuda", start_enhance_weight=3)
    sweep_all(S, source).finish()
    return source


def check_golden(source):
    z = R.golden()
    n = R.H * R.W
    assert source.image_error_buffered is True and tuple(source.image_error_buffer.shape) == (R.CAMS * R.FRAMES,)
    buffer = host(source.image_error_buffer)
    for c in range(R.CAMS):
        m = host(source.camera_data[c].image_error_maps)
        assert m.dtype == np.float32 and m.shape == (R.FRAMES, R.H, R.W)
        if bool(z["maps_bit_equal"]):
            assert same_bits(m, z["maps"][c]), c
        f64 = R.error_map(z["pred"][c], z["gt"][c], z["dyn"][c], np.float64)
        assert float(np.max(np.abs(m.astype(np.float64) - f64) / f64)) <= 6 * R.EPS32
        for f in range(R.FRAMES):
            i, exact = f * R.CAMS + c, m[f].astype(np.float64).mean()
            assert abs(float(buffer[i]) - exact) <= 2.0 ** -23 * exact
            assert abs(float(buffer[i]) - float(z["buffer"][i])) <= n * R.EPS32 * exact      # the reference's float32 sum: (n - 1) * 2^-24
            assert same_bits(host(source.image_error_stats[i]), np.float32([buffer[i], m[f].min(), m[f].max()]))
    return buffer


def test_sweep_and_batched_update_give_the_same_bits_and_the_goldens(S, swept):
    z = R.golden()
    streamed = check_golden(swept)
    batched = R.bare_pixel_source("cuda", start_enhance_weight=3)
    S.update_image_error_maps(batched, R.render_results(z["pred"], z["gt"], z["dyn"]))
    assert same_bits(check_golden(batched), streamed)
    for c in range(R.CAMS):
        assert same_bits(host(batched.camera_data[c].image_error_maps), host(swept.camera_data[c].image_error_maps))
    assert same_bits(host(batched.image_error_stats), host(swept.image_error_stats))
    # the unclamped render gives the same: the kernel clamps
    raw = R.bare_pixel_source("cuda")
    S.update_image_error_maps(raw, R.render_results(z["pred"], z["gt"], z["dyn"], clamp=False))
    assert same_bits(host(raw.image_error_buffer), streamed)
    # without a dynamic opacity: no boost anywhere
    plain = R.bare_pixel_source("cuda")
    results = R.render_results(z["pred"], z["gt"], None)
    S.update_image_error_maps(plain, results)
    assert same_bits(host(plain.camera_data[0].image_error_maps), R.error_map(z["pred"][0], z["gt"][0], None, np.float32))
    # the reference's shape assertion
    short = R.render_results(z["pred"], z["gt"], z["dyn"], num_frames=R.FRAMES - 1)
    with pytest.raises(ValueError):
        S.update_image_error_maps(R.bare_pixel_source("cuda"), short)


def test_finish_refuses_an_incomplete_sweep(S):
    for kw in (dict(skip={(1, 7)}), dict(skip={(0, 3)}, twice={(0, 4)})):
        source = R.bare_pixel_source("cuda")
        before = {c: source.camera_data[c].image_error_maps for c in range(R.CAMS)}
        with pytest.raises(ValueError):
            sweep_all(S, source, **kw).finish()
        assert source.image_error_buffered is False and source.image_error_buffer is None
        assert all(source.camera_data[c].image_error_maps is before[c] for c in range(R.CAMS))
    with pytest.raises(ValueError):      # a view that does not fit the camera's maps
        z = R.golden()
        results, image_infos, cam_infos = view_dicts(0, 0, z["pred"], z["gt"], z["dyn"])
        results = {"rgb": results["rgb"][:4], "Dynamic_opacity": results["Dynamic_opacity"][:4]}
        S.ErrorSweep(R.bare_pixel_source("cuda")).add(results, {**image_infos, "pixels": image_infos["pixels"][:4]}, cam_infos)


# ---- 5. the whole update, then a draw ----------------------------------------------------------------------------------------------------
class Randoms:
    def __init__(self, monkeypatch, values):
        self.values = list(values)
        monkeypatch.setattr(random, "random", lambda: self.values.pop(0))
        monkeypatch.setattr(random, "choice", lambda seq: "choice")


def test_cache_image_errors_fills_the_buffer_and_the_draw_uses_it(S, swept, monkeypatch):
    z = R.golden()
    source = R.bare_pixel_source("cuda", start_enhance_weight=3, buffer_downscale=8)

    class Split:
        def __len__(self):
            return R.CAMS * R.FRAMES

        def get_image(self, i, camera_downscale):
            assert camera_downscale == 1 and source.downscale_factor == 1 / 8
            _, image_infos, cam_infos = view_dicts(i % R.CAMS, i // R.CAMS, z["pred"], z["gt"], z["dyn"])
            return image_infos, cam_infos

    class Dataset:
        pixel_source, full_image_set = source, Split()

    class Trainer:
        calls, evals = 0, 0

        def set_eval(self):
            self.evals += 1

        def _get_downscale_factor(self):
            return 1

        def __call__(self, image_infos, cam_infos):
            assert not torch.is_grad_enabled()
            i, self.calls = self.calls, self.calls + 1
            return view_dicts(i % R.CAMS, i // R.CAMS, z["pred"], z["gt"], z["dyn"])[0]
    trainer = Trainer()
    S.cache_image_errors(trainer, Dataset())
    assert trainer.evals == 1 and trainer.calls == R.CAMS * R.FRAMES
    assert source.factor_log == [1 / 8, 1.0] and source.downscale_factor == 1.0 and source.camera_data[0].downscale_factor == 1.0
    assert source.image_error_buffered is True
    assert same_bits(host(source.image_error_buffer), host(swept.image_error_buffer))
    buffer = host(source.image_error_buffer)
    cands = R.candidate_lists(R.CAMS * R.FRAMES)["strided"]
    weights = R.draw_weights(buffer, cands, R.FRAMES, R.CAMS, 3)
    for u in (0.0, 0.37, 0.93, 1.0 - 2.0 ** -53):
        Randoms(monkeypatch, [0.1, u])      # 0.1 < buffer_ratio = 0.5: the table
        assert S.propose_training_image(source, cands) == cands[R.draw(weights, u)]
    assert len(source._bds_draw_tables) == 1 and source._bds_buffer_host[0] is source.image_error_buffer      # no further read-back
    Randoms(monkeypatch, [0.9])
    assert S.propose_training_image(source, cands) == "choice"
    # a buffer that somebody else set is read once
    source.image_error_buffer = dev(z["buffer"])
    Randoms(monkeypatch, [0.1, 0.37])
    assert S.propose_training_image(source, cands) == cands[R.draw(R.draw_weights(z["buffer"], cands, R.FRAMES, R.CAMS, 3), 0.37)]


# ---- 6. the video ------------------------------------------------------------------------------------------------------------------------
def test_image_error_video_equals_the_references_expression(S, swept):
    for c in range(R.CAMS):
        cam = swept.camera_data[c]
        m = cam.image_error_maps
        assert cam._bds_error_range[0] is m
        want = host((m - m.min()) / (m.max() - m.min())).reshape(R.FRAMES, R.H, R.W)      # pixel_source.py:412-426
        got = S.get_image_error_video(cam)
        assert isinstance(got, list) and len(got) == R.FRAMES and all(same_bits(g, w_) for g, w_ in zip(got, want))
        assert float(min(g.min() for g in got)) == 0.0 and float(max(g.max() for g in got)) == 1.0
    cam = R.BareCamera(0, 4, R.H, R.W, "cuda")      # maps that no update made: searched as the reference does
    cam.image_error_maps = torch.rand(4, R.H, R.W, device="cuda")
    m = cam.image_error_maps
    assert all(same_bits(g, w_) for g, w_ in zip(S.get_image_error_video(cam), host((m - m.min()) / (m.max() - m.min()))))
