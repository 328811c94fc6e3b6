"""The CPU restatement of adaptive density control (oracle/refine_oracle.py) against the golden vectors produced by the
reference's own VanillaGaussians.refinement_after (oracle/gen_golden_refine.py): this is what PINS that oracle."""
import glob
import os

import numpy as np
import pytest

from oracle import refine_oracle as RO

FILES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "refine_step*.npz")))


def load(path):
    z = np.load(path)
    ctrl = {k[5:]: z[k].item() for k in z.files if k.startswith("ctrl_")}
    P = {a: z["in" + a] for a in RO.PARAMS}
    M = {a: z["in_m" + a] for a in RO.PARAMS}
    V = {a: z["in_v" + a] for a in RO.PARAMS}
    return z, ctrl, P, M, V


def test_four_regimes_present():
    assert len(FILES) == 4


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-4] for f in FILES])
def test_refine_oracle_equals_reference(path):
    z, ctrl, P, M, V = load(path)
    oP, oM, oV, n_split = RO.refine(int(z["step"]), ctrl, float(z["scene_scale"]), int(z["num_train_images"]), P, M, V,
                                    z["in_xys_grad_norm"], z["in_vis_counts"], z["in_max_2Dsize"], z["samples"])
    assert n_split * ctrl["n_split_samples"] == z["samples"].shape[0]
    for a in RO.PARAMS:
        ref = z["out" + a]
        assert oP[a].shape == ref.shape, a                       # same topology decision for every Gaussian
        if a in ("_means", "_scales", "_opacities"):              # exp / log / 3x3 product: libm vs torch, last bits
            np.testing.assert_allclose(oP[a], ref, rtol=2e-6, atol=2e-6, err_msg=a)
        else:
            np.testing.assert_array_equal(oP[a], ref, err_msg=a)  # pure row movement
        np.testing.assert_array_equal(oM[a], z["out_m" + a], err_msg="exp_avg" + a)
        np.testing.assert_array_equal(oV[a], z["out_v" + a], err_msg="exp_avg_sq" + a)


RIGID = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "refine_rigid_*.npz")))


@pytest.mark.parametrize("path", RIGID, ids=[os.path.basename(f)[:-4] for f in RIGID])
def test_node_refinement_oracle_equals_reference(path):
    """RigidNodes.refinement_after (nodes/rigid.py:194-325, inherited by DeformableNodes): point_ids travel with the rows and the
    out-of-bound cull is decided per appended child (oracle/gen_golden_refine_rigid.py)."""
    z, ctrl, P, M, V = load(path)
    oP, oM, oV, n_split, ids = RO.refine_nodes(int(z["step"]), ctrl, float(z["scene_scale"]), int(z["num_train_images"]), P, M, V,
                                               z["in_xys_grad_norm"], z["in_vis_counts"], z["in_max_2Dsize"], z["samples"],
                                               z["in_point_ids"], z["instances_size"])
    assert n_split * ctrl["n_split_samples"] == z["samples"].shape[0]
    assert ids.dtype == np.int64
    np.testing.assert_array_equal(ids, z["out_point_ids"])
    for a in RO.PARAMS:
        ref = z["out" + a]
        assert oP[a].shape == ref.shape, a
        if a in ("_means", "_scales", "_opacities"):
            np.testing.assert_allclose(oP[a], ref, rtol=2e-6, atol=2e-6, err_msg=a)
        else:
            np.testing.assert_array_equal(oP[a], ref, err_msg=a)
        np.testing.assert_array_equal(oM[a], z["out_m" + a], err_msg="exp_avg" + a)
        np.testing.assert_array_equal(oV[a], z["out_v" + a], err_msg="exp_avg_sq" + a)


def test_node_goldens_exercise_the_per_child_box_test():
    """At least one split parent inside its box has a sampled child outside it (and the other way round): the decision cannot
    be taken per parent."""
    assert len(RIGID) == 3
    z, ctrl, P, M, V = load([f for f in RIGID if "oob_step3300" in f][0])
    sch = RO.schedule(int(z["step"]), ctrl, float(z["scene_scale"]), int(z["num_train_images"]))
    split, dup, keep_o, keep_s, keep_d = RO.plan(sch, ctrl, P["_scales"], P["_opacities"], z["in_xys_grad_norm"], z["in_vis_counts"],
                                                 z["in_max_2Dsize"])
    ctrl_no = dict(ctrl, cull_out_of_bound=False)
    oP, _, _, n_split, ids = RO.refine_nodes(int(z["step"]), ctrl_no, float(z["scene_scale"]), int(z["num_train_images"]), P, M, V,
                                             z["in_xys_grad_norm"], z["in_vis_counts"], z["in_max_2Dsize"], z["samples"],
                                             z["in_point_ids"], z["instances_size"])
    oob_new = RO.out_of_bound(oP["_means"], ids, z["instances_size"])
    oob_parent = RO.out_of_bound(P["_means"], z["in_point_ids"], z["instances_size"])
    KO, KS = int(keep_o.sum()), int(keep_s.sum())
    parents_of_children = np.nonzero(keep_s)[0]
    child0 = oob_new[KO:KO + KS]
    assert (child0 & ~oob_parent[parents_of_children]).any()
    assert (~child0 & oob_parent[parents_of_children]).any()
    assert oob_new.any() and not oob_new.all()


def test_schedule_regimes():
    z, ctrl, *_ = load(FILES[0])
    sc, n = float(z["scene_scale"]), int(z["num_train_images"])
    s = RO.schedule(3300, ctrl, sc, n)
    assert s["do_densify"] and s["do_cull"] and s["cull_by_scale"] and s["cull_by_screen"] and s["split_by_screen"] and not s["reset_opacity"]
    s = RO.schedule(1300, ctrl, sc, n)
    assert s["do_densify"] and s["do_cull"] and not s["cull_by_scale"] and not s["cull_by_screen"]
    s = RO.schedule(16300, ctrl, sc, n)
    assert not s["do_densify"] and s["do_cull"] and s["cull_by_scale"] and not s["cull_by_screen"]
    s = RO.schedule(3100, ctrl, sc, n)
    assert not s["do_densify"] and not s["do_cull"] and s["reset_opacity"]
    assert not RO.schedule(400, ctrl, sc, n)["active"]


PVG = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "pvg_refine_step*.npz")))


@pytest.mark.parametrize("step", [1300, 3100, 3300, 16300, 20300])
def test_product_schedule_forms_the_references_switches(step):
    """``densify.schedule`` and the periodic class's ``pvg_densify.schedule`` against the reference's own expressions, quoted here by
    line, over the ctrl tables the goldens were recorded with (both classes' shipped values; the periodic ones include a table whose
    ``densify_until_num_points`` lies below the row count)."""
    from bilateral_driving_amd import densify, pvg_densify

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    tables = [(load(FILES[0])[1], int(load(FILES[0])[0]["num_train_images"]), None)]
    for f in PVG:
        z = np.load(f)
        tables.append(({k[5:]: z[k].item() for k in z.files if k.startswith("ctrl_")}, int(z["num_train_images"]), int(z["N"])))
    assert len(tables) == 9 and any(c["densify_until_num_points"] < n for c, _, n in tables[1:])
    seen = set()
    for ctrl, num_train_images, num_points in tables:
        c = Cfg(ctrl)
        reset_interval = c.reset_alpha_interval                                                          # vanilla.py:212, pvg.py:154
        want = dict(do_densify=step < c.stop_split_at and step % reset_interval > max(num_train_images, c.refine_interval),   # vanilla.py:213-216
                    by_screen=step < c.stop_screen_size_at,                                              # vanilla.py:229, :318; pvg.py:179, :281
                    do_cull=step % reset_interval > max(num_train_images, c.refine_interval),            # vanilla.py:280, pvg.py:242
                    do_reset=step % reset_interval == c.refine_interval,                                 # vanilla.py:287, pvg.py:249
                    cull_by_scale=step > c.reset_alpha_interval)                                         # vanilla.py:311, pvg.py:274
        if num_points is None:
            got = densify.schedule(step, c, num_train_images)
        else:
            want["do_densify"] = want["do_densify"] and num_points < c.densify_until_num_points          # pvg.py:155-159
            got = pvg_densify.schedule(step, c, num_train_images, num_points)
        assert got == want and all(type(v) is bool for v in got.values()), (step, got, want)
        seen.add(tuple(sorted(got.items())))
    assert len(seen) >= (2 if step == 3300 else 1)      # at 3300 the full table switches the densification off


def test_product_refinement_has_no_cpu_path():
    """The product (bilateral_driving_amd.densify) must refuse CPU tensors instead of falling back to anything."""
    import types
    import torch
    from bilateral_driving_amd import _lib as L
    from bilateral_driving_amd.densify import refinement_after
    z, ctrl, P, M, V = load(FILES[0])

    class Cfg(dict):
        __getattr__ = dict.__getitem__
    model = types.SimpleNamespace(ctrl_cfg=Cfg(ctrl), scene_scale=30.0, num_train_images=150, step=3300, class_prefix="Background#",
                                  xys_grad_norm=torch.from_numpy(z["in_xys_grad_norm"]), vis_counts=torch.from_numpy(z["in_vis_counts"]),
                                  max_2Dsize=torch.from_numpy(z["in_max_2Dsize"]))
    for a in RO.PARAMS:
        setattr(model, a, torch.nn.Parameter(torch.from_numpy(P[a])))
    opt = torch.optim.Adam([{"params": [getattr(model, a)], "name": "Background#" + a} for a in RO.PARAMS], lr=0.0)
    with pytest.raises(L.BdsError):
        refinement_after(model, 3300, opt, verbose=False)
