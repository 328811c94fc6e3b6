"""``install`` / ``uninstall`` of the nine drop-in modules (bilateral_driving_amd/_patch.py) on stand-in classes and modules: whatever
the order, every target ends with exactly the ``__dict__`` it started with, a subclass never takes its base class's patch for its own,
and one module's ``uninstall()`` leaves the other modules' patches alone.  Pure Python, no GPU."""
import types

import pytest
import torch

from bilateral_driving_amd import deform, geometry, init, lidar, marshalling, nodes, pixels, pseudo_lidar, pvg

GG, REF = "get_gaussians", "_bds_reference_get_gaussians"
# id -> (install(target), uninstall(*targets), the name it sets, the attribute that keeps the former method or None)
CLASS_SEAMS = {
    "marshalling": (marshalling.install, marshalling.uninstall, GG, REF),
    "deform": (deform.install, deform.uninstall, "forward", "_bds_reference_forward"),
    "nodes": (nodes.install, nodes.uninstall, GG, REF),
    "pvg": (pvg.install, pvg.uninstall, GG, REF),
    "pixels": (lambda c: pixels.install(camera_data_class=c), pixels.uninstall, "get_image", None),
    "lidar": (lambda c: lidar.install(dataset_class=c), lidar.uninstall, "get_init_objects", None),
}
MODULE_SEAMS = {
    "init": (init.install, init.uninstall, "k_nearest_sklearn", None),
    "pseudo_lidar": (pseudo_lidar.install, pseudo_lidar.uninstall, "pto_ang_map", None),
    "geometry": (geometry.install, geometry.uninstall, "chamfer_distance", None),
    "lidar_module": (lambda m: lidar.install(pixel_source_module=m), lidar.uninstall, "sparse_lidar_map_downsampler", None),
}
SEAMS = {**CLASS_SEAMS, **MODULE_SEAMS}
WITH_REFERENCE = [k for k, v in CLASS_SEAMS.items() if v[3] is not None]


def make_class(name, method=None, base=object):
    """A class whose ``method`` (None: no method of its own) returns the class's name."""
    body = {} if method is None else {method: lambda self, *args, **kwargs: name}
    return type(name, (base,), body)


def make_target(seam, own=True):
    """A stand-in target of the seam's kind that defines the seam's name (``own``) or does not."""
    name = SEAMS[seam][2]
    if seam in CLASS_SEAMS:
        return make_class("Target", name if own else None)
    m = types.ModuleType("target")
    if own:
        setattr(m, name, lambda *args, **kwargs: "target")
    return m


def held(target):
    return dict(vars(target))


@pytest.mark.parametrize("seam", SEAMS)
def test_own_attribute_comes_back_as_the_identical_object(seam):
    install, uninstall, name, ref = SEAMS[seam]
    target = make_target(seam)
    before, original = held(target), vars(target)[name]
    install(target)
    assert vars(target)[name] is not original
    if ref is not None:
        assert vars(target)[ref] is original
    uninstall(target)
    assert vars(target)[name] is original and held(target) == before
    uninstall(target)                                   # never installed (any more): nothing happens
    assert held(target) == before


@pytest.mark.parametrize("seam", SEAMS)
def test_a_target_without_the_name_loses_it_again(seam):
    install, uninstall, name, _ = SEAMS[seam]
    target = make_target(seam, own=False)
    before = held(target)
    install(target)
    assert name in vars(target)
    uninstall(target)
    assert held(target) == before and not hasattr(target, name)


@pytest.mark.parametrize("seam", CLASS_SEAMS)
def test_inherited_method_leaves_nothing_behind_in_the_subclass(seam):
    install, uninstall, name, ref = CLASS_SEAMS[seam]
    Base = make_class("Base", name)
    Sub = make_class("Sub", None, Base)
    before, original = (held(Base), held(Sub)), vars(Base)[name]
    install(Sub)
    assert name in vars(Sub) and vars(Base)[name] is original
    if ref is not None:
        assert vars(Sub)[ref] is original and ref not in vars(Base)
    uninstall(Sub)
    assert name not in vars(Sub) and (ref is None or ref not in vars(Sub)) and held(Sub) == before[1]
    install(Base)                                       # a later patch of the base class reaches the subclass
    try:
        assert getattr(Sub, name) is vars(Base)[name] is not original
        assert type(Sub()).__dict__.get(name) is None
    finally:
        uninstall(Base)
    assert (held(Base), held(Sub)) == before and Sub().__getattribute__(name)() == "Base"


@pytest.mark.parametrize("undo", ["base_first", "sub_first"])
@pytest.mark.parametrize("do", ["base_first", "sub_first"])
@pytest.mark.parametrize("seam", CLASS_SEAMS)
def test_base_and_subclass_each_get_their_own_method_back(seam, do, undo):
    install, uninstall, name, ref = CLASS_SEAMS[seam]
    Base = make_class("Base", name)
    Sub = make_class("Sub", name, Base)
    before = (held(Base), held(Sub))
    for cls in ((Base, Sub) if do == "base_first" else (Sub, Base)):
        install(cls)
    if ref is not None:
        assert vars(Base)[ref] is before[0][name] and vars(Sub)[ref] is before[1][name]
    for cls in ((Base, Sub) if undo == "base_first" else (Sub, Base)):
        uninstall(cls)
    assert (held(Base), held(Sub)) == before
    assert getattr(Base(), name)() == "Base" and getattr(Sub(), name)() == "Sub"


@pytest.mark.parametrize("sub_owns", [True, False])
@pytest.mark.parametrize("undo", ["marshalling_first", "nodes_first"])
def test_two_modules_on_one_hierarchy(undo, sub_owns):
    Base = make_class("Base", GG)
    Sub = make_class("Sub", GG if sub_owns else None, Base)
    before = (held(Base), held(Sub))
    marshalling.install(Base)
    nodes.install(Sub)
    assert vars(Base)[GG] is marshalling.get_gaussians_lazy and vars(Sub)[GG] is nodes.rigid_get_gaussians
    assert vars(Sub)[REF] is (before[1][GG] if sub_owns else marshalling.get_gaussians_lazy)
    if undo == "nodes_first":
        nodes.uninstall()                               # no argument: this module's targets only
        assert vars(Base)[GG] is marshalling.get_gaussians_lazy and vars(Base)[REF] is before[0][GG] and held(Sub) == before[1]
        marshalling.uninstall(Base)
    else:
        marshalling.uninstall(Base)
        assert held(Base) == before[0] and vars(Sub)[GG] is nodes.rigid_get_gaussians
        nodes.uninstall()
    assert (held(Base), held(Sub)) == before
    assert Base().get_gaussians() == "Base" and Sub().get_gaussians() == ("Sub" if sub_owns else "Base")


def test_nodes_still_choose_the_form_by_get_deformation():
    Rigid = make_class("Rigid", GG)
    Deformable = type("Deformable", (Rigid,), {GG: lambda self, cam: "Deformable", "get_deformation": lambda self, **kwargs: None})
    before = (held(Rigid), held(Deformable))
    nodes.install(Rigid)
    nodes.install(Deformable)
    try:
        assert vars(Rigid)[GG] is nodes.rigid_get_gaussians and vars(Deformable)[GG] is nodes.deformable_get_gaussians
        assert vars(Rigid)[REF] is before[0][GG] and vars(Deformable)[REF] is before[1][GG]
    finally:
        nodes.uninstall(Rigid, Deformable)
    assert (held(Rigid), held(Deformable)) == before


def test_pseudo_lidar_still_sets_the_names_the_module_defines_else_all_four():
    some, none = make_target("pseudo_lidar"), make_target("pseudo_lidar", own=False)
    before = held(some)
    pseudo_lidar.install(some)
    pseudo_lidar.install(none)
    assert set(vars(some)) == set(before) and some.pto_ang_map is pseudo_lidar.pto_ang_map
    assert {n for n in vars(none) if not n.startswith("__")} == {"depth_map_to_lidar_points", "pto_ang_map", "pto_ang_map_vertical",
                                                                 "gen_sparse_points"}
    pseudo_lidar.uninstall(some, none)
    assert held(some) == before and not hasattr(none, "pto_ang_map")


@pytest.mark.parametrize("seam", SEAMS)
def test_installing_twice_keeps_the_first_former_value(seam):
    install, uninstall, name, ref = SEAMS[seam]
    target = make_target(seam)
    before, original = held(target), vars(target)[name]
    install(target)
    install(target)
    if ref is not None:
        assert vars(target)[ref] is original
    uninstall(target)
    assert vars(target)[name] is original and held(target) == before


@pytest.mark.parametrize("seam", MODULE_SEAMS)
def test_a_former_value_of_none_is_put_back_as_none(seam):
    install, uninstall, name, _ = MODULE_SEAMS[seam]
    target = make_target(seam)
    setattr(target, name, None)
    install(target)
    assert getattr(target, name) is not None
    uninstall()
    assert name in vars(target) and getattr(target, name) is None


@pytest.mark.parametrize("seam", SEAMS)
def test_uninstall_without_arguments_leaves_the_other_modules_patches(seam):
    install, uninstall, name, _ = SEAMS[seam]
    others = {k: make_target(k) for k in SEAMS if k != seam and not {k, seam} <= {"lidar", "lidar_module"}}
    mine = [make_target(seam), make_target(seam, own=False)]
    before = [held(t) for t in mine]
    originals = {k: vars(t)[SEAMS[k][2]] for k, t in others.items()}
    for k, t in others.items():
        SEAMS[k][0](t)
    for t in mine:
        install(t)
    try:
        uninstall()
        assert [held(t) for t in mine] == before
        for k, t in others.items():
            assert vars(t)[SEAMS[k][2]] is not originals[k], k
    finally:
        for k, t in others.items():
            SEAMS[k][1](t)
    for k, t in others.items():
        assert vars(t)[SEAMS[k][2]] is originals[k], k


class _Cfg:
    use_deformgs_for_nonrigid = False


@pytest.mark.parametrize("seam", WITH_REFERENCE)
def test_an_unpatched_subclass_of_a_patched_class_reaches_the_former_method(seam):
    """The CPU fallbacks call ``type(self)._bds_reference_...(self, ...)``: for an instance of a subclass that was never installed the
    attribute resolves, through inheritance, to the former method of the class that was."""
    install, uninstall, name, ref = CLASS_SEAMS[seam]
    Base = make_class("Base", name)
    original = vars(Base)[name]
    install(Base)
    try:
        Sub = make_class("Sub", None, Base)
        obj = Sub()
        assert ref not in vars(Sub) and getattr(type(obj), ref) is original
        obj._means, obj.sh_degree, obj.ctrl_cfg, obj.step = torch.zeros(2, 3), 0, _Cfg(), 0      # a model on the CPU
        if seam != "marshalling":                       # (marshalling has no CPU fallback: its method defers, whatever the device)
            args = (torch.zeros(2, 3), torch.zeros(2, 1)) if seam == "deform" else (None,)      # (x, t) or (cam)
            assert getattr(obj, name)(*args) == "Base"
    finally:
        uninstall(Base)
    assert getattr(Sub(), name)() == "Base" and not hasattr(Sub, ref)


def test_no_seam_bookkeeping_outside_the_patch_module():
    for module in (deform, geometry, init, lidar, marshalling, nodes, pixels, pseudo_lidar, pvg):
        assert not hasattr(module, "_INSTALLED") and not hasattr(module, "_MISSING"), module.__name__
        assert type(module._SEAM).__name__ == "Seam" and callable(module.install) and callable(module.uninstall)
    assert len({id(m._SEAM) for m in (deform, geometry, init, lidar, marshalling, nodes, pixels, pseudo_lidar, pvg)}) == 9
