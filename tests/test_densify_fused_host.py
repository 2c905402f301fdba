"""The fused densification surface (mygauhuman_amd.densify, csrc/densify.hip) as far as it can be checked without a GPU:
the entry points are declared and bound, every operation has the opt-in `fused` keyword with the old path as its default, and
fused=True on CPU tensors is an error that names the HIP device (there is no CPU path and no quiet fall-back)."""
import inspect
import os

import pytest
import torch

from mygauhuman_amd import _lib, build, densify
from tests.test_densify_cpu import make_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("gsr_kl_pairs", "gsr_densify_select", "gsr_densify_plan_workspace_bytes", "gsr_densify_plan", "gsr_build_rows")
OPERATIONS = ("prune_points", "densify_and_clone", "densify_and_split", "kl_densify_and_clone", "kl_densify_and_split", "kl_merge",
              "densify_and_prune", "kl_to_nearest")


def test_entry_points_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in _lib.TABLE and hasattr(_lib.lib, name), name
    assert "densify.hip" in [s for s, _ in build.SOURCES]
    assert os.path.exists(os.path.join(ROOT, "mygauhuman_amd", "csrc", "densify.hip"))
    # the size query runs on the host: a byte per row for the merge's marks and two counters per block of 256 rows
    assert _lib.lib.gsr_densify_plan_workspace_bytes(0) >= 0
    assert _lib.lib.gsr_densify_plan_workspace_bytes(4099) >= 4099 + 2 * 4 * 17
    # constants of the header and of the binding agree
    for c in ("DENSIFY_CLONE", "DENSIFY_SPLIT", "DENSIFY_MERGE", "PLAN_PRUNE", "PLAN_CLONE", "PLAN_SPLIT", "PLAN_MERGE", "BUILD_MOVE",
              "BUILD_CHILDREN", "BUILD_MERGE", "ROW_COPY", "ROW_XYZ", "ROW_LOG_SCALING", "ROW_ROTATION", "ROW_MEAN"):
        assert f"GSR_{c} = {getattr(_lib, c)}" in header, c


def test_bad_arguments_are_refused_before_anything_is_launched():
    for args in ((-1, None, None, None, None, None, None),):
        assert _lib.lib.gsr_kl_pairs(*args) == -1
    assert _lib.lib.gsr_densify_select(4, 7, None, 0, None, None, 0.0, 0.0, 0.0, None, None) == -1
    assert _lib.lib.gsr_densify_plan(4, 9, 2, None, None, None, None, None, 0, None) == -1
    assert _lib.lib.gsr_build_rows(0, None, None, None, None, None, 4, None, 4, 0, 0, None, None, 1.0, None, None) == -1
    assert b"gsr_build_rows" in _lib.lib.gsr_last_error()


def test_fused_keyword_exists_and_defaults_to_the_old_path():
    for name in OPERATIONS:
        p = inspect.signature(getattr(densify, name)).parameters
        assert "fused" in p and p["fused"].default is False, name
    assert inspect.signature(densify.densify_and_prune).parameters["kl_threshold"].default is None
    for name in ("device_select", "device_plan", "apply_device_plan", "kl_pairs"):
        assert callable(getattr(densify, name)), name
    p = inspect.signature(densify.apply_device_plan).parameters
    assert list(p)[:4] == ["model", "plan", "header", "reset_stats"] and p["children"].default is None and p["merge"].default is None
    p = inspect.signature(densify.device_plan).parameters
    assert list(p) == ["kind", "flags", "N", "pairs"] and p["N"].default == 2 and p["pairs"].default is None


def _cpu_model(P=32):
    class M:
        percent_dense = 0.01
        get_scaling = property(lambda self: torch.exp(self._scaling))
        get_opacity = property(lambda self: torch.sigmoid(self._opacity))
    m = M()
    st = make_state(P, 3)
    for g in densify.GROUPS:
        setattr(m, densify.ATTR[g], torch.nn.Parameter(torch.from_numpy(st["params"][g])))
    densify.training_setup(m, {g: 1e-3 for g in densify.GROUPS})
    return m


def test_fused_on_cpu_tensors_raises_and_names_the_device():
    m = _cpu_model()
    P = m._xyz.shape[0]
    grads = torch.full((P, 1), 1e-3)
    mask = torch.zeros(P, dtype=torch.bool)
    calls = [lambda: densify.prune_points(m, mask, fused=True),
             lambda: densify.densify_and_clone(m, grads, 4e-4, 2.0, fused=True),
             lambda: densify.densify_and_split(m, grads, 4e-4, 2.0, fused=True),
             lambda: densify.kl_densify_and_clone(m, grads, 4e-4, 2.0, fused=True),
             lambda: densify.kl_densify_and_split(m, grads, 4e-4, 2.0, fused=True),
             lambda: densify.kl_merge(m, grads, 4e-4, 2.0, fused=True),
             lambda: densify.kl_to_nearest(m, fused=True),
             lambda: densify.densify_and_prune(m, 4e-4, 0.005, 2.0, 20, fused=True),
             lambda: densify.device_plan("prune", mask),
             lambda: densify.device_select("clone", grads, m.get_scaling.detach(), 4e-4, 0.02),
             lambda: densify.kl_pairs(m._xyz, m._rotation, m._scaling, torch.zeros((P, 2), dtype=torch.int32)),
             lambda: densify.apply_device_plan(m, torch.zeros(P, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), False)]
    for fn in calls:
        with pytest.raises(RuntimeError, match="HIP"):
            fn()
    assert m._xyz.shape[0] == P  # nothing was touched
