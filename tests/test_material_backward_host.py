"""CPU-only tests of the materials-only backward (csrc/blend_colors_bwd.hip): the host-side argument checks of
gsr_rasterize_backward_colors, profile stage 6, the switches around render(geometry_grad=...), and the yardsticks of
tests/test_gpu_material_backward.py held against each other -- the CPU oracle's dL_dcolors against the float64 restatement on
every scene of tests/material_backward_cases.py, inside the bound the GPU test uses."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from mygauhuman_amd import _lib
from tests import material_backward_cases as mc
from tests import scenes, util
from tests.test_raster_reference_host import rel_err

FAKE = 4096  # a non-null "device pointer": every call below is refused before anything could read it


def _colors(*args):
    _lib.call("gsr_rasterize_backward_colors", None, *args, stream=0)


@pytest.mark.parametrize("args", [
    (-1, 0, 16, 16, FAKE, FAKE, FAKE, None, None, 0, None, None, 0),           # negative P
    (1, -1, 16, 16, FAKE, FAKE, FAKE, None, None, 0, None, None, 0),           # negative R
    (1, 1, -16, 16, FAKE, FAKE, FAKE, None, None, 0, None, None, 0),           # negative width
    (1, 1, 16, -16, FAKE, FAKE, FAKE, None, None, 0, None, None, 0),           # negative height
    (1, 1, 16, 16, FAKE, FAKE, FAKE, None, None, 3, None, None, 0),            # n_extra outside {0, 18}
    (1, 1, 16, 16, FAKE, FAKE, FAKE, None, None, 17, None, None, 0),
    (1, 1, 16, 16, FAKE, FAKE, FAKE, FAKE, None, 0, None, None, 0),            # dL_dpix without dL_dcolor
    (1, 1, 16, 16, FAKE, FAKE, FAKE, None, None, 18, None, FAKE, 0),           # n_extra = 18 without the pointer array
    (1, 1, 16, 16, None, FAKE, FAKE, None, None, 0, None, None, 0),            # a null buffer
], ids=["P", "R", "width", "height", "n_extra3", "n_extra17", "dL_dcolor", "dL_dout_extra", "geom_buffer"])
def test_colors_entry_refuses_bad_arguments_on_the_host(args):
    with pytest.raises(_lib.GsrError, match=r"gsr_rasterize_backward_colors failed \(-1\)"):
        _colors(*args)


def test_colors_entry_refuses_a_missing_dL_dextra():
    six = (C.c_void_p * 6)(*([None] * 6))
    with pytest.raises(_lib.GsrError, match=r"gsr_rasterize_backward_colors failed \(-1\).*dL_dextra"):
        _colors(1, 1, 16, 16, FAKE, FAKE, FAKE, None, None, 18, six, None, 0)


def test_colors_entry_with_nothing_to_do_is_ok():
    _colors(0, 0, 16, 16, None, None, None, None, None, 0, None, None, 0)  # P = 0: nothing is launched, nothing is read


def test_profile_stage_six():
    ms, n = C.c_double(-1.0), C.c_long(-1)
    assert _lib.lib.gsr_profile_read(6, C.byref(ms), C.byref(n)) == _lib.GSR_OK
    assert ms.value == 0.0 and n.value == 0
    assert _lib.lib.gsr_profile_read(7, C.byref(ms), C.byref(n)) == -1
    assert _lib.PROF_STAGES[6] == "blend_bwd_colors" and len(_lib.PROF_STAGES) == 7
    assert _lib.PROF_STAGES[:6] == ["preprocess_fwd", "scan", "binning", "blend_fwd", "blend_bwd", "preprocess_bwd"]


def test_install_dropin_sets_the_switch():
    import sys
    import mygauhuman_amd
    from mygauhuman_amd import gaussian_renderer as gr
    saved = dict(sys.modules)
    try:
        assert gr.GEOMETRY_GRAD is True
        mygauhuman_amd.install_dropin()
        assert gr.GEOMETRY_GRAD is True
        mygauhuman_amd.install_dropin(materials_backward=True)
        assert gr.GEOMETRY_GRAD == "auto"
    finally:
        gr.GEOMETRY_GRAD = True
        for k in set(sys.modules) - set(saved):
            del sys.modules[k]
        sys.modules.update(saved)


def test_geometry_frozen_reads_the_leaves_and_the_decoders():
    from mygauhuman_amd import gaussian_renderer as gr
    leaf = lambda on: torch.zeros(2, 3, requires_grad=on)  # noqa: E731
    m = types.SimpleNamespace(motion_offset_flag=False, pose_decoder=torch.nn.Linear(2, 2), lweight_offset_decoder=None,
                              _normal=leaf(True), _albedo=leaf(True), _roughness=leaf(True), **{n: leaf(False) for n in gr.GEOMETRY_LEAVES})
    assert gr.geometry_frozen(m)          # the decoders do not count without motion_offset_flag; the materials never do
    m.motion_offset_flag = True
    assert not gr.geometry_frozen(m)
    for p in m.pose_decoder.parameters():
        p.requires_grad_(False)
    assert gr.geometry_frozen(m)
    for n in gr.GEOMETRY_LEAVES:
        getattr(m, n).requires_grad_(True)
        assert not gr.geometry_frozen(m), n
        getattr(m, n).requires_grad_(False)


def test_render_refuses_what_the_short_path_cannot_carry():
    """Raised at call time, before anything touches a device."""
    from mygauhuman_amd import gaussian_renderer as gr
    pipe = types.SimpleNamespace(separate_feature_passes=False)
    with pytest.raises(ValueError, match="fused_loss"):
        gr.render(30001, None, None, pipe, None, fused_loss=object(), geometry_grad=False)
    pipe.separate_feature_passes = True
    with pytest.raises(ValueError, match="separate_feature_passes"):
        gr.render(30001, None, None, pipe, None, geometry_grad=False)
    with pytest.raises(ValueError, match="'auto'"):
        gr.render(30001, None, None, pipe, None, geometry_grad="sometimes")


def test_view_parallel_wrappers_refuse_the_short_path():
    from mygauhuman_amd import parallel
    with pytest.raises(ValueError, match="geometry_grad"):
        parallel.ViewParallelRender.__call__(object.__new__(parallel.ViewParallelRender), 1, None, None, geometry_grad=False)
    with pytest.raises(ValueError, match="geometry_grad"):
        parallel.ViewParallelStep.__call__(object.__new__(parallel.ViewParallelStep), None, None, None, None, geometry_grad=False)


@pytest.mark.parametrize("name", mc.NAMES)
def test_oracle_agrees_with_float64_inside_the_gpu_tests_bound(oracle, name, capsys):
    """The yardstick alone stays inside the bound the GPU test uses: no element of the oracle's dL_dcolors is beyond tol of the
    float64 restatement, for every gradient image of every scene; and the scenes are what they are meant to be."""
    c = mc.case(oracle, name)
    worst = 0.0
    for i in mc.LIVE_TRIPLES + (mc.MAIN,):
        _, t64, _ = mc.bounds(name, c.want[i].size)
        util.assert_close(f"{name} image {i}: oracle vs float64", c.want[i], c.want64[i], tol=t64, max_bad_frac=0.0)
        assert np.abs(c.want64[i]).max() > 0
        worst = max(worst, rel_err(c.want[i], c.want64[i]))
    with capsys.disabled():
        print(f"\n{name}: worst relative error of the oracle's dL_dcolors {worst:.2e}, keep {c.keep.mean():.3f}, lists "
              f"{c.lists.min()}..{c.lists.max()} (mean {c.lists.mean():.0f}), n_contrib <= {c.n_contrib_max}, culled {c.culled}")
    assert worst < (1e-4 if name == "needle" else 1e-5)
    assert c.keep.mean() >= mc.MIN_KEEP.get(name, mc.MIN_KEEP_DEFAULT)
    if name in scenes.FAMILIES:
        assert 34 <= c.lists.max() <= 139 and c.lists.min() > 0
        if name == "opaque":   # the walks end at T < 1e-4 under the 0.99 clamp: before the end of the list
            assert c.n_contrib_max < c.lists.max()
    else:
        long_tiles = c.lists[c.lists > 1024]
        assert len(long_tiles) == 4 and long_tiles.min() >= 1300 and c.lists.max() <= 1607
        if name == "stack_tail":
            assert (c.lists == 0).any() and c.culled == 0 and c.P == 1600
        else:
            assert 190 <= c.lists.mean() <= 196 and c.culled == 116 and not (c.lists == 0).any()
            assert c.n_contrib_max == (1607 if name == "stack_translucent" else 1601)
