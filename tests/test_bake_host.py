"""CPU tests of the occlusion bake's host side (mygauhuman_amd.baking): the restatements against the fixture made by the reference's
own baking.py (tests/golden/make_golden_bake.py), install_dropin(bake=True), and the refusals."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import bake_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = R.SCENES


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "bake_scenes.npz"))


@pytest.mark.parametrize("name", SCENES)
def test_fixture_visibility_is_defined_where_a_gaussian_faces_it(fx, name):
    """The fixture stores the reference's occlusion as vis [C, 512] (occlusion = dot_map * vis[cell]); vis is NaN exactly where no
    Gaussian of the cell faces the direction, by the hemisphere mask restated here from the rebuilt normals."""
    from mygauhuman_amd import baking
    means, scales, rots, opac, n = R.scene(name)
    cell = fx[f"{name}/pc_grid_indices"].astype(np.int64)
    vis = fx[f"{name}/vis"]
    _, dirs = baking.get_envmap_dirs()
    mask = R.hemisphere_mask(dirs, n).reshape(len(n), -1)
    seen = np.zeros(vis.shape, bool)
    np.logical_or.at(seen, cell, mask)
    np.testing.assert_array_equal(~np.isnan(vis), seen)
    assert np.nanmin(vis) < 1e-3 and np.nanmax(vis) <= 1.0


@pytest.mark.parametrize("name", SCENES)
def test_pc_to_grid_and_cube_cameras_match_reference(fx, name):
    from mygauhuman_amd import baking
    centres, sizes, inv, uniq = baking.pc_to_grid(torch.from_numpy(R.scene(name)[0]), 10)
    np.testing.assert_array_equal(inv.numpy(), fx[f"{name}/pc_grid_indices"])
    # (the reference ran on the CPU, where torch divides by the resolution; pc_to_grid multiplies by 0.1f as torch's GPU kernels do)
    np.testing.assert_allclose(centres.numpy(), fx[f"{name}/grid_centers"], rtol=1e-6, atol=1e-7)
    k = R.CAMERA_CELLS
    views, projs, campos = baking.cube_cameras(torch.from_numpy(fx[f"{name}/grid_centers"][:k]))
    np.testing.assert_array_equal(views.numpy(), fx[f"{name}/views"])
    np.testing.assert_allclose(projs.numpy(), fx[f"{name}/projs"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(campos.numpy(), fx[f"{name}/grid_centers"][:k, None, :].repeat(6, 1), rtol=1e-6, atol=1e-7)


def test_nearest_texel_restatements_agree():
    from mygauhuman_amd import baking
    _, dirs = baking.get_envmap_dirs()
    ours = baking.cube_nearest_texel(dirs).reshape(-1).numpy()
    np.testing.assert_array_equal(ours, R.nearest_texel(dirs.reshape(-1, 3).numpy(), 32))
    assert ours.min() >= 0 and ours.max() < 6 * 32 * 32
    rng = np.random.default_rng(0)
    d = rng.normal(0, 1, (20000, 3)).astype(np.float32)
    d[:6] = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d[6] = 0
    d[7] = [1, 1, 1]  # a cube corner: x wins
    np.testing.assert_array_equal(baking.cube_nearest_texel(torch.from_numpy(d)).numpy(), R.nearest_texel(d, 32))
    assert R.nearest_texel(d[6:7], 32)[0] == -1
    assert R.nearest_texel(d[7:8], 32)[0] // 1024 == 0


def test_cube_face_texel_convention():
    """Texel (f, i, j) of the stacked cube is pixel (x = j, y = i) of face f's camera: a direction through pixel (x, y) of face f's
    view lands on texel (f, y, x)."""
    from mygauhuman_amd import baking
    views, _, _ = baking.cube_cameras(torch.zeros((1, 3)))
    rays = baking.get_canonical_rays(32, 32, 1.0, 1.0)  # [H * W, 3] camera space, pixel order y-major
    for f in range(6):
        R_wc = views[0, f, :3, :3]  # row-vector convention: p_view = p_world @ R_wc
        world = rays @ R_wc.T
        texel = baking.cube_nearest_texel(world)
        np.testing.assert_array_equal(texel.numpy(), f * 1024 + np.arange(1024))


def test_install_dropin_bake_registers_baking():
    import mygauhuman_amd
    from mygauhuman_amd import baking
    from mygauhuman_amd import gaussian_renderer as gr
    saved = sys.modules.get("baking")
    try:
        sys.modules.pop("baking", None)
        mygauhuman_amd.install_dropin()
        assert "baking" not in sys.modules and gr.BAKE is False
        mygauhuman_amd.install_dropin(bake=True)
        assert sys.modules["baking"] is baking and gr.BAKE is True
        from baking import bake_set, get_canonical_rays, get_envmap_dirs, pc_to_grid  # noqa: F401
    finally:
        gr.BAKE = False
        if saved is None:
            sys.modules.pop("baking", None)
        else:
            sys.modules["baking"] = saved


@pytest.mark.parametrize("H,W", [(256, 512), (16, 16), (32, 32)])
def test_bake_set_refuses_other_sizes(H, W):
    from mygauhuman_amd import baking
    view = types.SimpleNamespace(occlusion=None)
    with pytest.raises(ValueError, match="16, 32"):
        baking.bake_set(view, None, torch.zeros((4, 3)), torch.zeros((4, 3)), H, W)
    assert view.occlusion is None


def test_fused_bake_needs_a_device():
    from mygauhuman_amd import baking
    g = types.SimpleNamespace(get_scaling=torch.ones((4, 3)), get_rotation=torch.ones((4, 4)), get_opacity=torch.ones((4, 1)))
    with pytest.raises(RuntimeError, match="HIP device"):
        baking.bake_set(types.SimpleNamespace(), g, torch.rand((4, 3)), torch.rand((4, 3)), 16, 32)


def test_env_occlusion_refuses_colour_maps():
    from mygauhuman_amd import baking
    with pytest.raises(ValueError, match="grey"):
        baking.env_occlusion(torch.zeros((4, 16, 32, 1)), torch.zeros((3, 16, 32)))


def test_pc_to_grid_zero_extent_rule():
    from mygauhuman_amd import baking
    pts = torch.tensor([[0.5, 0.0, 1.0], [0.5, 1.0, 2.0], [0.5, 0.55, 1.0]])
    centres, sizes, inv, uniq = baking.pc_to_grid(pts, 10)
    assert uniq[:, 0].tolist() == [0, 0, 0]
    assert float(sizes[0]) == 0.0 and inv.tolist() == [0, 2, 1]


def test_bake_tuning_key():
    from mygauhuman_amd import _lib
    _lib.set_tuning("bake_batch_cells", 5)
    _lib.set_tuning("bake_batch_cells", 0)
    with pytest.raises(_lib.GsrError):
        _lib.set_tuning("bake_batch_cells", -1)
