"""CPU-only tests of the environment light's own share of a PBR step (CubemapLight.grey_envmap, pbr.env_tv_loss, pbr.view_dirs;
csrc/pbr.hip): the float64 restatement the GPU tests compare with (tests/env_light_reference.py) is pinned to the
fixture the reference's own export_envmap made and to the camera's own matrices; the library exports the entry points and
validates their arguments without a device; every host-side error is raised with CPU tensors."""
import os

import numpy as np
import pytest
import torch

from tests import env_light_reference as E
from tests import pbr_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_SYMBOLS = ("gsr_pbr_env_grey", "gsr_pbr_env_tv_workspace_floats", "gsr_pbr_env_tv_forward", "gsr_pbr_env_tv_backward",
               "gsr_pbr_view_dirs")


def test_restated_grey_map_matches_the_reference_fixture():
    """The grey weights applied in numpy to the clamped envmap the reference exported from base16 = the restatement's grey map."""
    stored = np.load(os.path.join(GOLDEN, "pbr_light.npz"))["b16_envmap"]
    assert stored.shape == (16, 32, 3)
    want = (np.clip(stored.astype(np.float64), 0.0, 1.0) * np.array([0.2989, 0.587, 0.114])).sum(-1)[None]
    got = E.grey_envmap(R.fixture_inputs()["base16"], (16, 32))
    assert got.shape == (1, 16, 32)
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    assert want.min() > 0.05 and want.max() < 1.0  # (a map of zeros would agree with anything clamped)


def test_restated_view_dirs_match_the_camera_matrices():
    from mygauhuman_amd import baking, cameras
    H, W = 5, 7
    cam = cameras.look_at_camera(W, H, [0.4, -0.3, -2.5], [0.1, 0.2, 0.3])
    wvt = np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4)  # ViewCamera.world_view_transform (row-vector convention)
    rays = baking.get_canonical_rays(H, W, 0.5, 0.4).numpy().astype(np.float64)
    rays[3] = 0.0
    c2w = np.linalg.inv(wvt.T)
    unit = rays / np.maximum(np.linalg.norm(rays, axis=1, keepdims=True), 1e-12)
    want = np.stack([-(c2w[:3, :3] @ u) for u in unit]).reshape(H, W, 3)
    got = E.view_dirs(rays, wvt, H, W)
    assert np.abs(got - want).max() <= 1e-12
    assert np.all(got.reshape(-1, 3)[3] == 0.0)
    norms = np.linalg.norm(np.delete(got.reshape(-1, 3), 3, axis=0), axis=1)
    assert np.abs(norms - 1.0).max() <= 1e-6  # a rigid camera (its matrix holds float32 values): unit directions
    # the centre ray looks along the camera's forward axis: the view direction points back at the eye
    fwd = np.array([0.1, 0.2, 0.3]) - np.array([0.4, -0.3, -2.5])
    centre = E.view_dirs(np.array([[0.0, 0.0, 1.0]]), wvt, 1, 1)[0, 0]
    assert np.abs(centre + fwd / np.linalg.norm(fwd)).max() <= 1e-6


def test_symbols_are_exported_and_validate_without_a_device():
    from mygauhuman_amd import _lib
    lib = _lib.lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.gsr_pbr_env_tv_workspace_floats(256, 512) == 256 * 512 * 3 + 2 * 512   # e and two partial sums per 256 samples
    assert lib.gsr_pbr_env_tv_workspace_floats(9, 14) == 9 * 14 * 3 + 2
    assert lib.gsr_pbr_env_tv_workspace_floats(0, 14) == 0
    one = 4096  # any non-null address: the checks come before any launch
    assert lib.gsr_pbr_env_grey(0, one, 4, one, one, None) == -1 and b"gsr_pbr_env_grey" in lib.gsr_last_error()
    assert lib.gsr_pbr_env_grey(32, None, 4, one, one, None) == -1
    assert lib.gsr_pbr_env_grey(32, one, 0, None, None, None) == 0
    assert lib.gsr_pbr_env_tv_forward(32, one, 1, 8, one, one, one, None) == -1 and b"h, w >= 2" in lib.gsr_last_error()
    assert lib.gsr_pbr_env_tv_forward(32, one, 8, 8, one, None, one, None) == -1
    assert lib.gsr_pbr_env_tv_backward(32, 8, 8, one, one, one, one, 3, None) == -1 and b"reduce" in lib.gsr_last_error()
    assert lib.gsr_pbr_env_tv_backward(32, 8, 1, one, one, one, one, 0, None) == -1
    # a base whose gradient does not fit in LDS has only the window reduction
    assert lib.gsr_pbr_env_tv_backward(128, 8, 8, one, one, one, one, _lib.ENV_TV_WHOLE, None) == -1
    assert b"does not fit" in lib.gsr_last_error()
    assert lib.gsr_pbr_view_dirs(-1, one, one, one, None) == -1
    assert lib.gsr_pbr_view_dirs(4, one, None, one, None) == -1 and b"world_view_transform" in lib.gsr_last_error()
    assert lib.gsr_pbr_view_dirs(0, None, one, None, None) == 0


def test_names_are_exported_from_the_pbr_package():
    import mygauhuman_amd.pbr as pbr
    for name in ("env_tv_loss", "view_dirs", "CubemapLight"):
        assert name in pbr.__all__ and hasattr(pbr, name)
    assert callable(pbr.CubemapLight.grey_envmap)


def test_grey_envmap_errors_are_raised_on_the_host():
    from mygauhuman_amd.pbr import CubemapLight
    light = CubemapLight(base_res=8, device="cpu")
    for res in ([0, 32], [16, -1], [16]):
        with pytest.raises(ValueError):
            light.grey_envmap(res)
    with pytest.raises(RuntimeError, match="HIP device"):
        light.grey_envmap([16, 32])
    for shape in ((6, 8, 8, 1), (6, 8, 4, 3), (5, 8, 8, 3), (6, 8, 8)):
        bad = CubemapLight(base_res=8, device="cpu")
        bad.base = torch.nn.Parameter(torch.zeros(shape))
        with pytest.raises(NotImplementedError):
            bad.grey_envmap()


def test_env_tv_loss_errors_are_raised_on_the_host():
    from mygauhuman_amd.pbr import CubemapLight, env_tv_loss
    base = torch.rand(6, 8, 8, 3)
    dirs = torch.randn(4, 5, 3)
    for h, w in ((1, 5), (4, 1), (1, 1)):
        with pytest.raises(ValueError, match="2 x 2"):
            env_tv_loss(base, torch.randn(h, w, 3))
    for bad in (torch.rand(6, 8, 8, 1), torch.rand(6, 8, 4, 3), torch.rand(1, 6, 8, 8, 3), torch.rand(5, 8, 8, 3)):
        with pytest.raises(ValueError, match="cube map"):
            env_tv_loss(bad, dirs)
    for bad in (torch.randn(4, 5, 2), torch.randn(2, 4, 5, 3), torch.randn(20, 3)):
        with pytest.raises(ValueError, match="dirs"):
            env_tv_loss(base, bad)
    with pytest.raises(NotImplementedError, match="directions"):
        env_tv_loss(base, dirs.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="HIP device"):
        env_tv_loss(base, dirs)
    with pytest.raises(RuntimeError, match="HIP device"):
        env_tv_loss(base, dirs[None])
    with pytest.raises(RuntimeError, match="HIP device"):   # a light means its base
        env_tv_loss(CubemapLight(base_res=8, device="cpu"), dirs)


def test_view_dirs_errors_are_raised_on_the_host():
    from mygauhuman_amd.pbr import view_dirs
    rays, m = torch.randn(12, 3), torch.eye(4)
    with pytest.raises(ValueError, match="canonical_rays"):
        view_dirs(rays, m, 3, 5)
    with pytest.raises(ValueError, match="canonical_rays"):
        view_dirs(torch.randn(12, 2), m, 3, 4)
    for bad in (torch.eye(3), torch.eye(4, dtype=torch.float64), torch.zeros(1, 4, 4)):
        with pytest.raises(ValueError, match="world_view_transform"):
            view_dirs(rays, bad, 3, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        view_dirs(rays, m, 3, 4)
