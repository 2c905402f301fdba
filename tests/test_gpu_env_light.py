"""The environment light's own share of a PBR step on the GPU (csrc/pbr.hip behind CubemapLight.grey_envmap, pbr.env_tv_loss and
pbr.view_dirs) against the float64 restatement (tests/env_light_reference.py), the fixture the reference's own
export_envmap made, and the torch compositions these calls replace; then all three recorded into one graph, and guard bands
around everything they write."""
import os
import types

import numpy as np
import pytest
import torch

from tests import env_light_reference as E
from tests import pbr_reference as R
from tests import util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GREY = (0.2989, 0.587, 0.114)
# face edges, cube corners, texel-aligned and zero directions (the list test_gpu_pbr.py plants)
SPECIAL = np.array([[1, 1, 0], [1, -1, 0], [0, 1, 1], [0, -1, -1], [1, 0, -1], [-1, 0, 1], [1, 1, 1], [-1, 1, -1],
                    [1, -1, -1], [-1, -1, 1], [0, 0, 1], [0, 0, -1], [1, 0.5, 0.25], [0, 0, 0]], np.float64)


def _g(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _r(x):
    """The float64 restatement's copy of what the kernel sees (float32 values)."""
    return torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))


def _np(t):
    return t.detach().cpu().numpy()


def _base(N, seed=0):
    """A light with values outside [0, 1] on about a third of its texels, so that the grey map's clamp matters."""
    return np.random.default_rng(100 * N + seed).uniform(-0.3, 1.4, (6, N, N, 3)).astype(np.float32)


def _light(base):
    from mygauhuman_amd.pbr import CubemapLight
    light = CubemapLight(base_res=base.shape[1])
    with torch.no_grad():
        light.base.copy_(_g(base))
    return light


def _grey_composition(light, res):
    """train.py:195-198 as it stands without the fused call: export_envmap, the clamp, the grey weights."""
    with torch.no_grad():
        img = light.export_envmap(return_img=True, res=res).permute(2, 0, 1).clamp(0.0, 1.0)
        return (GREY[0] * img[0] + GREY[1] * img[1] + GREY[2] * img[2])[None]


# ---- the grey environment map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [[16, 32], [9, 14], [1, 1]], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("N", [8, 32])
def test_grey_envmap_matches_restatement_and_existing_path(N, res):
    base = _base(N)
    assert (base < 0).any() and (base > 1).any()
    light = _light(base)
    got = light.grey_envmap(res)
    assert tuple(got.shape) == (1, res[0], res[1]) and got.dtype == torch.float32 and not got.requires_grad
    util.assert_close("grey", _np(got), E.grey_envmap(base, res))
    comp = _grey_composition(light, res)
    err = float((got - comp).abs().max())
    assert err <= 1e-6, f"grey_envmap against export_envmap + clamp + weights: {err:.3e}"
    # the clamp matters on this light wherever the grid has more than its one pole sample: the unclamped grey differs
    raw = light.export_envmap(return_img=True, res=res).detach()
    assert res == [1, 1] or float(((GREY[0] * raw[..., 0] + GREY[1] * raw[..., 1] + GREY[2] * raw[..., 2])[None] - got).abs().max()) > 1e-3
    assert light.base.grad is None


def test_grey_envmap_matches_reference_fixture():
    stored = np.load(os.path.join(GOLDEN, "pbr_light.npz"))["b16_envmap"]
    light = _light(np.asarray(R.fixture_inputs()["base16"], np.float32))
    util.assert_close("grey of the reference's envmap", _np(light.grey_envmap([16, 32])), E.grey_of(stored)[None])


def test_grey_envmap_out_is_written_in_place_and_the_grid_is_cached():
    light = _light(_base(32))
    out = torch.full((1, 16, 32), -7.0, device="cuda")
    got = light.grey_envmap(out=out)
    assert got.data_ptr() == out.data_ptr() and got is out
    assert torch.equal(out, light.grey_envmap([16, 32]))
    grid = light._grey_dirs[(16, 32, light.base.device)]
    light.grey_envmap([16, 32])
    assert light._grey_dirs[(16, 32, light.base.device)] is grid and len(light._grey_dirs) == 1
    with pytest.raises(ValueError, match="out"):
        light.grey_envmap([16, 32], out=torch.empty(16, 32, device="cuda"))


# ---- the environment-map TV ----------------------------------------------------------------------------------------------------
_TV_REF = {}


def _tv_reference(N, key, dirs):
    """Value and d_base of the restatement, computed once per case."""
    if (N, key) not in _TV_REF:
        b64 = _r(_base(N)).requires_grad_(True)
        v = E.env_tv_loss(b64, _r(dirs).numpy())
        v.backward()
        _TV_REF[(N, key)] = (float(v.detach()), b64.grad.numpy().copy())
    return _TV_REF[(N, key)]


def _tv_dirs(key):
    if key == "random":
        rng = np.random.default_rng(5)
        d = rng.normal(size=(17 * 23, 3))
        d[3:3 + len(SPECIAL)] = SPECIAL          # (not from index 0: the zero direction gets a neighbour on every side)
        d[40:40 + len(SPECIAL)] = SPECIAL[::-1]
        return d.reshape(17, 23, 3).astype(np.float32)
    return R.envmap_dirs(list(key)).astype(np.float32)


def _tv_check(N, key, reduce=None):
    from mygauhuman_amd.pbr import env_tv_loss
    dirs = _tv_dirs(key)
    want_v, want_g = _tv_reference(N, key, dirs)
    b = _g(_base(N)).requires_grad_(True)
    d = _g(dirs)
    v = env_tv_loss(b, d) if reduce is None else env_tv_loss(b, d, reduce=reduce)
    assert v.dim() == 0 and v.dtype == torch.float32
    v.backward()
    print(f"N {N} dirs {key} reduce {reduce}: value {float(v.detach()):.8e} (want {want_v:.8e}), "
          f"max |d_base error| {np.abs(_np(b.grad) - want_g).max():.3e} of {np.abs(want_g).max():.3e}")
    util.assert_close("tv", np.array([float(v.detach())]), np.array([want_v]))
    util.assert_close("d_base", _np(b.grad), want_g, max_bad_frac=1e-3)
    assert float(b.grad.abs().sum()) > 0
    return b, d, v


@pytest.mark.parametrize("res", [(2, 2), (9, 14), (16, 32), (64, 128)], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("N", [8, 32])
def test_env_tv_loss_matches_restatement(N, res):
    _tv_check(N, res)


def test_env_tv_loss_matches_restatement_at_the_reference_size():
    b, d, v = _tv_check(32, (256, 512))
    assert float((b.grad != 0).float().mean()) == 1.0   # every texel of the light takes a gradient at this size


@pytest.mark.parametrize("N", [8, 32])
def test_env_tv_loss_special_directions(N):
    _tv_check(N, "random")


@pytest.mark.parametrize("res", [(9, 14), (64, 128)], ids=lambda r: f"{r[0]}x{r[1]}")
@pytest.mark.parametrize("reduce", ["window", "whole"])
def test_env_tv_loss_both_reductions(reduce, res):
    from mygauhuman_amd import _lib
    _tv_check(32, res, reduce=_lib.ENV_TV_WINDOW if reduce == "window" else _lib.ENV_TV_WHOLE)


def test_env_tv_loss_base_whose_gradient_does_not_fit_in_lds():
    """N = 128: 294,912 gradient floats, eight LDS windows (the fallback path); a light given as the module."""
    from mygauhuman_amd import _lib
    from mygauhuman_amd.pbr import env_tv_loss
    _tv_check(128, (16, 32))
    light = _light(_base(128))
    d = _g(_tv_dirs((16, 32)))
    assert float(env_tv_loss(light, d[None])) == float(env_tv_loss(light.base, d))
    with pytest.raises(_lib.GsrError, match="does not fit"):
        env_tv_loss(light.base, d, reduce=_lib.ENV_TV_WHOLE).backward()


def test_env_tv_loss_matches_texture_composition_and_accumulates():
    from mygauhuman_amd.nvdiffrast.torch import texture
    from mygauhuman_amd.pbr import env_tv_loss
    d = _g(_tv_dirs("random"))
    b = _g(_base(32)).requires_grad_(True)
    e = texture(b[None], d[None], filter_mode="linear", boundary_mode="cube")[0]
    comp = ((e[1:] - e[:-1]) ** 2).mean() + ((e[:, 1:] - e[:, :-1]) ** 2).mean()
    comp.backward()
    want_g = b.grad.clone()
    b.grad = None
    v = env_tv_loss(b, d)
    (3.0 * v).backward()   # an upstream gradient other than one
    util.assert_close("tv against the composition", np.array([float(v)]), np.array([float(comp)]))
    util.assert_close("d_base against the composition", _np(b.grad), 3.0 * _np(want_g), max_bad_frac=1e-3)
    assert float(v) == float(env_tv_loss(b, d))   # the forward's sums run in a fixed order
    env_tv_loss(b, d).backward()                  # a second backward adds
    util.assert_close("accumulated d_base", _np(b.grad), 4.0 * _np(want_g), max_bad_frac=1e-3)
    assert float(b.grad.abs().sum()) > 0
    assert float(env_tv_loss(b.detach(), d)) == float(v)   # nothing to differentiate: still the value
    with pytest.raises(NotImplementedError, match="directions"):   # as texture(): no gradient for the directions, on the device too
        env_tv_loss(b, d.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="once_differentiable"):   # no double backward: it would treat d_base as a constant
        w = torch.ones((), device="cuda", requires_grad=True)   # (an upstream gradient that is itself differentiable)
        g, = torch.autograd.grad(w * env_tv_loss(b, d), b, create_graph=True)
        g.sum().backward()


# ---- view directions -----------------------------------------------------------------------------------------------------------
def _cameras():
    from mygauhuman_amd import cameras
    look = np.asarray(cameras.look_at_camera(64, 64, [0.4, -0.3, -2.5], [0.1, 0.2, 0.3])["viewmatrix"], np.float32).reshape(4, 4)
    a = 2.0 * np.eye(3) + np.array([[0.0, 0.6, 0.0], [0.0, 0.0, -0.4], [0.3, 0.0, 0.0]])   # scale 2 and a shear
    affine = np.eye(4, dtype=np.float32)
    affine[:3, :3] = a
    affine[3, :3] = [0.7, -1.1, 2.3]
    return {"look_at": look, "affine": affine}


@pytest.mark.parametrize("H,W", [(1, 1), (17, 23), (512, 512)])
@pytest.mark.parametrize("camera", ["look_at", "affine"])
def test_view_dirs_match_restatement(camera, H, W):
    from mygauhuman_amd import baking
    from mygauhuman_amd.pbr import view_dirs
    m = _cameras()[camera]
    cond = np.linalg.cond(m[:3, :3].astype(np.float64))
    assert cond <= 10.0, cond
    rays = baking.get_canonical_rays(H, W, 0.46, 0.4, device="cuda").float()
    if H * W > 1:
        rays[(H * W) // 2] = 0.0
    got = view_dirs(rays, _g(m), H, W)
    assert tuple(got.shape) == (H, W, 3) and got.dtype == torch.float32
    util.assert_close("view_dirs", _np(got), E.view_dirs(_np(rays), m, H, W))
    if H * W > 1:
        assert float(got.reshape(-1, 3)[(H * W) // 2].abs().max()) == 0.0   # F.normalize's rule: a zero ray gives zero
    zero = view_dirs(torch.zeros(1, 3, device="cuda"), _g(m), 1, 1)
    assert float(zero.abs().max()) == 0.0


def test_view_dirs_equal_evaluate_view_dirs_of_and_out_is_in_place():
    from mygauhuman_amd import baking, evaluate
    from mygauhuman_amd.pbr import view_dirs
    H, W = 17, 23
    m = _g(_cameras()["look_at"])
    rays = baking.get_canonical_rays(H, W, 0.46, 0.4, device="cuda").float()
    want = evaluate.view_dirs_of(types.SimpleNamespace(world_view_transform=m), rays, H, W)
    out = torch.full((H, W, 3), -7.0, device="cuda")
    got = view_dirs(rays, m, H, W, out=out)
    assert got is out
    util.assert_close("view_dirs against evaluate.view_dirs_of", _np(out), _np(want))
    with pytest.raises(ValueError, match="out"):
        view_dirs(rays, m, H, W, out=torch.empty(H * W, 3, device="cuda"))


# ---- all three inside one graph ------------------------------------------------------------------------------------------------
def test_light_inputs_are_captured_by_graphed_frame():
    """grey_envmap(out=), view_dirs(out=) and env_tv_loss(...).backward() recorded by graph.GraphedFrame: the capture passes its own
    verification, and a replay equals the eager calls at 2e-5 (the existing capture test's bound for atomics order), also after the
    light and the camera matrix are overwritten in place."""
    from mygauhuman_amd import baking
    from mygauhuman_amd.graph import GraphedFrame
    from mygauhuman_amd.pbr import env_tv_loss, view_dirs
    H, W = 33, 47
    cams = _cameras()
    light = _light(_base(32))
    wvt = _g(cams["look_at"])
    rays = baking.get_canonical_rays(H, W, 0.46, 0.4, device="cuda").float()
    dirs = _g(_tv_dirs((64, 128)))
    env = torch.zeros(1, 16, 32, device="cuda")
    vd = torch.zeros(H, W, 3, device="cuda")
    params = [light.base]

    def step():
        light.grey_envmap(out=env)
        view_dirs(rays, wvt, H, W, out=vd)
        loss = env_tv_loss(light.base, dirs)
        loss.backward()
        return loss.detach()

    def eager():
        light.base.grad = None
        loss = step()
        torch.cuda.synchronize()
        return loss.clone(), env.clone(), vd.clone(), light.base.grad.detach().clone()

    frame = GraphedFrame(step, warmup=3, zero_grads=params)
    for trial in range(2):
        if trial == 1:   # the next iteration's light and camera through the same graph
            with torch.no_grad():
                light.base.copy_(_g(_base(32, seed=1)))
            wvt.copy_(_g(cams["affine"]))
        loss_e, env_e, vd_e, grad_e = eager()
        env.zero_()
        vd.zero_()
        loss_g = frame.replay()
        torch.cuda.synchronize()
        frame.check()
        util.assert_close(f"captured loss {trial}", _np(loss_g).reshape(1), _np(loss_e).reshape(1), tol=2e-5)
        util.assert_close(f"captured grey map {trial}", _np(env), _np(env_e), tol=2e-5)
        util.assert_close(f"captured view_dirs {trial}", _np(vd), _np(vd_e), tol=2e-5)
        util.assert_close(f"captured d_base {trial}", _np(light.base.grad), _np(grad_e), tol=2e-5)
        if trial == 1:   # the replay saw the new inputs
            util.assert_close("view_dirs of the new camera", _np(vd), E.view_dirs(_np(rays), cams["affine"], H, W))
            util.assert_close("grey map of the new light", _np(env), E.grey_envmap(_base(32, seed=1), (16, 32)))
    assert float(light.base.grad.abs().sum()) > 0


# ---- guard bands -----------------------------------------------------------------------------------------------------------------
def test_writes_stay_inside_their_arrays(monkeypatch):
    """The bytes around out, the e workspace, the loss and d_base are untouched at shapes that fill no wave and no tile."""
    from mygauhuman_amd import baking
    from mygauhuman_amd.pbr import env
    from tests.test_gpu_guardband import GuardedTorch
    g = GuardedTorch()
    monkeypatch.setattr(env, "torch", g)
    for N in (8, 32):
        light = _light(_base(N))
        light.grey_envmap([9, 14])
        assert g.check("grey_envmap") == 1
        light.grey_envmap([9, 14], out=g.empty(1, 9, 14, device="cuda", dtype=torch.float32))
        assert g.check("grey_envmap(out=)") == 1
        b = _g(_base(N)).requires_grad_(True)
        v = env.env_tv_loss(b, _g(_tv_dirs((9, 14))))
        assert g.check("env_tv_loss forward") == 2    # the workspace (e and the partial sums), the loss
        v.backward()
        assert g.check("env_tv_loss backward") == 1   # d_base
        assert float(b.grad.abs().sum()) > 0
    m = _g(_cameras()["affine"])
    rays = baking.get_canonical_rays(17, 23, 0.46, 0.4, device="cuda").float()
    env.view_dirs(rays, m, 17, 23)
    assert g.check("view_dirs") == 1
    env.view_dirs(rays, m, 17, 23, out=g.empty(17, 23, 3, device="cuda", dtype=torch.float32))
    assert g.check("view_dirs(out=)") == 1
