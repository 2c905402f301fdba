"""The occlusion bake on the GPU (csrc/bake.hip behind mygauhuman_amd.baking): the grid against pc_to_grid bit for bit, the fused
visibility against the reference's algorithm run through the rasterizer (bake_set(fused=False)), the full bake against the
fixture made by the reference's own baking.py (tests/golden/make_golden_bake.py), guard bands, batching and determinism, the
per-frame reduction against its torch expression, and render() with install_dropin(bake=True)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import bake_reference as R
from tests import util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(means, scales, rots, opac, sh_degree=0):
    P = means.shape[0]
    return types.SimpleNamespace(get_xyz=means, get_scaling=scales, get_rotation=rots, get_opacity=opac,
                                 get_features=torch.zeros((P, 1, 3), device=means.device), active_sh_degree=sh_degree)


def _human(P, seed=0):
    from mygauhuman_amd import human_synth
    model, _ = human_synth.build(P, seed=seed)
    means = model.get_xyz.detach()
    g = torch.Generator().manual_seed(seed)
    n = torch.nn.functional.normalize(torch.randn((P, 3), generator=g), dim=1).cuda()
    return _model(means, model.get_scaling.detach(), model.get_rotation.detach(), model.get_opacity.detach()), means, n


def _edge_scene(P=3000, seed=3):
    """Points filling [-1, 1]^3 (cell size 0.2: neighbouring cells' Gaussians straddle the z = 0.2 cull plane), opacities that
    include exactly 1/255 and 0.99, scales from tiny to ones that cover all four tiles of a face, dense enough to terminate."""
    g = torch.Generator().manual_seed(seed)
    means = torch.rand((P, 3), generator=g) * 2 - 1
    scales = torch.exp(torch.randn((P, 3), generator=g) * 0.8 + np.log(0.04))
    scales[: P // 20] = 0.35
    rots = torch.nn.functional.normalize(torch.randn((P, 4), generator=g), dim=1)
    opac = torch.rand((P, 1), generator=g)
    opac[0::7] = 1.0 / 255.0
    opac[1::7] = 0.99
    opac[2::7] = 1.0
    n = torch.nn.functional.normalize(torch.randn((P, 3), generator=g), dim=1)
    d = lambda t: t.float().cuda().contiguous()  # noqa: E731
    return _model(d(means), d(scales), d(rots), d(opac)), d(means), d(n)


def _view():
    return types.SimpleNamespace(occlusion=None)


# ---- grid ------------------------------------------------------------------------------------------------------------------
def _grid_points(kind, P):
    g = torch.Generator().manual_seed(P)
    if kind == "random":
        return torch.randn((P, 3), generator=g) * torch.tensor([0.3, 0.8, 0.2]) + 0.1
    if kind == "flat_x":  # one zero-extent axis
        p = torch.randn((P, 3), generator=g)
        p[:, 0] = 0.25
        return p
    if kind == "one_cell":  # every axis zero-extent
        return torch.full((P, 3), -0.5)
    if kind == "all_cells":  # a point at every cell centre of a 10^3 lattice plus the two corners
        ax = (torch.arange(10, dtype=torch.float32) + 0.5) / 10
        pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        return torch.cat([pts, torch.zeros((1, 3)), torch.ones((1, 3))])
    raise ValueError(kind)


@pytest.mark.parametrize("kind,P", [("random", 1), ("random", 2), ("random", 63), ("random", 64), ("random", 65), ("random", 4000),
                                    ("random", 200000), ("flat_x", 500), ("one_cell", 10), ("all_cells", 0)])
def test_grid_matches_pc_to_grid(kind, P):
    from mygauhuman_amd import baking
    pts = _grid_points(kind, P).cuda().contiguous()
    cell, centres, size, idx = baking.grid_cells(pts)
    want_c, want_size, want_inv, want_idx = baking.pc_to_grid(pts, 10)
    assert centres.shape[0] == want_c.shape[0]
    if kind == "all_cells":
        assert centres.shape[0] == 1000
    if kind == "one_cell":
        assert centres.shape[0] == 1
    np.testing.assert_array_equal(cell.cpu().numpy(), want_inv.cpu().numpy())
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx.cpu().numpy())
    np.testing.assert_array_equal(centres.cpu().numpy().view(np.uint32), want_c.float().cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(size.cpu().numpy().view(np.uint32), want_size.cpu().numpy().view(np.uint32))


def test_grid_of_nothing():
    from mygauhuman_amd import baking
    cell, centres, _, _ = baking.grid_cells(torch.zeros((0, 3), device="cuda"))
    assert cell.shape == (0,) and centres.shape == (0, 3)
    out = baking.bake_set(_view(), _model(*(torch.zeros((0, k), device="cuda") for k in (3, 3, 4, 1))), torch.zeros((0, 3), device="cuda"),
                          torch.zeros((0, 3), device="cuda"), 16, 32)
    assert out.shape == (0, 16, 32, 1)


# ---- visibility against the reference's algorithm --------------------------------------------------------------------------
def _compare(model, means, n):
    from mygauhuman_amd import baking
    got = baking.bake_set(_view(), model, means, n, 16, 32).cpu().numpy()
    want = baking.bake_set(_view(), model, means, n, 16, 32, fused=False).cpu().numpy()
    assert np.isfinite(got).all()
    # bit-identical almost everywhere; the odd texel where an opacity of exactly 1/255 sits on the alpha threshold may round the
    # other way (then by about 1e-5): allowed for one element in 1e5, none past the outer bound
    print("bit-identical fraction", float((got.view(np.uint32) == want.view(np.uint32)).mean()))
    util.assert_close("occlusion", got, want, tol=1e-5, max_bad_frac=1e-5)
    return got, want


@pytest.mark.parametrize("P", [4000, 13000])
def test_fused_bake_matches_rasterizer_composition_human(P):
    got, want = _compare(*_human(P))
    assert (want > 0).any() and (want < 1).any()


def test_fused_bake_matches_rasterizer_composition_edge_cases():
    model, means, n = _edge_scene()
    got, want = _compare(model, means, n)
    from mygauhuman_amd import baking
    assert baking.LAST_STATS["cells"] > 900
    # early termination happened somewhere (a texel darker than the 1e-4 stop allows only with a stop) and light got through too
    assert (want > 0).any() and (np.abs(want) < 1e-3).any()


@pytest.mark.parametrize("name", R.SCENES)
def test_fused_bake_matches_reference_fixture(name):
    """Against the reference's own baking.py (tests/golden/make_golden_bake.py): inputs rebuilt, the occlusion rebuilt from the
    stored per-cell visibility and the reference's hemisphere mask."""
    from mygauhuman_amd import baking
    fx = np.load(os.path.join(GOLDEN, "bake_scenes.npz"))
    means, scales, rots, opac, n = R.scene(name)
    d = lambda a: torch.from_numpy(a).cuda().contiguous()  # noqa: E731
    model = _model(d(means), d(scales), d(rots), d(opac))
    cell, centres, size, idx = baking.grid_cells(d(means))
    np.testing.assert_array_equal(cell.cpu().numpy(), fx[f"{name}/pc_grid_indices"])
    # (the fixture ran on the CPU, where torch divides by the grid resolution instead of multiplying by 0.1f: an ulp)
    util.assert_close(f"{name} centres", centres.cpu().numpy(), fx[f"{name}/grid_centers"], tol=1e-6)
    views, projs, campos = baking.cube_cameras(centres[:R.CAMERA_CELLS])
    util.assert_close(f"{name} views", views.cpu().numpy(), fx[f"{name}/views"], tol=1e-6)
    util.assert_close(f"{name} projs", projs.cpu().numpy(), fx[f"{name}/projs"], tol=1e-6)
    _, dirs = baking.get_envmap_dirs()
    want = R.occlusion_of(fx[f"{name}/vis"], fx[f"{name}/pc_grid_indices"].astype(np.int64), R.hemisphere_mask(dirs, n))
    got = baking.bake_set(_view(), model, d(means), d(n), 16, 32).cpu().numpy()
    util.assert_close(f"{name} occlusion", got, want, tol=1e-4)


# ---- guard bands, batching, determinism ------------------------------------------------------------------------------------
def test_outputs_have_guard_bands():
    from mygauhuman_amd import _lib, baking
    model, means, n = _human(4000)
    cell, centres, _, _ = baking.grid_cells(means)
    Cn, P, G = centres.shape[0], means.shape[0], 4096
    _, dirs = baking.get_envmap_dirs()
    dirs = dirs.reshape(-1, 3).cuda().contiguous()
    want = baking.bake_visibility(means, model.get_scaling, model.get_rotation, model.get_opacity, cell, centres, dirs)
    sentinel = -1234.5
    vis = torch.full((Cn * 512 + 2 * G,), sentinel, device="cuda")
    views, projs, _ = baking.cube_cameras(centres)
    texel = baking.cube_nearest_texel(dirs).int().cuda()
    f = lambda t: t.detach().float().contiguous()  # noqa: E731
    m, s, r, o = f(means), f(model.get_scaling), f(model.get_rotation), f(model.get_opacity)
    scene = _lib.BakeScene(P, Cn, m.data_ptr(), s.data_ptr(), r.data_ptr(), o.data_ptr(), cell.data_ptr(), views.data_ptr(),
                           projs.data_ptr(), texel.data_ptr(), 512)
    plan = torch.empty((_lib.lib.gsr_bake_plan_bytes(P, Cn),), dtype=torch.uint8, device="cuda")
    inst = (C.c_ulonglong * 2)()
    _lib.check(_lib.lib.gsr_bake_plan(C.byref(scene), plan.data_ptr(), plan.numel(), inst, None), "plan")
    ws = torch.empty((_lib.lib.gsr_bake_visibility_workspace_bytes(Cn, int(inst[0])),), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.gsr_bake_visibility(C.byref(scene), plan.data_ptr(), vis[G:].data_ptr(), ws.data_ptr(), ws.numel(), None,
                                            None), "visibility")
    occ = torch.full((P * 512 + 2 * G,), sentinel, device="cuda")
    _lib.check(_lib.lib.gsr_bake_expand(P, 512, cell.data_ptr(), f(n).data_ptr(), dirs.data_ptr(), vis[G:].data_ptr(),
                                        occ[G:].data_ptr(), None), "expand")
    env = torch.rand((512,), device="cuda")
    red = torch.full((P * 3 + 2 * G,), sentinel, device="cuda")
    _lib.check(_lib.lib.gsr_bake_env_reduce(P, occ[G:].data_ptr(), env.data_ptr(), red[G:].data_ptr(), None), "env_reduce")
    torch.cuda.synchronize()
    for name, buf, k in (("vis", vis, Cn * 512), ("occ", occ, P * 512), ("env", red, P * 3)):
        assert (buf[:G] == sentinel).all() and (buf[G + k:] == sentinel).all(), name
    assert torch.equal(vis[G:G + Cn * 512].reshape(Cn, 512), want)


def test_batches_and_repeats_give_the_same_bits():
    from mygauhuman_amd import _lib, baking
    model, means, n = _human(4000, seed=1)
    a = baking.bake_set(_view(), model, means, n, 16, 32)
    assert baking.LAST_STATS["batches"] == 1
    b = baking.bake_set(_view(), model, means, n, 16, 32)
    assert torch.equal(a, b)
    c = baking.bake_set(_view(), model, means, n, 16, 32, workspace_bytes=1 << 20)
    assert baking.LAST_STATS["batches"] > 1
    assert torch.equal(a, c)
    _lib.set_tuning("bake_batch_cells", 3)
    try:
        d = baking.bake_set(_view(), model, means, n, 16, 32)
        assert baking.LAST_STATS["batches"] >= baking.LAST_STATS["cells"] // 3
    finally:
        _lib.set_tuning("bake_batch_cells", 0)
    assert torch.equal(a, d)


# ---- per-frame reduction ---------------------------------------------------------------------------------------------------
def test_env_reduction_matches_torch_at_200k():
    from mygauhuman_amd import baking
    g = torch.Generator(device="cuda").manual_seed(0)
    occ = torch.rand((200000, 16, 32, 1), device="cuda", generator=g) * 1.4 - 0.2
    envmap = torch.rand((1, 16, 32), device="cuda", generator=g) * 0.01
    got = baking.env_occlusion(occ, envmap)
    want = (torch.clamp(occ, min=0, max=1) * envmap.permute(1, 2, 0)).sum(dim=(1, 2)).repeat(1, 3).clamp(min=0.0, max=1.0)
    util.assert_close("env occlusion", got.cpu().numpy(), want.cpu().numpy(), tol=1e-5)
    big = baking.env_occlusion(occ, envmap * 100)  # the outer clamp
    assert float(big.max()) == 1.0


# ---- render() ----------------------------------------------------------------------------------------------------------------
def test_render_bakes_and_caches_with_bake_on():
    import mygauhuman_amd
    from mygauhuman_amd import baking
    from mygauhuman_amd import gaussian_renderer as gr
    from tests.test_gpu_render import _human_scene
    s = _human_scene(None)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    bg = torch.zeros(3, device="cuda")
    env = torch.rand((1, 16, 32), device="cuda") * 0.01
    s.cam.occlusion = None
    placeholder = gr.render(30001, s.cam, s.model, pipe, bg, envmap=env)["occlusion"]
    assert s.cam.occlusion is None
    try:
        mygauhuman_amd.install_dropin(bake=True)
        import sys
        assert sys.modules["baking"] is baking
        out = gr.render(30001, s.cam, s.model, pipe, bg, envmap=env)
        baked = s.cam.occlusion
        assert baked is not None and baked.shape[1:] == (16, 32, 1)
        cached = gr.render(30001, s.cam, s.model, pipe, bg, envmap=env)
        assert s.cam.occlusion is baked
        assert torch.equal(cached["occlusion"], out["occlusion"])
    finally:
        gr.BAKE = False
    # the same frame, its camera baked by the reference's algorithm (bake_set(fused=False) in render()'s place)
    s.cam.occlusion = None
    ref_cam = s.cam
    calls = {}
    real = baking.bake_set

    def oracle_bake(view, gaussians, means3D, normal, H, W, light_map=None):
        calls["n"] = calls.get("n", 0) + 1
        return real(view, gaussians, means3D, normal, H, W, fused=False)
    baking.bake_set = oracle_bake
    try:
        gr.BAKE = True
        ref_out = gr.render(30001, ref_cam, s.model, pipe, bg, envmap=env)
    finally:
        gr.BAKE = False
        baking.bake_set = real
    assert calls["n"] == 1
    util.assert_close("baked occlusion", baked.cpu().numpy(), ref_cam.occlusion.cpu().numpy(), tol=1e-5)
    # gradients of the occlusion image: same loss through both frames
    w = torch.rand_like(out["occlusion"])
    for o in (out, ref_out):
        assert o["occlusion"].requires_grad
    gw = [torch.autograd.grad((o["occlusion"] * w).sum(), s.model._xyz, retain_graph=True)[0] for o in (out, ref_out)]
    util.assert_close("occlusion image", out["occlusion"].detach().cpu().numpy(), ref_out["occlusion"].detach().cpu().numpy(), tol=1e-4)
    util.assert_close("d occlusion / d xyz", gw[0].cpu().numpy(), gw[1].cpu().numpy(), tol=1e-4)
    # bake off again: the placeholder frame is unchanged
    s.cam.occlusion = None
    again = gr.render(30001, s.cam, s.model, pipe, bg, envmap=env)["occlusion"]
    assert torch.equal(again, placeholder)
