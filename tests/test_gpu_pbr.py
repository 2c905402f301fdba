"""The image-based-lighting stage on the GPU (csrc/pbr.hip behind mygauhuman_amd.pbr and mygauhuman_amd.nvdiffrast.torch): every
kernel forward and backward against the float64 restatement (tests/pbr_reference.py) and the fixture made by the reference's
own pbr code (tests/golden/make_golden_pbr.py), then render() -> pbr_shading -> the PBR loss end to end."""
import os
import types

import numpy as np
import pytest
import torch

from tests import pbr_reference as R
from tests import util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LUT_PATH = os.path.join(GOLDEN, "pbr_brdf_256_256.bin")
SIZES = [(1, 1), (17, 23), (512, 512), (1024, 1024)]


@pytest.fixture(scope="module")
def fx():
    """The reference's outputs (stored, float32) with the inputs they were made from (rebuilt, not stored)."""
    return {**R.fixture_inputs(), **np.load(os.path.join(GOLDEN, "pbr_light.npz"))}


def _g(x):
    return torch.from_numpy(np.asarray(x, np.float32)).cuda()


def _r(x):
    """The float64 restatement's copy of what the kernel sees (float32 values)."""
    return torch.from_numpy(np.asarray(x, np.float32).astype(np.float64))


def _r_roughness(x):
    """Roughness for the restatement: float32 copies of 0.08 / 0.5 / 1.0 stay ON get_mip's clamp bounds, as they are for the
    kernel (and for the reference's float32 torch.clamp, whose Python-scalar bounds are float32 there too)."""
    x64 = _r(x)
    for b in (0.08, 0.5, 1.0):
        x64 = torch.where(x64 == float(np.float32(b)), torch.full_like(x64, b), x64)
    return x64


def _np(t):
    return t.detach().cpu().numpy()


def _dirs(n, rng):
    """Random directions with face edges, cube corners, texel-aligned and zero directions planted."""
    d = rng.normal(size=(n, 3))
    special = np.array([[1, 1, 0], [1, -1, 0], [0, 1, 1], [0, -1, -1], [1, 0, -1], [-1, 0, 1], [1, 1, 1], [-1, 1, -1],
                        [1, -1, -1], [-1, -1, 1], [0, 0, 1], [0, 0, -1], [1, 0.5, 0.25], [0, 0, 0]], np.float64)
    k = min(len(special), n)
    d[:k] = special[:k]
    return d.astype(np.float32)


def _lut():
    from mygauhuman_amd.pbr import get_brdf_lut
    return get_brdf_lut(LUT_PATH)


# ---- generic texture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_cube_texture_forward_backward(H, W):
    from mygauhuman_amd.nvdiffrast.torch import texture
    rng = np.random.default_rng(H * 7 + W)
    tex = rng.uniform(0, 1, (6, 32, 32, 3)).astype(np.float32)
    d = _dirs(H * W, rng).reshape(1, H, W, 3)
    g = rng.normal(size=(1, H, W, 3)).astype(np.float32)
    t = _g(tex).requires_grad_(True)
    out = texture(t[None], _g(d), filter_mode="linear", boundary_mode="cube")
    out.backward(_g(g))
    t64 = _r(tex).requires_grad_(True)
    o64 = R.texture(t64[None], _r(d), filter_mode="linear", boundary_mode="cube")
    (o64 * _r(g)).sum().backward()
    util.assert_close("out", _np(out), _np(o64))
    util.assert_close("d_tex", _np(t.grad), _np(t64.grad))


@pytest.mark.parametrize("H,W", [(17, 23), (512, 512)])
def test_lut_texture_clamp_forward_backward(H, W):
    from mygauhuman_amd.nvdiffrast.torch import texture
    rng = np.random.default_rng(1)
    lut = _lut().numpy()
    uv = rng.uniform(-0.2, 1.2, (1, H, W, 2)).astype(np.float32)
    g = rng.normal(size=(1, H, W, 2)).astype(np.float32)
    t, u = _g(lut).requires_grad_(True), _g(uv).requires_grad_(True)
    out = texture(t, u, filter_mode="linear", boundary_mode="clamp")
    out.backward(_g(g))
    t64, u64 = _r(lut).requires_grad_(True), _r(uv).requires_grad_(True)
    o64 = R.texture(t64, u64, filter_mode="linear", boundary_mode="clamp")
    (o64 * _r(g)).sum().backward()
    util.assert_close("out", _np(out), _np(o64))
    util.assert_close("d_lut", _np(t.grad), _np(t64.grad))
    util.assert_close("d_uv", _np(u.grad), _np(u64.grad))


@pytest.mark.parametrize("H,W", [(17, 23), (1024, 1024)])
def test_mip_texture_trilinear_forward_backward(H, W):
    from mygauhuman_amd.nvdiffrast.torch import texture
    rng = np.random.default_rng(2)
    levels = [rng.uniform(0, 1, (6, n, n, 3)).astype(np.float32) for n in (32, 16, 8)]
    d = _dirs(H * W, rng).reshape(1, H, W, 3)
    bias = rng.uniform(-0.5, 2.5, (1, H, W)).astype(np.float32)
    bias.reshape(-1)[:5] = [0.0, 1.0, 2.0, -0.25, 2.25]
    g = rng.normal(size=(1, H, W, 3)).astype(np.float32)
    ts = [_g(x).requires_grad_(True) for x in levels]
    b = _g(bias).requires_grad_(True)
    out = texture(ts[0][None], _g(d), mip=[x[None] for x in ts[1:]], mip_level_bias=b, filter_mode="linear-mipmap-linear",
                  boundary_mode="cube")
    out.backward(_g(g))
    t64 = [_r(x).requires_grad_(True) for x in levels]
    b64 = _r(bias).requires_grad_(True)
    o64 = R.texture(t64[0][None], _r(d), mip=[x[None] for x in t64[1:]], mip_level_bias=b64, filter_mode="linear-mipmap-linear",
                    boundary_mode="cube")
    (o64 * _r(g)).sum().backward()
    util.assert_close("out", _np(out), _np(o64))
    for i in range(3):
        util.assert_close(f"d_level{i}", _np(ts[i].grad), _np(t64[i].grad))
    util.assert_close("d_bias", _np(b.grad), _np(b64.grad))


# ---- prefilter -------------------------------------------------------------------------------------------------------------
def test_prefilter_kernels_match_reference_fixture(fx):
    from mygauhuman_amd.pbr.light import cubemap_mip, diffuse_cubemap, specular_cubemap
    b = _g(fx["base16"]).requires_grad_(True)
    for k, fn in (("mip", cubemap_mip), ("diffuse", diffuse_cubemap), ("specular", lambda x: specular_cubemap(x, 0.5))):
        out = fn(b)
        util.assert_close(k, _np(out), fx[f"b16_{k}"])
        g, = torch.autograd.grad((out * _g(fx[f"w16_{k}"])).sum(), b)
        util.assert_close("d_" + k, _np(g), fx[f"b16_d_{k}"])


@pytest.mark.parametrize("n,roughness", [(32, 0.08), (16, 0.5), (8, 1.0), (32, 0.29)])
def test_prefilter_kernels_match_restatement(n, roughness):
    """The non-adjoint mip backward, the diffuse sum and the specular lobe at each roughness of the schedule."""
    from mygauhuman_amd.pbr.light import cubemap_mip, diffuse_cubemap, specular_cubemap
    rng = np.random.default_rng(n)
    base = rng.uniform(0.1, 1.0, (6, n, n, 3)).astype(np.float32)
    b, b64 = _g(base).requires_grad_(True), _r(base).requires_grad_(True)
    for k, fn, fn64 in (("mip", cubemap_mip, R.CubemapMip.apply), ("diffuse", diffuse_cubemap, R.diffuse_cubemap),
                        ("specular", lambda x: specular_cubemap(x, roughness), lambda x: R.specular_cubemap(x, roughness))):
        out, o64 = fn(b), fn64(b64)
        w = rng.normal(size=tuple(o64.shape)).astype(np.float32)
        util.assert_close(k, _np(out), _np(o64))
        g, = torch.autograd.grad((out * _g(w)).sum(), b)
        g64, = torch.autograd.grad((o64 * _r(w)).sum(), b64)
        util.assert_close("d_" + k, _np(g), _np(g64))


def test_envmap_export_matches_reference_fixture(fx):
    from mygauhuman_amd.pbr import CubemapLight
    light = CubemapLight(base_res=16)
    with torch.no_grad():
        light.base.copy_(_g(fx["base16"]))
    env = light.export_envmap(return_img=True, res=[16, 32])
    util.assert_close("envmap", _np(env), fx["b16_envmap"])
    (env * _g(fx["w16_envmap"])).sum().backward()
    util.assert_close("d_envmap", _np(light.base.grad), fx["b16_d_envmap"])


# ---- shading ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "tone", "gamma", "metallic"])
def test_shading_and_build_mips_match_reference_fixture(fx, case):
    """build_mips + pbr_shading + a weighted sum of every result, backward to the pixels and the light's base."""
    from mygauhuman_amd.pbr import CubemapLight, pbr_shading
    tone, gamma, met = case == "tone", case == "gamma", case == "metallic"
    light = CubemapLight(base_res=32)
    with torch.no_grad():
        light.base.copy_(_g(fx["base32"]))
    light.build_mips()
    px = {k[3:]: _g(v) for k, v in fx.items() if k.startswith("px_")}
    for k in ("albedo", "roughness", "occlusion", "metallic"):
        px[k].requires_grad_(True)
    res = pbr_shading(light, px["normals"], px["view_dirs"], px["albedo"], px["roughness"], px["mask"], tone=tone, gamma=gamma,
                      occlusion=px["occlusion"], metallic=px["metallic"] if met else None, brdf_lut=_lut().cuda())
    H, W = px["normals"].shape[:2]
    loss = 0
    for k in ("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light"):
        assert res[k].shape == (H, W, 3)
        util.assert_close(k, _np(res[k]), fx[f"{case}_{k}"])
        loss = loss + (res[k] * _g(fx["w_" + k])).sum()
    loss.backward()
    for k in ("albedo", "roughness", "occlusion") + (("metallic",) if met else ()):
        util.assert_close("d_" + k, _np(px[k].grad), fx[f"{case}_d_{k}"])
    if f"{case}_d_base" in fx:  # stored for plain and metallic
        util.assert_close("d_base", _np(light.base.grad), fx[f"{case}_d_base"])


def _pixels(H, W, rng, zero_mask=False):
    n = _dirs(H * W, rng).astype(np.float64)
    n[np.linalg.norm(n, axis=1) == 0] = [0, 1, 0]
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    v = n + 0.7 * rng.normal(size=n.shape)
    v[1::7] = -n[1::7]  # back-facing: NoV at its clamp
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rough = rng.uniform(0, 1, (H * W, 1))
    rough[:3, 0] = [0.08, 0.5, 1.0][:H * W]
    rough[3::11, 0] = 0.08
    rough[4::13, 0] = 0.5
    rough[5::17, 0] = 1.0
    mask = (rng.uniform(size=(H * W, 1)) > 0.2).astype(np.float64) * (0 if zero_mask else 1)
    p = dict(normals=n, view_dirs=v, albedo=rng.uniform(0.05, 0.95, (H * W, 3)), roughness=rough,
             occlusion=rng.uniform(0.3, 1, (H * W, 1)), metallic=rng.uniform(0, 1, (H * W, 1)), mask=mask)
    return {k: x.reshape(H, W, -1).astype(np.float32) for k, x in p.items()}


def _shade_both(px, light, tone=False, gamma=False, met=False, seed=0):
    """The fused pass and the float64 composition on the same light levels; returns both results and gradients."""
    from mygauhuman_amd.pbr import pbr_shading
    H, W = px["normals"].shape[:2]
    rng = np.random.default_rng(seed)
    wts = {k: rng.normal(size=(H, W, 3)).astype(np.float32) for k in ("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light")}
    lut = _lut()
    out = {}
    for side in ("gpu", "ref"):
        cv = _g if side == "gpu" else _r
        t = {k: cv(v) for k, v in px.items()}
        if side == "ref":
            t["roughness"] = _r_roughness(px["roughness"])
        for k in ("albedo", "roughness", "occlusion", "metallic"):
            t[k].requires_grad_(True)
        lt = types.SimpleNamespace(diffuse=cv(_np(light.diffuse)).requires_grad_(True),
                                   specular=[cv(_np(s)).requires_grad_(True) for s in light.specular])
        lt.get_mip = light.get_mip if side == "gpu" else R.Light64.get_mip.__get__(lt)
        fn = pbr_shading if side == "gpu" else R.pbr_shading
        res = fn(lt, t["normals"], t["view_dirs"], t["albedo"], t["roughness"], t["mask"], tone=tone, gamma=gamma,
                 occlusion=t["occlusion"], metallic=t["metallic"] if met else None,
                 brdf_lut=lut.cuda() if side == "gpu" else lut.double())
        loss = sum((res[k].reshape(H, W, 3) * cv(w)).sum() for k, w in wts.items())
        loss.backward()
        o = {k: _np(res[k]).reshape(H, W, 3) for k in wts}
        o.update({"d_" + k: _np(t[k].grad) for k in ("albedo", "roughness", "occlusion") + (("metallic",) if met else ())})
        o["d_diffuse"] = _np(lt.diffuse.grad)
        o.update({f"d_specular{i}": _np(s.grad) for i, s in enumerate(lt.specular)})
        out[side] = o
    return out["gpu"], out["ref"]


@pytest.fixture(scope="module")
def light32():
    from mygauhuman_amd.pbr import CubemapLight
    torch.manual_seed(0)
    light = CubemapLight(base_res=32)
    with torch.no_grad():
        light.build_mips()
    return light


@pytest.mark.parametrize("H,W", SIZES)
def test_shading_matches_restatement(light32, H, W):
    got, want = _shade_both(_pixels(H, W, np.random.default_rng(H + W)), light32, seed=H)
    for k in want:
        util.assert_close(k, got[k], want[k])


@pytest.mark.parametrize("variant", ["zero_mask", "tone", "gamma", "metallic", "tone_gamma_metallic"])
def test_shading_variants_match_restatement(light32, variant):
    px = _pixels(17, 23, np.random.default_rng(5), zero_mask=variant == "zero_mask")
    got, want = _shade_both(px, light32, tone="tone" in variant, gamma="gamma" in variant, met="metallic" in variant)
    if variant == "zero_mask":
        assert (got["render_rgb"] == 0).all()
    for k in want:
        util.assert_close(k, got[k], want[k])


def test_shading_refuses_normals_that_require_grad(light32):
    from mygauhuman_amd.pbr import pbr_shading
    px = {k: _g(v) for k, v in _pixels(4, 4, np.random.default_rng(0)).items()}
    with pytest.raises(ValueError, match="normals and view_dirs"):
        pbr_shading(light32, px["normals"].requires_grad_(True), px["view_dirs"], px["albedo"], px["roughness"], px["mask"],
                    brdf_lut=_lut().cuda())
    with pytest.raises(ValueError, match="normals and view_dirs"):
        pbr_shading(light32, px["normals"].detach(), px["view_dirs"].requires_grad_(True), px["albedo"], px["roughness"],
                    px["mask"], brdf_lut=_lut().cuda())


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_render_pbr_loss_reaches_gaussians_and_light():
    """render() -> pbr_shading -> the PBR-phase image loss of train.py:299-318 (l1 + ssim + BRDF TV; lpips is out of scope) plus
    the env-map TV term through dr.texture: the gradient reaches the Gaussians' parameters and the light."""
    import mygauhuman_amd
    from mygauhuman_amd.gaussian_renderer import render
    from mygauhuman_amd.loss_utils import l1_loss, ssim
    from tests.test_gpu_render import _human_scene
    mygauhuman_amd.install_dropin(pbr=True)
    import nvdiffrast.torch as dr
    from pbr import CubemapLight, get_brdf_lut, pbr_shading
    s = _human_scene(None)
    pipe = types.SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=True)
    torch.manual_seed(0)
    cubemap = CubemapLight(base_res=32).cuda()
    env = cubemap.export_envmap(return_img=True, res=[16, 32]).permute(2, 0, 1).clamp(0.0, 1.0)
    out = render(1, s.cam, s.model, pipe, _g([0, 0, 0]), envmap=env.mean(0, keepdim=True).detach())
    H, W = out["render"].shape[1:]
    cubemap.build_mips()
    alpha = out["render_alpha"]
    roughness = out["roughness"][0:1] * (1.0 - 0.04) + 0.04
    view_dirs = torch.nn.functional.normalize(_g(np.random.default_rng(0).normal(size=(H, W, 3))), dim=-1)
    res = pbr_shading(light=cubemap, normals=out["world_normal"].permute(1, 2, 0).detach(), view_dirs=view_dirs,
                      mask=alpha.permute(1, 2, 0), albedo=out["albedo"].permute(1, 2, 0), roughness=roughness.permute(1, 2, 0),
                      metallic=None, tone=False, gamma=False, occlusion=out["occlusion"][0:1].permute(1, 2, 0),
                      brdf_lut=get_brdf_lut(LUT_PATH).cuda())
    render_rgb = res["render_rgb"].permute(2, 0, 1)
    gt = torch.rand(3, H, W, device="cuda")
    bound = alpha[0] > 0
    loss = l1_loss(render_rgb.permute(1, 2, 0)[bound], gt.permute(1, 2, 0)[bound]) + 0.01 * (1.0 - ssim(render_rgb[None], gt[None]))
    pred = torch.cat([out["albedo"], roughness], 0)
    tv_h = (pred[:, 1:, :] - pred[:, :-1, :]) ** 2 * (alpha[:, 1:, :] * alpha[:, :-1, :])
    tv_w = (pred[:, :, 1:] - pred[:, :, :-1]) ** 2 * (alpha[:, :, 1:] * alpha[:, :, :-1])
    loss = loss + tv_h.mean() + tv_w.mean()
    envmap = dr.texture(cubemap.base[None], _g(R.envmap_dirs([256, 512]))[None].contiguous(), filter_mode="linear",
                        boundary_mode="cube")[0]
    loss = loss + 0.01 * (((envmap[1:] - envmap[:-1]) ** 2).mean() + ((envmap[:, 1:] - envmap[:, :-1]) ** 2).mean())
    loss.backward()
    assert torch.isfinite(loss)
    g = cubemap.base.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0
    for name, p in zip(("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "normal", "albedo"), s.model.parameters()):
        if name in ("xyz", "opacity", "albedo"):
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name


def test_adam_on_light_and_materials_tracks_the_restatement():
    """Twenty Adam steps on cubemap.base + albedo + roughness (build_mips and pbr_shading every step, a smooth image loss) on the
    kernels and on the float64 restatement from the same start."""
    from mygauhuman_amd.pbr import CubemapLight, pbr_shading
    rng = np.random.default_rng(11)
    H, W = 24, 32
    px = _pixels(H, W, rng)
    px["roughness"] = rng.uniform(0.12, 0.95, (H, W, 1)).astype(np.float32)  # a trajectory away from get_mip's clamp bounds
    gt = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    base0 = rng.uniform(0.2, 0.8, (6, 32, 32, 3)).astype(np.float32)
    lut = _lut()
    final = {}
    for side in ("gpu", "ref"):
        cv = _g if side == "gpu" else _r
        if side == "gpu":
            light = CubemapLight(base_res=32)
            with torch.no_grad():
                light.base.copy_(cv(base0))
            base = light.base
        else:
            base = cv(base0).requires_grad_(True)
            light = R.Light64(base)
        alb, rough = cv(px["albedo"]).requires_grad_(True), cv(px["roughness"]).requires_grad_(True)
        opt = torch.optim.Adam([base, alb, rough], lr=1e-3)
        for _ in range(20):
            opt.zero_grad()
            light.build_mips()
            fn = pbr_shading if side == "gpu" else R.pbr_shading
            res = fn(light, cv(px["normals"]), cv(px["view_dirs"]), alb, rough, cv(px["mask"]), occlusion=cv(px["occlusion"]),
                     brdf_lut=lut.cuda() if side == "gpu" else lut.double())
            loss = ((res["render_rgb"] - cv(gt)) ** 2).mean() + 0.1 * (res["specular_rgb"] ** 2).mean()
            loss.backward()
            opt.step()
        final[side] = {"base": _np(base), "albedo": _np(alb), "roughness": _np(rough)}
    for k in final["ref"]:
        util.assert_close(k, final["gpu"][k], final["ref"][k], max_bad_frac=1e-3)
