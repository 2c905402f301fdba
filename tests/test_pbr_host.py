"""CPU tests of the image-based-lighting stage: the float64 restatement (tests/pbr_reference.py) against the fixture the
reference's own pbr/shade.py and pbr/light.py produced (tests/golden/make_golden_pbr.py), the Python surface (state_dict keys,
install_dropin(pbr=True), get_brdf_lut) and the refused call shapes."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import pbr_reference as R
from tests import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LUT_PATH = os.path.join(GOLDEN, "pbr_brdf_256_256.bin")


@pytest.fixture(scope="module")
def fx():
    """The reference's outputs (stored, float32) with the inputs they were made from (rebuilt, not stored)."""
    return {**R.fixture_inputs(), **np.load(os.path.join(GOLDEN, "pbr_light.npz"))}


def _lut64():
    return torch.from_numpy(np.fromfile(LUT_PATH, dtype=np.float32).reshape(1, 256, 256, 2).astype(np.float64))


def test_cube_taps_seams_and_corners():
    N = 8
    rng = np.random.default_rng(0)
    d = np.concatenate([rng.normal(size=(2000, 3)), [[1, 1, 0], [1, 1, 1], [-1, 1, -1], [0, 0, 1], [1, 0.999999, 0.3]]])
    idx, w = R.cube_taps(d, N)
    np.testing.assert_allclose(w.sum(1), 1.0, rtol=0, atol=1e-12)
    assert (idx >= -1).all() and (idx < 6 * N * N).all()
    # every live tap's texel-centre direction lies close to the lookup direction (a wrapped tap lands next to the seam)
    td, _ = R.texel_dirs(N)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    for k in range(4):
        live = (idx[:, k] >= 0) & (w[:, k] > 0)
        cos = (td[idx[live, k]] * dn[live]).sum(1)
        assert cos.min() > np.cos(2.5 * np.pi / 2 / N), cos.min()
    # a corner direction: no corner tap survives, the three texels around the cube corner share the weight
    i, wc = R.cube_taps(np.array([[1.0, 1.0, 1.0]]), N)
    live = i[0][wc[0] > 0]
    assert len(set(live.tolist())) == 3
    np.testing.assert_allclose(np.sort(wc[0][wc[0] > 0]), [1 / 3] * 3, atol=1e-12)
    # the zero direction samples nothing
    i0, w0 = R.cube_taps(np.zeros((1, 3)), N)
    assert (i0 == -1).all() and (w0 == 0).all()


def test_restatement_prefilter_matches_fixture(fx):
    b = torch.from_numpy(fx["base16"]).requires_grad_(True)
    for k, t in (("mip", R.CubemapMip.apply(b)), ("diffuse", R.diffuse_cubemap(b)), ("specular", R.specular_cubemap(b, 0.5))):
        util.assert_close(k, t.detach().numpy(), fx[f"b16_{k}"], tol=1e-6)
        g, = torch.autograd.grad((t * torch.from_numpy(fx[f"w16_{k}"])).sum(), b)
        util.assert_close("d_" + k, g.numpy(), fx[f"b16_d_{k}"], tol=1e-6)
    env = R.texture(b[None], torch.from_numpy(R.envmap_dirs([16, 32]))[None], filter_mode="linear", boundary_mode="cube")[0]
    util.assert_close("envmap", env.detach().numpy(), fx["b16_envmap"], tol=1e-6)
    g, = torch.autograd.grad((env * torch.from_numpy(fx["w16_envmap"])).sum(), b)
    util.assert_close("d_envmap", g.numpy(), fx["b16_d_envmap"], tol=1e-6)


@pytest.mark.parametrize("case", ["plain", "metallic"])
def test_restatement_shading_matches_reference_composition(fx, case):
    """Our float64 composition of pbr_shading + build_mips against the reference's own code (on the same samplers); 1e-6: the
    fixture stores float32 values."""
    light = R.Light64(torch.from_numpy(fx["base32"]).requires_grad_(True))
    light.build_mips()
    px = {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("px_")}
    for k in ("albedo", "roughness", "occlusion", "metallic"):
        px[k].requires_grad_(True)
    res = R.pbr_shading(light, px["normals"], px["view_dirs"], px["albedo"], px["roughness"], px["mask"],
                        occlusion=px["occlusion"], metallic=px["metallic"] if case == "metallic" else None, brdf_lut=_lut64())
    loss = 0
    for k in ("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light"):
        util.assert_close(k, res[k].detach().numpy(), fx[f"{case}_{k}"], tol=1e-6)
        loss = loss + (res[k] * torch.from_numpy(fx["w_" + k])).sum()
    loss.backward()
    for k in ("albedo", "roughness", "occlusion") + (("metallic",) if case == "metallic" else ()):
        util.assert_close("d_" + k, px[k].grad.numpy(), fx[f"{case}_d_{k}"], tol=1e-6)
    util.assert_close("d_base", light.base.grad.numpy(), fx[f"{case}_d_base"], tol=1e-6)


def test_state_dict_keys_match_the_reference_class(tmp_path):
    from mygauhuman_amd.pbr import CubemapLight
    light = CubemapLight(base_res=8, device="cpu")
    # pbr/light.py registers the same Parameter twice: `base` and `env_base`
    assert list(light.state_dict().keys()) == ["base", "env_base"]
    assert light.base is light.env_base and light.base.shape == (6, 8, 8, 3)
    saved = torch.full((6, 8, 8, 3), 0.5)
    torch.save({"cubemap": {"base": saved, "env_base": saved}}, tmp_path / "env_map7000.pth")
    light.load_state_dict(torch.load(tmp_path / "env_map7000.pth")["cubemap"])
    assert float(light.base.detach().sum()) == 0.5 * saved.numel()
    with torch.no_grad():  # as the reference's callers do: an in-place op on the leaf
        light.clamp_(min=0.0, max=0.25)
    assert float(light.base.max()) == 0.25
    with pytest.raises(NotImplementedError, match="1-channel"):
        CubemapLight(base_res=8, train=True, device="cpu")


def test_install_dropin_registers_pbr_and_nvdiffrast(monkeypatch):
    import importlib

    import mygauhuman_amd
    for name in ("pbr", "pbr.light", "pbr.shade", "nvdiffrast", "nvdiffrast.torch"):
        monkeypatch.setitem(sys.modules, name, None)  # recorded, so that teardown restores the table as it was
        del sys.modules[name]
    mygauhuman_amd.install_dropin()
    assert "pbr" not in sys.modules and "nvdiffrast" not in sys.modules  # the default stays as it was
    mygauhuman_amd.install_dropin(pbr=True)
    from pbr import CubemapLight, get_brdf_lut, pbr_shading, saturate_dot  # noqa: F401
    import nvdiffrast.torch as dr
    assert CubemapLight is importlib.import_module("mygauhuman_amd.pbr").CubemapLight
    assert dr.texture is importlib.import_module("mygauhuman_amd.nvdiffrast.torch").texture
    a = torch.tensor([[0.6, 0.8, 0.0], [0.0, -1.0, 0.0]])
    assert saturate_dot(a, torch.tensor([[0.6, 0.8, 0.0], [0.0, 1.0, 0.0]])).flatten().tolist() == pytest.approx([1.0, 1e-4])


def test_get_brdf_lut_lookup_and_failure(tmp_path, monkeypatch):
    from mygauhuman_amd.pbr import get_brdf_lut
    lut = get_brdf_lut(LUT_PATH)
    assert lut.shape == (1, 256, 256, 2) and lut.dtype == torch.float32
    (tmp_path / "pbr").mkdir()
    (tmp_path / "pbr" / "brdf_256_256.bin").write_bytes(open(LUT_PATH, "rb").read())
    monkeypatch.setattr(sys, "path", [str(tmp_path / "nowhere"), str(tmp_path)])
    assert torch.equal(get_brdf_lut(), lut)
    monkeypatch.setattr(sys, "path", [str(tmp_path / "nowhere")])
    with pytest.raises(FileNotFoundError, match="nowhere"):
        get_brdf_lut()
    with pytest.raises(FileNotFoundError, match="missing.bin"):
        get_brdf_lut(str(tmp_path / "missing.bin"))


def test_unsupported_texture_calls_raise():
    from mygauhuman_amd.nvdiffrast.torch import texture
    cube = torch.zeros(1, 6, 8, 8, 3)
    dirs = torch.ones(1, 2, 2, 3)
    img = torch.zeros(1, 4, 4, 2)
    uv = torch.zeros(1, 2, 2, 2)
    bad = [
        lambda: texture(cube, dirs, filter_mode="nearest", boundary_mode="cube"),
        lambda: texture(cube, dirs, filter_mode="linear", boundary_mode="wrap"),
        lambda: texture(img, uv, filter_mode="linear", boundary_mode="zero"),
        lambda: texture(img, uv, filter_mode="linear-mipmap-linear", boundary_mode="clamp", mip=[img], mip_level_bias=uv[..., 0]),
        lambda: texture(cube, dirs, filter_mode="linear", boundary_mode="cube", mip=[cube]),
        lambda: texture(cube, dirs, uv_da=dirs, filter_mode="linear", boundary_mode="cube"),
        lambda: texture(cube, dirs, filter_mode="linear-mipmap-linear", boundary_mode="cube"),
        lambda: texture(cube, dirs.clone().requires_grad_(True), filter_mode="linear", boundary_mode="cube"),
        lambda: texture(img, dirs, filter_mode="linear", boundary_mode="clamp"),
        lambda: texture(cube, dirs, filter_mode="auto", boundary_mode="cube"),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(NotImplementedError):
            f()
            pytest.fail(f"call {i} did not raise")


def test_pbr_shading_refuses_normals_or_view_dirs_that_require_grad():
    from mygauhuman_amd.pbr import pbr_shading
    n = torch.zeros(2, 2, 3, requires_grad=True)
    v = torch.zeros(2, 2, 3)
    x = torch.zeros(2, 2, 1)
    with pytest.raises(ValueError, match="normals and view_dirs"):
        pbr_shading(None, n, v, v, x, x)
    with pytest.raises(ValueError, match="normals and view_dirs"):
        pbr_shading(None, v, n, v, x, x)
