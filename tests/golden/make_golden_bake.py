"""Generate tests/golden/bake_scenes.npz (CPU) from the reference's OWN baking.py, so that pc_to_grid, the cube cameras, the
per-cell composition and the hemisphere mask are pinned by the reference's code, not by ours.

    python tests/golden/make_golden_bake.py /path/to/reference

baking.py imports modules that do not exist here; they are stood in for in sys.modules before it is imported:
  * diff_gaussian_rasterization._C.rasterize_gaussians -> the CPU oracle (oracle.rasterize_forward, pinned to the reference);
  * nvdiffrast.torch.texture (filter_mode="nearest", boundary_mode="cube") -> the float64 restatement (tests/bake_reference.py);
  * everything else it imports at module top (scene, gs_ir, arguments, gaussian_renderer, utils.*, imageio, tqdm, torchvision)
    -> empty modules, except utils.graphics_utils.getProjectionMatrix, which is the reference's own.
The module's `torch` name is pointed at a shim whose zeros / linspace / tensor drop device="cuda", and Tensor.cuda() is the
identity while it runs.  The inputs are not stored: tests/bake_reference.py scene() rebuilds them bit for bit.  The occlusion
is stored as the per-cell visibility it is made of (occlusion = dot_map * vis[cell]; tests/bake_reference.py occlusion_of), the
cube matrices for the first few cells."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402
from tests import bake_reference as R  # noqa: E402


class _TorchShim(types.ModuleType):
    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **kw):
        kw.pop("device", None)
        return torch.zeros(*a, **kw)

    def linspace(self, *a, **kw):
        kw.pop("device", None)
        return torch.linspace(*a, **kw)

    def tensor(self, *a, **kw):
        kw.pop("device", None)
        return torch.tensor(*a, **kw)

    def zeros_like(self, *a, **kw):
        kw.pop("device", None)
        return torch.zeros_like(*a, **kw)


CALLS = []


def rasterize_gaussians(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                        tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, debug):
    CALLS.append((viewmatrix.clone(), projmatrix.clone()))
    n = lambda t: t.detach().cpu().numpy().astype(np.float32)  # noqa: E731
    P = means3D.shape[0]
    f = oracle.rasterize_forward(n(means3D), n(opacity).reshape(-1), n(viewmatrix), n(projmatrix), n(campos), W, H, tanfovx, tanfovy,
                                 n(bg), scales=n(scales), rotations=n(rotations), scale_modifier=scale_modifier,
                                 shs=n(sh)[:P], degree=degree)
    img = f["img"]
    alpha = torch.from_numpy(np.asarray(img["alpha"], np.float32).reshape(1, H, W))
    return 0, torch.zeros((3, H, W)), torch.zeros((1, H, W)), alpha, torch.zeros(P, dtype=torch.int32)


def import_reference(ref_root):
    spec = importlib.util.spec_from_file_location("ref_graphics_utils", os.path.join(ref_root, "utils", "graphics_utils.py"))
    gu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gu)
    dgr_c = _mod("diff_gaussian_rasterization._C", rasterize_gaussians=rasterize_gaussians)
    dr = _mod("nvdiffrast.torch", texture=lambda tex, uv, filter_mode=None, boundary_mode=None: R.texture_nearest(tex, uv))
    mods = {"nvdiffrast": _mod("nvdiffrast", torch=dr), "nvdiffrast.torch": dr,
            "diff_gaussian_rasterization": _mod("diff_gaussian_rasterization", _C=dgr_c), "diff_gaussian_rasterization._C": dgr_c,
            "gs_ir": _mod("gs_ir", _C=None), "scene": _mod("scene", Scene=None), "tqdm": _mod("tqdm", trange=range, tqdm=iter),
            "arguments": _mod("arguments", ModelParams=None, PipelineParams=None, get_combined_args=None),
            "gaussian_renderer": _mod("gaussian_renderer", GaussianModel=None), "utils": _mod("utils"),
            "utils.graphics_utils": gu, "utils.sh_utils": _mod("utils.sh_utils", components_from_spherical_harmonics=None),
            "utils.general_utils": _mod("utils.general_utils", safe_state=None), "imageio": _mod("imageio"),
            "imageio.v2": _mod("imageio.v2"), "torchvision": _mod("torchvision"),
            "torchvision.transforms": _mod("torchvision.transforms", Grayscale=None)}
    sys.modules.update(mods)
    spec = importlib.util.spec_from_file_location("ref_baking", os.path.join(ref_root, "baking.py"))
    baking = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(baking)
    baking.torch = _TorchShim("torch")
    return baking


def _mod(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def main(ref_root):
    baking = import_reference(ref_root)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **kw: self
    out = {}
    try:
        for name in R.SCENES:
            means, scales, rots, opac, n = R.scene(name)
            t = {k: torch.from_numpy(v) for k, v in dict(means3D=means, scales=scales, rotations=rots, opacity=opac, normal=n).items()}
            g = types.SimpleNamespace(get_xyz=t["means3D"], get_opacity=t["opacity"], get_features=torch.zeros((len(means), 1, 3)),
                                      get_scaling=t["scales"], get_rotation=t["rotations"], active_sh_degree=0)
            centres, sizes, inv, uniq = baking.pc_to_grid(t["means3D"], 10)
            view = types.SimpleNamespace()
            view.set_occlusion = lambda o, v=view: setattr(v, "occlusion", o)
            CALLS.clear()
            occ = baking.bake_set(view, g, t["means3D"], t["normal"], 16, 32)
            assert view.occlusion is occ
            C = centres.shape[0]
            assert len(CALLS) == 6 * C
            # stored compactly: occlusion = dot_map * vis[cell], with dot_map recomputed from the rebuilt normals by the
            # reference's own expression; visibility_of checks that this reproduces the reference's output bit for bit
            _, dirs = baking.get_envmap_dirs()
            mask = R.hemisphere_mask(dirs, t["normal"])
            k = R.CAMERA_CELLS
            out[f"{name}/grid_centers"] = centres.numpy().astype(np.float32)
            out[f"{name}/pc_grid_indices"] = inv.numpy().astype(np.int16)
            out[f"{name}/views"] = torch.stack([c[0] for c in CALLS[:6 * k]]).reshape(-1, 6, 4, 4).numpy()
            out[f"{name}/projs"] = torch.stack([c[1] for c in CALLS[:6 * k]]).reshape(-1, 6, 4, 4).numpy()
            out[f"{name}/vis"] = R.visibility_of(occ.numpy().astype(np.float32), inv.numpy(), mask, C)
            print(name, "P", len(means), "cells", C, "occlusion mean", float(occ.mean()))
    finally:
        torch.Tensor.cuda = cuda
    np.savez_compressed(os.path.join(HERE, "bake_scenes.npz"), **out)
    print("wrote", os.path.join(HERE, "bake_scenes.npz"), len(out), "arrays")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT", "."))
