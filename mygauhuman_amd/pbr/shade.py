"""pbr_shading on one fused kernel forward and one backward (csrc/pbr.hip), behind the reference's pbr/shade.py signature and
result keys; get_brdf_lut and saturate_dot as there.

The fused pass, per pixel: the diffuse light (light.diffuse ** (1/2.2), clamped, looked up at the normal) times the occlusion and
the albedo; NoV = saturate_dot(normal, view); the BRDF LUT at (NoV, roughness); the specular cube, trilinear at the reflected
direction and the level get_mip(roughness); F0 = 0.04 or from metallic; diffuse + specular, clamped (or ACES when tone), then
linear_to_srgb when gamma, then the mask select.  Gradients reach albedo, roughness (through the LUT and the mip level),
occlusion, metallic, light.diffuse and every light.specular level.  Normals and view directions take none: the reference detaches
the normals and the view directions are constants, so a tensor of either that requires grad is refused."""
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

from . import _ops
from .light import CubemapLight

LUT_NAME = os.path.join("pbr", "brdf_256_256.bin")


def saturate_dot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a * b).sum(dim=-1, keepdim=True).clamp(min=1e-4, max=1.0)


def get_brdf_lut(path: Optional[str] = None) -> torch.Tensor:
    """The split-sum BRDF LUT [1, 256, 256, 2] (rows: roughness, columns: NoV), float32 on the CPU.  It is reference data and is
    not shipped: read from `path`, else from pbr/brdf_256_256.bin under an entry of sys.path (the reference checkout the drivers
    run from)."""
    tried = [path] if path is not None else [os.path.join(p or os.getcwd(), LUT_NAME) for p in sys.path]
    for p in tried:
        if os.path.isfile(p):
            return torch.from_numpy(np.fromfile(p, dtype=np.float32).reshape(1, 256, 256, 2))
    raise FileNotFoundError("get_brdf_lut: brdf_256_256.bin not found; looked at " + ", ".join(tried) +
                            " (pass path=, or run from a checkout that has pbr/brdf_256_256.bin)")


def pbr_shading(
    light: CubemapLight,
    normals: torch.Tensor,  # [H, W, 3]
    view_dirs: torch.Tensor,  # [H, W, 3]
    albedo: torch.Tensor,  # [H, W, 3]
    roughness: torch.Tensor,  # [H, W, 1]
    mask: torch.Tensor,  # [H, W, 1]
    tone: bool = False,
    gamma: bool = False,
    occlusion: Optional[torch.Tensor] = None,  # [H, W, 1]
    metallic: Optional[torch.Tensor] = None,
    brdf_lut: Optional[torch.Tensor] = None,
    background: Optional[torch.Tensor] = None,
) -> Dict:
    if normals.requires_grad or view_dirs.requires_grad:
        raise ValueError("pbr_shading: normals and view_dirs take no gradient on the fused pass (the reference detaches the "
                         "normals); pass normals.detach() / view_dirs.detach()")
    if brdf_lut is None:
        raise ValueError("pbr_shading: brdf_lut is required (get_brdf_lut())")
    H, W, _ = normals.shape
    n = H * W
    dev = normals.device
    lut = brdf_lut.to(dev)
    lut = lut.reshape(lut.shape[-3:])
    bg_in_kernel = background is None or not background.requires_grad
    outs = _ops.ShadeFn.apply(
        (bool(tone), bool(gamma)), normals.reshape(n, 3), view_dirs.reshape(n, 3), mask.reshape(n),
        background.expand(H, W, 3).reshape(n, 3) if (background is not None and bg_in_kernel) else None, lut,
        albedo.reshape(n, 3), roughness.reshape(n),
        occlusion.reshape(n) if occlusion is not None else None,
        metallic.reshape(n) if metallic is not None else None,
        light.diffuse, *light.specular)
    render_rgb, diffuse_rgb, specular_rgb, diffuse_light = (o.reshape(H, W, 3) for o in outs)
    if not bg_in_kernel:
        render_rgb = torch.where(mask.reshape(H, W, 1) > 0, render_rgb, background)
    return {
        "diffuse_light": diffuse_light,
        "render_rgb": render_rgb,
        "diffuse_rgb": diffuse_rgb[None].squeeze(),
        "specular_rgb": specular_rgb[None].squeeze(),
    }
