"""CubemapLight on the fused kernels: the reference's pbr/light.py class (same constructor (plus `device`, default "cuda" as there), parameter `base` also registered as
`env_base`, so state_dict keys match and env_map<iter>.pth loads), with the mip chain, the diffuse and the GGX specular
prefilter on csrc/pbr.hip, forward and backward.  Three channels only: the 1-channel light (train=True) is not built."""
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _ops


def diffuse_cubemap(cubemap: torch.Tensor) -> torch.Tensor:
    return _ops.DiffuseFn.apply(cubemap)


def specular_cubemap(cubemap: torch.Tensor, roughness: float, cutoff: float = 0.99) -> torch.Tensor:
    if cubemap.shape[0] != 6 or cubemap.shape[1] != cubemap.shape[2]:
        raise ValueError(f"bad shape for a cube map: {tuple(cubemap.shape)}")
    return _ops.SpecularFn.apply(cubemap, float(roughness), float(cutoff))


def cubemap_mip(cubemap: torch.Tensor) -> torch.Tensor:
    return _ops.CubeMipFn.apply(cubemap)


class CubemapLight(nn.Module):
    LIGHT_MIN_RES = 8

    MIN_ROUGHNESS = 0.08
    MAX_ROUGHNESS = 0.5

    def __init__(self, base_res: int = 512, scale: float = 0.5, bias: float = 0.25, train: bool = False,
                 device="cuda") -> None:
        super().__init__()
        if train:
            raise NotImplementedError("CubemapLight(train=True): the 1-channel light is not built; 3-channel lights only")
        self.mtx = None
        self.is_train = train
        base = torch.rand(6, base_res, base_res, 3, dtype=torch.float32, device=device) * scale + bias
        self.base = nn.Parameter(base)
        self.register_parameter("env_base", self.base)
        self._grey_dirs = {}  # (h, w, device) -> grey_envmap's direction grid

    def _check(self):
        if self.base.dim() != 4 or self.base.shape[-1] != 3:
            raise NotImplementedError(f"CubemapLight: 3-channel lights only, base has shape {tuple(self.base.shape)}")

    def xfm(self, mtx) -> None:
        self.mtx = mtx

    def clamp_(self, min: Optional[float] = None, max: Optional[float] = None) -> None:
        self.base.clamp_(min, max)

    def get_mip(self, roughness: torch.Tensor) -> torch.Tensor:
        return torch.where(
            roughness < self.MAX_ROUGHNESS,
            (torch.clamp(roughness, self.MIN_ROUGHNESS, self.MAX_ROUGHNESS) - self.MIN_ROUGHNESS)
            / (self.MAX_ROUGHNESS - self.MIN_ROUGHNESS) * (len(self.specular) - 2),
            (torch.clamp(roughness, self.MAX_ROUGHNESS, 1.0) - self.MAX_ROUGHNESS) / (1.0 - self.MAX_ROUGHNESS)
            + len(self.specular) - 2,
        )

    def build_mips(self, cutoff: float = 0.99) -> None:
        self._check()
        self.specular = [self.base]
        while self.specular[-1].shape[1] > self.LIGHT_MIN_RES:
            self.specular += [cubemap_mip(self.specular[-1])]
        self.diffuse = diffuse_cubemap(self.specular[0])
        # the reference's roughness schedule, its division by len - 2 included (a base of 16 raises ZeroDivisionError there too)
        for idx in range(len(self.specular) - 1):
            roughness = (idx / (len(self.specular) - 2)) * (self.MAX_ROUGHNESS - self.MIN_ROUGHNESS) + self.MIN_ROUGHNESS
            self.specular[idx] = specular_cubemap(self.specular[idx], roughness, cutoff)
        self.specular[-1] = specular_cubemap(self.specular[-1], 1.0, cutoff)

    def grey_envmap(self, res: List[int] = [16, 32], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """train.py:195-198 / render.py:164-167 in one launch: Grayscale()(export_envmap(return_img=True, res).permute(2, 0, 1)
        .clamp(0, 1)), [1, h, w], without a gradient.  The direction grid (export_envmap's own expressions) is built once per
        (res, device) at the first call: call once before recording a graph, so that the grid is not allocated in the graph's pool
        (graph.GraphedFrame's warm-up does).  Grids of other devices are dropped, so a light moved with .to() keeps one.  out= is
        written in place and returned, so a captured graph refreshes the map render(envmap=...) reads."""
        from . import env
        if self.base.dim() != 4 or self.base.shape[0] != 6 or self.base.shape[1] != self.base.shape[2] or self.base.shape[3] != 3:
            raise NotImplementedError(f"CubemapLight: 3-channel cube lights [6, N, N, 3] only, base has shape {tuple(self.base.shape)}")
        if len(res) != 2 or int(res[0]) < 1 or int(res[1]) < 1:
            raise ValueError(f"grey_envmap: res must be two positive sizes, got {list(res)}")
        dev = self.base.device
        if not self.base.is_cuda:
            raise RuntimeError("grey_envmap: the light must live on a HIP device (no CPU path)")
        key = (int(res[0]), int(res[1]), dev)
        cache = self.__dict__.setdefault("_grey_dirs", {})
        if key not in cache:
            for old in [k for k in cache if k[2] != dev]:
                del cache[old]
            gy, gx = torch.meshgrid(torch.linspace(0.0, 1.0, key[0], device=dev), torch.linspace(-1.0, 1.0, key[1], device=dev),
                                    indexing="ij")
            sintheta, costheta = torch.sin(gy * np.pi), torch.cos(gy * np.pi)
            sinphi, cosphi = torch.sin(gx * np.pi), torch.cos(gx * np.pi)
            cache[key] = torch.stack((sintheta * sinphi, costheta, -sintheta * cosphi), dim=-1).contiguous()
        with torch.no_grad():
            return env.grey_envmap(self.base, cache[key], out)

    def export_envmap(self, filename: Optional[str] = None, res: List[int] = [256, 512],
                      return_img: bool = False) -> Optional[torch.Tensor]:
        from ..nvdiffrast.torch import texture
        dev = self.base.device
        gy, gx = torch.meshgrid(torch.linspace(0.0, 1.0, res[0], device=dev), torch.linspace(-1.0, 1.0, res[1], device=dev),
                                indexing="ij")
        sintheta, costheta = torch.sin(gy * np.pi), torch.cos(gy * np.pi)
        sinphi, cosphi = torch.sin(gx * np.pi), torch.cos(gx * np.pi)
        reflvec = torch.stack((sintheta * sinphi, costheta, -sintheta * cosphi), dim=-1)
        color = texture(self.base[None, ...], reflvec[None, ...].contiguous(), filter_mode="linear", boundary_mode="cube")[0]
        if return_img:
            return color
        import cv2  # only to write the image, as in the reference
        cv2.imwrite(filename, color.clamp(min=0.0).detach().cpu().numpy()[..., ::-1])
