"""The reference's pbr package (CubemapLight, pbr_shading, get_brdf_lut, saturate_dot) on csrc/pbr.hip; install_dropin(pbr=True)
registers it as `pbr`.  The PBR phase's training loss (PbrPhaseLoss and its parts) runs on csrc/pbr_loss.hip; its SSIM term on the bound-mask crop (loss_utils.bounding_rect, ssim_crop) is re-exported next to it.  The light's own share of a step -- CubemapLight.grey_envmap, env_tv_loss, view_dirs (env.py) -- makes no host read either."""
from ..loss_utils import bounding_rect, ssim_crop
from .env import env_tv_loss, view_dirs
from .light import CubemapLight
from .loss import MaterialSmoothness, PbrPhaseLoss, gaussian_entropy, get_masked_tv_loss
from .shade import get_brdf_lut, pbr_shading, saturate_dot

__all__ = ["CubemapLight", "MaterialSmoothness", "PbrPhaseLoss", "bounding_rect", "env_tv_loss", "gaussian_entropy", "get_brdf_lut",
           "get_masked_tv_loss", "pbr_shading", "saturate_dot", "ssim_crop", "view_dirs"]
