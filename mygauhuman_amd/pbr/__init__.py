"""The reference's pbr package (CubemapLight, pbr_shading, get_brdf_lut, saturate_dot) on csrc/pbr.hip; install_dropin(pbr=True)
registers it as `pbr`."""
from .light import CubemapLight
from .shade import get_brdf_lut, pbr_shading, saturate_dot

__all__ = ["CubemapLight", "get_brdf_lut", "pbr_shading", "saturate_dot"]
