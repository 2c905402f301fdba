"""A stand-in for nvdiffrast that provides nvdiffrast.torch.texture for the reference's call shapes only (csrc/pbr.hip)."""
from . import torch  # noqa: F401
