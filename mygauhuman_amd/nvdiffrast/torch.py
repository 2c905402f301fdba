"""nvdiffrast.torch.texture for exactly the three call shapes of the reference (pbr/light.py, pbr/shade.py, train.py:352-358):

    texture(cube[1, 6, N, N, C], dirs[1, h, w, 3], filter_mode="linear", boundary_mode="cube")
    texture(image[1, H, W, C], uv[1, h, w, 2], filter_mode="linear", boundary_mode="clamp")
    texture(cube[1, 6, N, N, C], dirs[1, h, w, 3], mip=[levels], mip_level_bias=bias[1, h, w],
            filter_mode="linear-mipmap-linear", boundary_mode="cube")

on csrc/pbr.hip, forward and backward (gradients: the texture and its mip levels, the 2-D uv, mip_level_bias).  Any other mode or
argument raises NotImplementedError."""
from ..pbr import _ops


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode="auto", boundary_mode="wrap", max_mip_level=None):
    if uv_da is not None or max_mip_level is not None:
        raise NotImplementedError("texture: uv_da / max_mip_level are not supported")
    if boundary_mode == "cube":
        if tex.dim() != 5 or tex.shape[0] != 1 or tex.shape[1] != 6 or tex.shape[2] != tex.shape[3] or uv.shape[-1] != 3:
            raise NotImplementedError("texture: cube lookups take tex [1, 6, N, N, C] and directions [1, h, w, 3]")
        if uv.requires_grad:
            raise NotImplementedError("texture: no gradient with respect to cube-map directions")
    elif boundary_mode == "clamp":
        if tex.dim() != 4 or tex.shape[0] != 1 or uv.shape[-1] != 2:
            raise NotImplementedError("texture: 2-D lookups take tex [1, H, W, C] and uv [1, h, w, 2]")
    else:
        raise NotImplementedError(f"texture: boundary_mode={boundary_mode!r} (only 'cube' and 'clamp')")
    if uv.dim() != 4 or uv.shape[0] != 1 or not 1 <= tex.shape[-1] <= 4:
        raise NotImplementedError("texture: one minibatch entry, uv [1, h, w, *], 1..4 channels")
    if filter_mode == "linear":
        if mip is not None or mip_level_bias is not None:
            raise NotImplementedError("texture: filter_mode='linear' takes no mip / mip_level_bias")
        levels = [tex[0]]
        bias = None
    elif filter_mode == "linear-mipmap-linear":
        if boundary_mode != "cube" or mip is None or mip_level_bias is None or not isinstance(mip, (list, tuple)):
            raise NotImplementedError("texture: 'linear-mipmap-linear' takes a cube map, an explicit mip list and mip_level_bias")
        if any(m.dim() != 5 or m.shape[0] != 1 or m.shape[1] != 6 for m in mip):
            raise NotImplementedError("texture: mip levels are [1, 6, n, n, C]")
        levels = [tex[0]] + [m[0] for m in mip]
        bias = mip_level_bias.reshape(-1)
    else:
        raise NotImplementedError(f"texture: filter_mode={filter_mode!r} (only 'linear' and 'linear-mipmap-linear')")
    lead = uv.shape[:-1]
    out = _ops.TextureFn.apply(boundary_mode == "cube", uv.reshape(-1, uv.shape[-1]), bias, *levels)
    return out.reshape(*lead, tex.shape[-1])


__all__ = ["texture"]
