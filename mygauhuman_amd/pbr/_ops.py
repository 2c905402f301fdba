"""Autograd functions over the image-based-lighting kernels of csrc/pbr.hip (include/gsr.h gsr_pbr_*).  Tensors must live on
the GPU and are used as contiguous float32: there is no CPU path."""
import ctypes as C

import numpy as np
import torch

from .._lib import PBR_MAX_LEVELS, PbrShade, PbrTexture, call, ptr


def _dev(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensors must live on a HIP device (no CPU path)")
    return t.detach().contiguous().float()


def make_texture(levels, cube, grads=None):
    """gsr_pbr_texture over level tensors ([6, n, n, C] cube faces or [H, W, C] images, contiguous float32)."""
    if not 1 <= len(levels) <= PBR_MAX_LEVELS:
        raise ValueError(f"1..{PBR_MAX_LEVELS} mip levels are supported, got {len(levels)}")
    t = PbrTexture()
    t.cube, t.channels, t.levels = int(cube), int(levels[0].shape[-1]), len(levels)
    for i, lv in enumerate(levels):
        t.height[i], t.width[i] = (lv.shape[1], lv.shape[2]) if cube else (lv.shape[0], lv.shape[1])
        t.data[i] = lv.data_ptr()
        t.grad[i] = ptr(grads[i]) if grads is not None and grads[i] is not None else None
    return t


class TextureFn(torch.autograd.Function):
    """out[n, C] = lookup of coords ([n, 3] directions on a cube, [n, 2] uv on a 2-D texture with the clamp boundary), trilinear
    over the levels by bias [n] when given.  Gradients: every level, the uv (2-D only) and the bias."""
    @staticmethod
    def forward(ctx, cube, coords, bias, *levels):
        lv = [_dev(t, "texture") for t in levels]
        c = _dev(coords, "texture")
        b = _dev(bias, "texture") if bias is not None else None
        n = c.shape[0]
        out = torch.empty(n, lv[0].shape[-1], device=c.device, dtype=torch.float32)
        tex = make_texture(lv, cube)
        call("gsr_pbr_texture_forward", c.device, C.byref(tex), n, ptr(c), ptr(b), ptr(out))
        ctx.cube = cube
        ctx.save_for_backward(c, b, *lv)
        return out

    @staticmethod
    def backward(ctx, g):
        c, b, *lv = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = [torch.zeros_like(t) if need[3 + i] else None for i, t in enumerate(lv)]
        dc = torch.empty_like(c) if (need[1] and not ctx.cube) else None
        db = torch.empty_like(b) if (b is not None and need[2]) else None
        g = g.contiguous().float()
        tex = make_texture(lv, ctx.cube, grads)
        call("gsr_pbr_texture_backward", c.device, C.byref(tex), c.shape[0], ptr(c), ptr(b), ptr(g), ptr(dc), ptr(db))
        return (None, dc, db, *grads)


class CubeMipFn(torch.autograd.Function):
    """CubemapLight's 2x2 mip (pbr/light.py cubemap_mip) with the reference's own backward."""
    @staticmethod
    def forward(ctx, cube):
        x = _dev(cube, "cubemap_mip")
        n, ch = x.shape[1], x.shape[-1]
        out = torch.empty(6, n // 2, n // 2, ch, device=x.device, dtype=torch.float32)
        call("gsr_pbr_cube_mip_forward", x.device, n, ch, ptr(x), ptr(out))
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        n, ch = g.shape[1] * 2, g.shape[-1]
        out = torch.empty(6, n, n, ch, device=g.device, dtype=torch.float32)
        call("gsr_pbr_cube_mip_backward", g.device, n, ch, ptr(g), ptr(out))
        return out


class DiffuseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube):
        x = _dev(cube, "diffuse_cubemap")
        out = torch.empty_like(x)
        call("gsr_pbr_diffuse_forward", x.device, x.shape[1], ptr(x), ptr(out))
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous().float()
        out = torch.empty_like(g)
        call("gsr_pbr_diffuse_backward", g.device, g.shape[1], ptr(g), ptr(out))
        return out


_CUTOFFS = {}


def ndf_cutoff(roughness, cutoff):
    """The GGX lobe's cosine bound that keeps `cutoff` of its energy: the host-side search of the reference's specular_cubemap
    (a million-sample cumulative sum), cached per (roughness, cutoff)."""
    key = (float(roughness), float(cutoff))
    if key not in _CUTOFFS:
        costheta = np.cos(np.linspace(0, np.pi / 2.0, 1000000))
        a2 = key[0] ** 4
        c = np.clip(costheta, 0.0, 1.0)
        d = (c * a2 - c) * c + 1.0
        D = np.cumsum(a2 / (d * d * np.pi))
        _CUTOFFS[key] = float(costheta[np.argmax(D >= D[..., -1] * key[1])])
    return _CUTOFFS[key]


class SpecularFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cube, roughness, cutoff):
        x = _dev(cube, "specular_cubemap")
        n = x.shape[1]
        out = torch.empty_like(x)
        wsum = torch.empty(6, n, n, device=x.device, dtype=torch.float32)
        cos_cut = ndf_cutoff(roughness, cutoff)
        call("gsr_pbr_specular_forward", x.device, n, roughness, cos_cut, ptr(x), ptr(out), ptr(wsum))
        ctx.save_for_backward(wsum)
        ctx.args = (roughness, cos_cut)
        return out

    @staticmethod
    def backward(ctx, g):
        wsum, = ctx.saved_tensors
        g = g.contiguous().float()
        out = torch.empty_like(g)
        call("gsr_pbr_specular_backward", g.device, g.shape[1], ctx.args[0], ctx.args[1], ptr(wsum), ptr(g), ptr(out))
        return out, None, None


class ShadeFn(torch.autograd.Function):
    """pbr_shading fused: returns render_rgb, diffuse_rgb, specular_rgb, diffuse_light ([n, 3] each)."""
    @staticmethod
    def forward(ctx, flags, normals, view_dirs, mask, background, lut, albedo, roughness, occlusion, metallic, diffuse, *specular):
        tone, gamma = flags
        t = {k: (_dev(v, "pbr_shading") if v is not None else None) for k, v in
             dict(normals=normals, view_dirs=view_dirs, mask=mask, background=background, lut=lut, albedo=albedo,
                  roughness=roughness, occlusion=occlusion, metallic=metallic, diffuse=diffuse).items()}
        spec = [_dev(s, "pbr_shading") for s in specular]
        n = t["normals"].shape[0]
        outs = [torch.empty(n, 3, device=t["normals"].device, dtype=torch.float32) for _ in range(4)]
        s = ShadeFn._struct(t, spec, tone, gamma)
        s.render_rgb, s.diffuse_rgb, s.specular_rgb, s.diffuse_light = (o.data_ptr() for o in outs)
        call("gsr_pbr_shade_forward", t["normals"].device, C.byref(s))
        ctx.flags = (tone, gamma)
        ctx.keys = list(t)
        ctx.save_for_backward(*[t[k] for k in t], *spec)
        return tuple(outs)

    @staticmethod
    def _struct(t, spec, tone, gamma):
        s = PbrShade()
        s.n, s.tone, s.gamma = t["normals"].shape[0], int(bool(tone)), int(bool(gamma))
        for k in ("normals", "view_dirs", "albedo", "roughness", "mask", "occlusion", "metallic", "background"):
            setattr(s, k, ptr(t[k]))
        s.diffuse = make_texture([t["diffuse"]], True)
        s.specular = make_texture(spec, True)
        s.lut = make_texture([t["lut"]], False)
        return s

    @staticmethod
    def backward(ctx, g_render, g_diffuse, g_specular, g_light):
        saved = ctx.saved_tensors
        nk = len(ctx.keys)
        t = dict(zip(ctx.keys, saved[:nk]))
        spec = list(saved[nk:])
        need = ctx.needs_input_grad  # (flags, normals, view_dirs, mask, background, lut, albedo, roughness, occlusion, metallic, ...)
        s = ShadeFn._struct(t, spec, *ctx.flags)
        gs = [g.contiguous().float() if g is not None else None for g in (g_render, g_diffuse, g_specular, g_light)]
        s.d_render_rgb, s.d_diffuse_rgb, s.d_specular_rgb, s.d_diffuse_light = (ptr(g) for g in gs)
        d_alb = torch.empty_like(t["albedo"]) if need[6] else None
        d_rough = torch.empty_like(t["roughness"]) if need[7] else None
        d_occ = torch.empty_like(t["occlusion"]) if need[8] else None
        d_met = torch.empty_like(t["metallic"]) if need[9] else None
        s.d_albedo, s.d_roughness, s.d_occlusion, s.d_metallic = ptr(d_alb), ptr(d_rough), ptr(d_occ), ptr(d_met)
        d_dif = torch.zeros_like(t["diffuse"]) if need[10] else None
        d_spec = [torch.zeros_like(x) if need[11 + i] else None for i, x in enumerate(spec)]
        s.diffuse.grad[0] = ptr(d_dif)
        for i, d in enumerate(d_spec):
            s.specular.grad[i] = ptr(d)
        call("gsr_pbr_shade_backward", t["normals"].device, C.byref(s))
        return (None, None, None, None, None, None, d_alb, d_rough, d_occ, d_met, d_dif, *d_spec)
