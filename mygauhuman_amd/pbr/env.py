"""The environment light's own share of a PBR step on csrc/pbr.hip, without host reads, so that a whole PBR
iteration records into graph.GraphedFrame with the light's inputs computed inside the graph:

    CubemapLight.grey_envmap(res, out)                    train.py:195-198, render.py:164-167 (light.py; the kernel call is here)
    env_tv_loss(base, dirs)                               train.py:352-363: the TV of the cube lookup over a latitude-longitude grid
    view_dirs(canonical_rays, world_view_transform, H, W) train.py:217, 238-242, render.py:215-222

Tensors must live on the GPU (no CPU path); they are read as contiguous float32."""
import torch

from .._lib import ENV_TV_AUTO, call, lib, ptr

# torchvision.transforms.functional.rgb_to_grayscale's weights (the kernel holds the same constants)
GREY_WEIGHTS = (0.2989, 0.587, 0.114)


def _cube_n(base, what, exc=ValueError):
    if not isinstance(base, torch.Tensor) or base.dim() != 4 or base.shape[0] != 6 or base.shape[1] != base.shape[2] or \
            base.shape[3] != 3 or base.shape[1] < 1:
        shape = tuple(base.shape) if isinstance(base, torch.Tensor) else type(base).__name__
        raise exc(f"{what}: base must be a 3-channel cube map [6, N, N, 3], got {shape}")
    return base.shape[1]


def _on_dev(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensors must live on a HIP device (no CPU path)")


def _same_dev(a, b, what):
    _on_dev(a, what)
    _on_dev(b, what)
    if a.device != b.device:
        raise RuntimeError(f"{what}: tensors live on different devices ({a.device}, {b.device})")


def grey_envmap(base, dirs, out=None):
    """[1, h, w] grey values of clamp(lookup(base, dirs [h, w, 3]), 0, 1); one launch, no gradient."""
    n_face = _cube_n(base, "grey_envmap", NotImplementedError)
    _same_dev(base, dirs, "grey_envmap")
    h, w = dirs.shape[:2]
    if out is None:
        out = torch.empty(1, h, w, device=base.device, dtype=torch.float32)
    elif tuple(out.shape) != (1, h, w) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != base.device:
        raise ValueError(f"grey_envmap: out must be a contiguous float32 [1, {h}, {w}] tensor on {base.device}")
    b = base.detach().contiguous().float()
    call("gsr_pbr_env_grey", base.device, n_face, ptr(b), h * w, ptr(dirs), ptr(out))
    return out


class _EnvTvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, base, dirs, reduce):
        b, d = base.detach().contiguous().float(), dirs.detach().contiguous().float()
        h, w = d.shape[-3], d.shape[-2]
        ws = torch.empty(int(lib.gsr_pbr_env_tv_workspace_floats(h, w)), device=b.device, dtype=torch.float32)
        loss = torch.empty((), device=b.device, dtype=torch.float32)
        call("gsr_pbr_env_tv_forward", b.device, b.shape[1], ptr(b), h, w, ptr(d), ptr(ws), ptr(loss))
        ctx.save_for_backward(d, ws)
        ctx.args = (b.shape[1], h, w, reduce)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        d, ws = ctx.saved_tensors
        n_face, h, w, reduce = ctx.args
        d_base = torch.zeros(6, n_face, n_face, 3, device=d.device, dtype=torch.float32)
        up = g.detach().contiguous().float()
        call("gsr_pbr_env_tv_backward", d.device, n_face, h, w, ptr(d), ptr(ws), ptr(up), ptr(d_base), reduce)
        return d_base, None, None


def env_tv_loss(base, dirs, reduce=ENV_TV_AUTO):
    """train.py:352-363 fused: ((e[1:] - e[:-1])**2).mean() + ((e[:, 1:] - e[:, :-1])**2).mean() of e = the linear cube lookup of
    base [6, N, N, 3] (or a CubemapLight: its base) at dirs [h, w, 3] or [1, h, w, 3]; a 0-dim tensor whose gradient reaches base
    only.  Two launches forward (partial sums, then their sum in a fixed order: repeats give the same bits), one backward after
    the gradient's zero fill (float atomics: not bit-identical between repeats).  A zero direction samples 0.
    reduce: how the backward splits its samples (_lib.ENV_TV_*; measurement only)."""
    if isinstance(base, torch.nn.Module) and hasattr(base, "base"):
        base = base.base
    _cube_n(base, "env_tv_loss")
    if not isinstance(dirs, torch.Tensor) or dirs.shape[-1:] != (3,) or not (dirs.dim() == 3 or (dirs.dim() == 4 and dirs.shape[0] == 1)):
        raise ValueError(f"env_tv_loss: dirs must be [h, w, 3] or [1, h, w, 3], got "
                         f"{tuple(dirs.shape) if isinstance(dirs, torch.Tensor) else type(dirs).__name__}")
    h, w = dirs.shape[-3], dirs.shape[-2]
    if h < 2 or w < 2:
        raise ValueError(f"env_tv_loss: the grid must be at least 2 x 2 (a mean over no differences is NaN), got {h} x {w}")
    if h * w > 1 << 28:
        raise ValueError("env_tv_loss: at most 2^28 directions")
    if dirs.requires_grad:
        raise NotImplementedError("env_tv_loss: no gradient with respect to cube-map directions")
    _same_dev(base, dirs, "env_tv_loss")
    return _EnvTvFn.apply(base, dirs, int(reduce))


def view_dirs(canonical_rays, world_view_transform, H, W, out=None):
    """render.py:215-222 in one launch: -(c2w[:3, :3] @ normalize(ray)) per pixel, [H, W, 3], with c2w = inverse(world_view_transform.T)
    formed in the kernel (a 4 x 4 cofactor inverse), so that a new camera matrix written in place is seen by a captured graph.
    canonical_rays [H * W, 3]; world_view_transform [4, 4] float32 on the rays' device (cameras.ViewCamera's row-vector convention).
    F.normalize's rule: a zero ray gives zero.  No gradient.  A singular matrix gives non-finite directions (torch.inverse raises
    there, which takes a host read); out= is written in place and returned."""
    H, W = int(H), int(W)
    if not isinstance(canonical_rays, torch.Tensor) or canonical_rays.dim() != 2 or canonical_rays.shape[1] != 3 or \
            canonical_rays.shape[0] != H * W or H < 1 or W < 1:
        raise ValueError(f"view_dirs: canonical_rays must be [H * W, 3] = [{H * W}, 3], got "
                         f"{tuple(canonical_rays.shape) if isinstance(canonical_rays, torch.Tensor) else type(canonical_rays).__name__}")
    m = world_view_transform
    if not isinstance(m, torch.Tensor) or tuple(m.shape) != (4, 4) or m.dtype != torch.float32:
        raise ValueError("view_dirs: world_view_transform must be a float32 [4, 4] tensor")
    _same_dev(canonical_rays, m, "view_dirs")
    if out is None:
        out = torch.empty(H, W, 3, device=m.device, dtype=torch.float32)
    elif tuple(out.shape) != (H, W, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != m.device:
        raise ValueError(f"view_dirs: out must be a contiguous float32 [{H}, {W}, 3] tensor on {m.device}")
    rays, m = canonical_rays.detach().contiguous().float(), m.detach().contiguous()
    call("gsr_pbr_view_dirs", m.device, H * W, ptr(rays), ptr(m), ptr(out))
    return out
