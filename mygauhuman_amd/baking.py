"""baking.py of the reference (bake_set and its helpers) on the HIP bake of csrc/bake.hip.

bake_set() bins the posed Gaussians into a 10^3 grid, renders for every occupied cell the six 90-degree cube faces (32 x 32, the
cell's own Gaussians left out) with the rasterizer's semantics, reads each face at the nearest texel of 16 x 32 equirect
directions and masks the result by each Gaussian's normal hemisphere: occlusion [P, 16, 32, 1] = 1 - alpha in the direction.

fused=False runs the reference's algorithm as written, 6 rasterizer calls per cell through diff_gaussian_rasterization._C; it is
the test oracle and the benchmark baseline.  Both use the same cube cameras (cube_cameras) and the same nearest-texel rule
(cube_nearest_texel: the face and texel addressing of nvdiffrast.torch.texture here, the texel that contains the point).
The envmap directions are computed on the CPU and moved, so that every device sees the same bits.
"""
import ctypes as C
import math
from typing import List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import call, lib

RES = 10             # grid cells per axis (pc_to_grid(points, 10))
FACE = 32            # cube face size
ENV_H, ENV_W = 16, 32
WORKSPACE_BYTES = 512 << 20  # visibility workspace budget: cells are baked in batches whose instances fit (20 B each)
LAST_STATS = {}      # of the last fused bake: instances, largest batch, batches, capacity, workspace bytes, cells

# the reference's six cube-face camera-to-world rotations (baking.py:147-196), face order +x -x +y -y +z -z
CUBE_ROTATIONS = (
    ((0.0, 0.0, 1.0, 0.0), (0.0, -1.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
    ((0.0, 0.0, -1.0, 0.0), (0.0, -1.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
    ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
    ((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (0.0, -1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
    ((1.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
    ((-1.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (0.0, 0.0, 0.0, 1.0)),
)


def get_envmap_dirs(res: List[int] = [16, 32], device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(solid_angles [H, W, 1], directions [H, W, 3]) as the reference computes them, on `device` (default CPU)."""
    gy, gx = torch.meshgrid(torch.linspace(0.0, 1.0, res[0], device=device), torch.linspace(-1.0, 1.0, res[1], device=device),
                            indexing="ij")
    d_theta, d_phi = np.pi / res[0], 2 * np.pi / res[1]
    sintheta, costheta = torch.sin(gy * np.pi), torch.cos(gy * np.pi)
    sinphi, cosphi = torch.sin(gx * np.pi), torch.cos(gx * np.pi)
    reflvec = torch.stack((sintheta * sinphi, costheta, -sintheta * cosphi), dim=-1)
    solid_angles = ((costheta - torch.cos(gy * np.pi + d_theta)) * d_phi)[..., None]
    return solid_angles, reflvec


def get_canonical_rays(H: int, W: int, tan_fovx: float, tan_fovy: float, device=None) -> torch.Tensor:
    """Unnormalised camera-space ray directions [H * W, 3] (the reference's, on `device`)."""
    cen_x, cen_y = W / 2, H / 2
    focal_x, focal_y = W / (2.0 * tan_fovx), H / (2.0 * tan_fovy)
    x, y = torch.meshgrid(torch.arange(W, device=device), torch.arange(H, device=device), indexing="xy")
    x, y = x.flatten(), y.flatten()
    return F.pad(torch.stack([(x - cen_x + 0.5) / focal_x, (y - cen_y + 0.5) / focal_y], dim=-1), (0, 1), value=1.0)


def pc_to_grid(pc, res):
    """The reference's pc_to_grid on any device, with the arithmetic it gets on the GPU: `(max - min) / res` divides by a host
    scalar, which torch's GPU kernels evaluate as a multiplication by the float32 reciprocal; that is written out here so that
    the CPU gives the same bits.  A zero-extent axis (0 / 0 there) puts every point at index 0."""
    min_coords = torch.min(pc, dim=0)[0]
    max_coords = torch.max(pc, dim=0)[0]
    inv = torch.tensor(1.0 / res, dtype=pc.dtype, device=pc.device)
    grid_sizes = torch.stack([(max_coords[k] - min_coords[k]) * inv for k in range(3)])
    q = torch.floor((pc - min_coords) / grid_sizes)
    pc_indices = torch.where(torch.isnan(q), torch.zeros_like(q), q).long().clamp(min=0, max=res - 1)
    unique_indices, unique_inverse = torch.unique(pc_indices, return_inverse=True, dim=0)
    grid_centers = min_coords[None, :] + (unique_indices * grid_sizes[None, :]) + grid_sizes[None, :] / 2
    return grid_centers, grid_sizes, unique_inverse, unique_indices


def projection_matrix(device=None):
    """getProjectionMatrix(znear=0.01, zfar=5, fovX=fovY=pi/2).transpose(0, 1) (utils/graphics_utils.py:51-70)."""
    znear, zfar = 0.01, 5.0
    tan_half = math.tan(math.pi * 0.5 / 2)
    top, right = tan_half * znear, tan_half * znear
    P = torch.zeros(4, 4)
    P[0, 0] = 2.0 * znear / (right - (-right))
    P[1, 1] = 2.0 * znear / (top - (-top))
    P[0, 2] = (right + -right) / (right - (-right))
    P[1, 2] = (top + -top) / (top - (-top))
    P[3, 2] = 1.0
    P[2, 2] = 1.0 * zfar / (zfar - znear)
    P[2, 3] = -2 * (zfar * znear) / (zfar - znear)
    return P.transpose(0, 1).to(device)


def cube_cameras(centres):
    """(world_view_transform, full_proj_transform, camera_center) [C, 6, 4, 4], [C, 6, 4, 4], [C, 6, 3] of the cube faces at
    `centres` [C, 3]: the reference's expression sequence (baking.py:247-257), batched over cells and faces."""
    dev = centres.device
    c2w = torch.tensor(CUBE_ROTATIONS, device=dev)[None].repeat(centres.shape[0], 1, 1, 1)
    c2w[:, :, :3, 3] = centres[:, None, :]
    w2c = torch.inverse(c2w)
    Rt = torch.zeros_like(w2c)
    Rt[..., :3, :3] = w2c[..., :3, :3]  # getWorld2ViewTorch(R, T) with R = w2c[:3, :3].T stores R.T
    Rt[..., :3, 3] = w2c[..., :3, 3]
    Rt[..., 3, 3] = 1.0
    view = Rt.transpose(-1, -2).contiguous()
    full = torch.matmul(view, projection_matrix(dev)).contiguous()
    campos = torch.inverse(view)[..., 3, :3].contiguous()
    return view, full, campos


def cube_nearest_texel(dirs, N=FACE):
    """Texel index face * N * N + y * N + x of the texel containing each direction [..., 3] (float64 arithmetic): the face and
    face-local coordinates of nvdiffrast.torch.texture's cube addressing, u = clamp((a / m + 1) / 2, 0, 1),
    x = min(floor(u N), N - 1).  A zero or non-finite direction gets -1."""
    d = dirs.detach().to(torch.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    f = torch.where(az > torch.maximum(ax, ay), torch.where(z < 0, 5, 4),
                    torch.where(ay > ax, torch.where(y < 0, 3, 2), torch.where(x < 0, 1, 0)))
    m = torch.stack([x, -x, y, -y, z, -z], 1).gather(1, f[:, None])[:, 0]
    a = torch.stack([-z, z, x, x, x, -x], 1).gather(1, f[:, None])[:, 0]
    b = torch.stack([-y, -y, z, -z, -y, -y], 1).gather(1, f[:, None])[:, 0]
    valid = (m > 0) & torch.isfinite(a) & torch.isfinite(b) & torch.isfinite(m)
    ms = torch.where(valid, m, torch.ones_like(m))
    u = ((a / ms + 1.0) * 0.5).clamp(0.0, 1.0)
    v = ((b / ms + 1.0) * 0.5).clamp(0.0, 1.0)
    tx = torch.clamp(torch.floor(u * N), max=N - 1).long()
    ty = torch.clamp(torch.floor(v * N), max=N - 1).long()
    idx = (f * N + ty) * N + tx
    return torch.where(valid, idx, torch.full_like(idx, -1)).reshape(dirs.shape[:-1])


def cube_nearest(cube, dirs):
    """Nearest lookup of `cube` [6, N, N, C] at `dirs` [..., 3] -> [..., C] (cube_nearest_texel; 0 where there is no texel)."""
    N, Cn = cube.shape[1], cube.shape[3]
    idx = cube_nearest_texel(dirs, N).reshape(-1).to(cube.device)
    flat = cube.reshape(-1, Cn)
    out = flat[idx.clamp(min=0)] * (idx >= 0)[:, None].to(cube.dtype)
    return out.reshape(tuple(dirs.shape[:-1]) + (Cn,))


def grid_cells(points):
    """pc_to_grid on the HIP kernels: (cell id [P] int32, centres [C, 3], grid sizes [3], cell indices [C, 3] int32).  The
    occupied cells are numbered in torch.unique's order, so cell ids equal pc_to_grid's unique_inverse.  Reads C to the host."""
    dev = points.device
    pts = points.detach().float().contiguous()
    P = pts.shape[0]
    cell = torch.empty((P,), dtype=torch.int32, device=dev)
    centres = torch.empty((RES ** 3, 3), dtype=torch.float32, device=dev)
    size = torch.empty((3,), dtype=torch.float32, device=dev)
    idx = torch.empty((RES ** 3, 3), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.gsr_bake_grid_workspace_bytes(),), dtype=torch.uint8, device=dev)
    n = C.c_int(0)
    call("gsr_bake_grid", dev, P, pts.data_ptr(), cell.data_ptr(), centres.data_ptr(), size.data_ptr(), idx.data_ptr(), C.byref(n),
         ws.data_ptr(), ws.numel())
    return cell, centres[:n.value], size, idx[:n.value]


def bake_visibility(means3D, scales, rotations, opacity, cell, centres, dirs, workspace_bytes=None):
    """vis [C, n_dirs] = 1 - the alpha image of cell c's cube (without its own Gaussians) at each direction's nearest texel."""
    dev = means3D.device
    P, Cn = means3D.shape[0], centres.shape[0]
    vis = torch.empty((Cn, dirs.shape[0]), dtype=torch.float32, device=dev)
    if P == 0 or Cn == 0:
        return vis
    f32 = lambda t: t.detach().float().contiguous()  # noqa: E731
    means3D, scales, rotations, opacity = f32(means3D), f32(scales), f32(rotations), f32(opacity).reshape(-1)
    views, projs, _ = cube_cameras(centres)
    texel = cube_nearest_texel(dirs).to(torch.int32).to(dev).contiguous()
    scene = _lib.BakeScene(P, Cn, means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(), opacity.data_ptr(), cell.data_ptr(),
                           views.data_ptr(), projs.data_ptr(), texel.data_ptr(), texel.numel())
    plan = torch.empty((lib.gsr_bake_plan_bytes(P, Cn),), dtype=torch.uint8, device=dev)
    inst = (C.c_ulonglong * 2)()
    stats = (C.c_ulonglong * 4)()
    call("gsr_bake_plan", dev, C.byref(scene), plan.data_ptr(), plan.numel(), inst)
    budget = WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    fixed = lib.gsr_bake_visibility_workspace_bytes(Cn, 0)
    cap = max(int(inst[1]), min(int(inst[0]), max(0, budget - fixed) // 20))
    ws = torch.empty((lib.gsr_bake_visibility_workspace_bytes(Cn, cap),), dtype=torch.uint8, device=dev)
    call("gsr_bake_visibility", dev, C.byref(scene), plan.data_ptr(), vis.data_ptr(), ws.data_ptr(), ws.numel(), stats)
    LAST_STATS.clear()
    LAST_STATS.update(instances=int(stats[0]), largest_batch=int(stats[1]), batches=int(stats[2]), capacity=int(stats[3]),
                      workspace_bytes=int(ws.numel() + plan.numel()), cells=Cn)
    return vis


def expand(cell, normal, dirs, vis, H=ENV_H, W=ENV_W):
    """occ [P, H, W, 1] = (dir . n > 0) * vis[cell]."""
    dev = vis.device
    P = cell.shape[0]
    occ = torch.empty((P, H, W, 1), dtype=torch.float32, device=dev)
    n = normal.detach().float().reshape(-1, 3).contiguous()
    d = dirs.detach().float().reshape(-1, 3).contiguous().to(dev)
    call("gsr_bake_expand", dev, P, d.shape[0], cell.data_ptr(), n.data_ptr(), d.data_ptr(), vis.data_ptr(), occ.data_ptr())
    return occ


def env_occlusion(occlusion, envmap):
    """clamp(sum_hw clamp(occlusion, 0, 1) * envmap, 0, 1).repeat(1, 3): [P, 16, 32, 1] against a grey [1, 16, 32] map -> [P, 3]."""
    if tuple(occlusion.shape[1:]) != (ENV_H, ENV_W, 1) or envmap.numel() != ENV_H * ENV_W:
        raise ValueError(f"env_occlusion: occlusion [P, {ENV_H}, {ENV_W}, 1] and a grey envmap [1, {ENV_H}, {ENV_W}] "
                         f"(got {tuple(occlusion.shape)} and {tuple(envmap.shape)})")
    dev = occlusion.device
    occ = occlusion.detach().float().contiguous()
    env = envmap.detach().float().reshape(-1).contiguous()
    P = occ.shape[0]
    out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    call("gsr_bake_env_reduce", dev, P, occ.data_ptr(), env.data_ptr(), out.data_ptr())
    return out


def _bake_fused(gaussians, means3D, normal, workspace_bytes=None):
    dev = means3D.device
    if not means3D.is_cuda:
        raise RuntimeError("bake_set: tensors must live on a HIP device (fused=False runs the reference's algorithm)")
    P = means3D.shape[0]
    if P == 0:
        return torch.zeros((0, ENV_H, ENV_W, 1), device=dev)
    cell, centres, _, _ = grid_cells(means3D)
    _, dirs = get_envmap_dirs()
    dirs = dirs.reshape(-1, 3).to(dev)
    vis = bake_visibility(means3D, gaussians.get_scaling, gaussians.get_rotation, gaussians.get_opacity, cell, centres, dirs,
                          workspace_bytes)
    return expand(cell, normal, dirs, vis)


def _bake_reference(gaussians, means3D, normal, H, W):
    """baking.py:136-309 as written, through diff_gaussian_rasterization._C (6 rasterizer calls per occupied cell)."""
    from .diff_gaussian_rasterization import _C
    dev = means3D.device
    res = 32
    bg_color = torch.zeros([3, res, res], device=dev)
    points = means3D
    grid_centers, grid_sizes, pc_grid_indices, unique_indices = pc_to_grid(points, 10)
    num_grid = grid_centers.shape[0]
    views, projs, campos = cube_cameras(grid_centers)
    opacity = gaussians.get_opacity
    shs = gaussians.get_features
    scales = gaussians.get_scaling
    rots = gaussians.get_rotation
    solid_angles, envmap_dirs = get_envmap_dirs()
    envmap_dirs = envmap_dirs.to(dev)
    _occlusion = torch.zeros((opacity.shape[0], H, W, 1), device=opacity.device)
    dot_map = ((envmap_dirs * normal.unsqueeze(1).unsqueeze(1)).sum(dim=-1, keepdim=True) > 0)
    for grid_id in range(num_grid):
        grid_mask = (pc_grid_indices == grid_id).int()
        render_mask = pc_grid_indices != grid_id
        opacity_cubemap = []
        valid_means3D = means3D[render_mask]
        valid_opacity = opacity[render_mask]
        valid_scales = scales[render_mask]
        valid_rots = rots[render_mask]
        for r_idx in range(6):
            (num_rendered, rendered_image, depth_map, opacity_map, radii, *_) = _C.rasterize_gaussians(
                bg_color, valid_means3D, torch.Tensor([]), valid_opacity, valid_scales, valid_rots, 1.0, torch.Tensor([]),
                views[grid_id, r_idx], projs[grid_id, r_idx], 1.0, 1.0, res, res, shs, gaussians.active_sh_degree,
                campos[grid_id, r_idx], False, False)
            opacity_cubemap.append(opacity_map.permute(1, 2, 0))
        opacity_envmap = cube_nearest(torch.stack(opacity_cubemap), envmap_dirs)  # dr.texture(..., filter_mode="nearest")
        grid_mask_expanded = (grid_mask.unsqueeze(1).unsqueeze(1).unsqueeze(1)).expand(grid_mask.shape[0], H, W, 1)
        _occlusion += grid_mask_expanded * (1 - opacity_envmap)
    return dot_map * _occlusion


def bake_set(view, gaussians, means3D, normal, H, W, light_map=None, fused=True, workspace_bytes=None):
    """The reference's bake_set: occlusion [P, H, W, 1] of the posed Gaussians `means3D` with unit normals `normal` [P, 3],
    stored on `view` (view.set_occlusion, or view.occlusion) and returned.  Only H, W = 16, 32 exist (the reference cannot
    broadcast other sizes either).  light_map is unused, as in the reference.  fused=False: the reference's algorithm through
    6 rasterizer calls per cell.  workspace_bytes: the visibility workspace budget (default WORKSPACE_BYTES)."""
    if (int(H), int(W)) != (ENV_H, ENV_W):
        raise ValueError(f"bake_set: only H, W = {ENV_H}, {ENV_W} are supported (the envmap directions are {ENV_H} x {ENV_W}); "
                         f"got {H}, {W}")
    with torch.no_grad():
        if fused:
            occlusion = _bake_fused(gaussians, means3D, normal, workspace_bytes)
        else:
            occlusion = _bake_reference(gaussians, means3D, normal, ENV_H, ENV_W)
    if hasattr(view, "set_occlusion"):
        view.set_occlusion(occlusion)
    else:
        view.occlusion = occlusion
    return occlusion
