"""Float64 restatement of the environment light's own share of a PBR step (mygauhuman_amd.pbr: CubemapLight.grey_envmap,
env_tv_loss, view_dirs), built on the cube lookup of tests/pbr_reference.py and numpy's inverse.  CPU only."""
import numpy as np
import torch

from tests import pbr_reference as R

# torchvision.transforms.functional.rgb_to_grayscale
GREY_WEIGHTS = np.array([0.2989, 0.587, 0.114])


def _lookup(base, dirs):
    """base [6, N, N, 3] (float64 torch, any grad) at dirs [h, w, 3] -> [h, w, 3]."""
    d = torch.as_tensor(np.asarray(dirs, np.float64))
    return R.texture(base[None], d[None], filter_mode="linear", boundary_mode="cube")[0]


def grey_of(rgb):
    """The grey value of clamp(rgb [..., 3], 0, 1) -> [...]."""
    return (np.clip(np.asarray(rgb, np.float64), 0.0, 1.0) * GREY_WEIGHTS).sum(-1)


def grey_envmap(base, res=(16, 32), dirs=None):
    """[1, h, w]: the grey environment map of base [6, N, N, 3] over export_envmap's grid of `res` (or over dirs [h, w, 3])."""
    d = R.envmap_dirs(list(res)) if dirs is None else dirs
    e = _lookup(torch.as_tensor(np.asarray(base, np.float64)), d)
    return grey_of(e.numpy())[None]


def env_tv_loss(base, dirs):
    """base: float64 torch [6, N, N, 3] (its autograd supplies d_base); dirs [h, w, 3] -> 0-dim."""
    e = _lookup(base, dirs)
    return ((e[1:] - e[:-1]) ** 2).mean() + ((e[:, 1:] - e[:, :-1]) ** 2).mean()


def view_dirs(canonical_rays, world_view_transform, H, W):
    """-(c2w[:3, :3] @ ray / max(|ray|, 1e-12)) per pixel, c2w = inverse(world_view_transform.T) -> [H, W, 3]."""
    rays = np.asarray(canonical_rays, np.float64)
    c2w = np.linalg.inv(np.asarray(world_view_transform, np.float64).T)
    unit = rays / np.maximum(np.linalg.norm(rays, axis=-1, keepdims=True), 1e-12)
    return -(unit @ c2w[:3, :3].T).reshape(H, W, 3)
