"""Float64 restatement of the bake's nearest cube lookup (dr.texture(..., filter_mode="nearest", boundary_mode="cube") as this
project reads a cube: DESIGN.md sections 10 and 11), the inputs of the bake fixture, and the per-cell form the fixture stores its outputs in (tests/golden/make_golden_bake.py)."""
import numpy as np

from tests.pbr_reference import _face_coords, _face_of


def nearest_texel(dirs, N):
    """Texel index face * N * N + y * N + x of the texel containing each direction [n, 3]; -1 for a zero / non-finite one."""
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    f = _face_of(x, y, z)
    a, b, m = _face_coords(f, x, y, z)
    valid = (m > 0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(m)
    ms = np.where(valid, m, 1.0)
    u = np.clip((np.where(valid, a, 0.0) / ms + 1.0) * 0.5, 0.0, 1.0)
    v = np.clip((np.where(valid, b, 0.0) / ms + 1.0) * 0.5, 0.0, 1.0)
    tx = np.minimum(np.floor(u * N), N - 1).astype(np.int64)
    ty = np.minimum(np.floor(v * N), N - 1).astype(np.int64)
    return np.where(valid, (f * N + ty) * N + tx, -1)


def texture_nearest(tex, uv):
    """dr.texture(tex [1, 6, N, N, C], uv [1, H, W, 3], filter_mode="nearest", boundary_mode="cube") -> [1, H, W, C]."""
    import torch
    t = tex[0]
    N, Cn = t.shape[1], t.shape[3]
    idx = nearest_texel(uv.detach().cpu().numpy().reshape(-1, 3), N)
    flat = t.reshape(-1, Cn)
    out = flat[torch.from_numpy(np.maximum(idx, 0))] * torch.from_numpy(idx >= 0).to(flat.dtype)[:, None]
    return out.reshape(1, uv.shape[1], uv.shape[2], Cn)


def scene(name):
    """(means3D, scales, rotations, opacity, normal) float32 of a fixture scene (rebuilt by the tests, not stored)."""
    rng = np.random.default_rng({"blob": 1, "clumps": 2}[name])
    if name == "blob":  # a small body-like cloud: 300 Gaussians over a hundred-odd cells
        P = 300
        means = rng.normal(0, [0.15, 0.45, 0.1], (P, 3))
        scales = np.exp(rng.normal(np.log(0.03), 0.3, (P, 3)))
    else:  # 500 larger, denser Gaussians in 27 clumps on a 3 x 3 x 3 lattice: few cells, lists that terminate
        P = 500
        centre = rng.integers(0, 3, (P, 3)) - 1.0
        means = centre + rng.normal(0, 0.04, (P, 3))
        scales = np.exp(rng.normal(np.log(0.08), 0.5, (P, 3)))
    rots = rng.normal(0, 1, (P, 4))
    rots /= np.linalg.norm(rots, axis=1, keepdims=True)
    opac = 1 / (1 + np.exp(-rng.normal(0.5, 1.5, (P, 1))))
    n = rng.normal(0, 1, (P, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f(means), f(scales), f(rots), f(opac), f(n)


SCENES = ("blob", "clumps")
CAMERA_CELLS = 8  # cells whose cube matrices the fixture keeps


def hemisphere_mask(dirs, normal):
    """The reference's dot_map: (dirs [H, W, 3] * normal [P, 1, 1, 3]).sum(-1, keepdim=True) > 0, in torch on the CPU."""
    import torch
    return ((torch.as_tensor(dirs) * torch.as_tensor(normal).unsqueeze(1).unsqueeze(1)).sum(dim=-1, keepdim=True) > 0).numpy()


def visibility_of(occ, cell, mask, C):
    """The per-cell visibility [C, H * W] the occlusion [P, H, W, 1] = mask * vis[cell] was made from; NaN where no Gaussian of the
    cell faces the direction.  Raises if the occlusion does not have that form."""
    P = occ.shape[0]
    o, m = occ.reshape(P, -1), mask.reshape(P, -1)
    vis = np.full((C, o.shape[1]), np.nan, np.float32)
    for c in range(C):
        rows = cell == c
        seen = m[rows].any(0)
        vals = np.where(m[rows], o[rows], np.nan)
        first = vals[np.argmax(m[rows], 0), np.arange(o.shape[1])]
        assert np.all((vals == first[None]) | np.isnan(vals)), "occlusion differs between the Gaussians of one cell"
        vis[c, seen] = first[seen]
    rebuilt = occlusion_of(vis, cell, mask)
    assert np.array_equal(rebuilt, occ.reshape(rebuilt.shape)), "occlusion is not mask * vis[cell]"
    return vis


def occlusion_of(vis, cell, mask):
    """occlusion [P, H, W, 1] = mask * vis[cell] (0 where masked)."""
    P = cell.shape[0]
    m = mask.reshape(P, -1)
    v = vis[cell]
    return np.where(m, v, np.float32(0.0)).astype(np.float32).reshape(mask.shape)
