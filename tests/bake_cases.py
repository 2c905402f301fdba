"""Seeded inputs and the float64 side of the occlusion-bake parity tests (tests/test_gpu_bake_f64.py; their promises are asserted
without a GPU in tests/test_bake_cases_host.py).  Everything is numpy float32 -- what the kernels are given -- built on the CPU;
of the package only the host helpers of mygauhuman_amd.baking are used (cube_cameras, get_canonical_rays, cube_nearest_texel,
pc_to_grid).

The float64 side is tests/raster_reference.py aimed at the cube: face f of cell k is a 32 x 32 camera with tanfov 1 and the
matrices of baking.cube_cameras, the cell's own Gaussians left out, and vis = 1 - alpha.  Its margin mask marks the texels where
a discrete decision is too close to its threshold for float32 and float64 to have to agree.

What a scene promises (the host test asserts each with the reference alone):
  * body, box     at most 5 % of the compared texels in the margin mask, at most 20 % of any (cell, face); terminated texels,
                  0.99-clamped texels, texels no Gaussian reaches, and a face that sees nothing at all;
  * lengths       (face, tile) t of cell 0 holds exactly LENGTHS[t] Gaussians and every Gaussian lies in exactly one tile, so the
                  list of that tile has that length: the 64-entry walk batches and the three sort back-ends (<= 512, <= 2,048,
                  longer) at and around their edges; cell 1 sees nothing;
  * planted       per face one Gaussian each side of the z <= 0.2 cull, Gaussians behind the camera, centres outside the face
                  whose footprint reaches in (inside and beyond the 1.3 frustum clamp), centres on the tile seam and on the face
                  corner, a Gaussian over all four tiles and a dense front layer that terminates part of the face;
  * the direction sets name the texels they are meant to (per-tile counts of the plan, -1 for a zero or NaN direction).
"""
import functools
import types

import numpy as np
import torch

from mygauhuman_amd import baking
from tests import raster_reference as rr

F32 = np.float32
N = baking.FACE                      # 32
TEXELS = 6 * N * N                   # 6,144
BODY_SEED, BOX_SEED, LENGTHS_SEED, PLANTED_SEED = 2, 2, 5, 0
# list length of (face, tile) t = face * 4 + tile_y * 2 + tile_x of the scene "lengths"
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 320, 511, 512, 513, 700, 1, 2047, 2048, 2049, 2100, 7, 200, 448, 384, 0, 65]
# needed pixels per (face, tile) that the plan direction set holds at least once each
PLAN_COUNTS = (0, 1, 63, 64, 65, 128, 129, 192, 193, 255, 256)
_BG = np.zeros(3, F32)


@functools.lru_cache(maxsize=None)
def _origin_rotations():
    """[6, 3, 3] float64: p_view = p_world @ R[f] for the cube at the origin (signed permutations)."""
    views, _, _ = baking.cube_cameras(torch.zeros((1, 3)))
    return views[0, :, :3, :3].numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def full_cube_dirs():
    """[6144, 3] float32: the ray through every texel centre, in texel order (cube_nearest_texel gives arange(6144))."""
    views, _, _ = baking.cube_cameras(torch.zeros((1, 3)))
    rays = baking.get_canonical_rays(N, N, 1.0, 1.0)
    return torch.cat([rays @ views[0, f, :3, :3].T for f in range(6)]).float().contiguous()


def pixel_to_world(f, px, py, z):
    """World position (float64) of face f's pixel coordinate (px, py) at view depth z, for the cube at the origin."""
    px, py, z = (np.asarray(a, np.float64) for a in (px, py, z))
    view = np.stack([((2 * px + 1) / N - 1) * z, ((2 * py + 1) / N - 1) * z, z], -1)
    return view @ _origin_rotations()[f].T


# ---- the float64 side --------------------------------------------------------------------------------------------------------
def face_camera(views, projs, campos, k, f):
    return dict(W=N, H=N, tanfovx=1.0, tanfovy=1.0, viewmatrix=views[k, f].numpy(), projmatrix=projs[k, f].numpy(),
                campos=campos[k, f].numpy())


def _gaussians(means, scales, rots, opac, keep):
    n = int(keep.sum())
    return dict(means3D=means[keep], opacities=opac.reshape(-1)[keep], scales=scales[keep], rotations=rots[keep],
                shs=np.zeros((n, 1, 3), F32), sh_degree=0)


def reference_visibility(means, scales, rots, opac, cell, centres, cells):
    """The float64 visibility of the listed cells: vis [K, 6144] = 1 - alpha, the margin mask and the statistics terminated,
    clamped, n_contrib (all [K, 6144]) of raster_reference.forward per face, and `faces`: per (row, face) the kept Gaussians' ids
    with their radii, txtz, tytz, z and the frustum limit."""
    views, projs, campos = baking.cube_cameras(torch.as_tensor(np.asarray(centres, F32)))
    K = len(cells)
    out = types.SimpleNamespace(vis=np.ones((K, TEXELS)), margin=np.zeros((K, TEXELS), bool), terminated=np.zeros((K, TEXELS), bool),
                                clamped=np.zeros((K, TEXELS), bool), n_contrib=np.zeros((K, TEXELS), np.int64), faces={})
    for i, k in enumerate(cells):
        keep = np.asarray(cell) != k
        if not keep.any():
            continue
        g = _gaussians(means, scales, rots, opac, keep)
        for f in range(6):
            with np.errstate(invalid="ignore"):  # a centre in the camera's z = 0 plane has no pixel (NaN); it is culled by its z
                r = rr.forward(face_camera(views, projs, campos, k, f), g, _BG, "sh")
            s = slice(f * N * N, (f + 1) * N * N)
            out.vis[i, s] = 1.0 - r["alpha"].reshape(-1)
            for name in ("margin", "terminated", "clamped", "n_contrib"):
                getattr(out, name)[i, s] = r[name].reshape(-1)
            out.faces[(i, f)] = dict(ids=np.nonzero(keep)[0], radii=r["radii"], txtz=r["txtz"], tytz=r["tytz"], z=r["z"],
                                     limx=r["limx"], limy=r["limy"])
    return out


def reference_rects(means, scales, rots, opac, centre):
    """Per face of a cube at `centre`: (alive [P], x0, y0, x1, y1 [P]) of the float64 tile rectangles of every Gaussian."""
    views, projs, campos = baking.cube_cameras(torch.as_tensor(np.asarray(centre, F32)).reshape(1, 3))
    g = _gaussians(means, scales, rots, opac, np.ones(len(means), bool))
    out = []
    for f in range(6):
        with np.errstate(invalid="ignore"):
            S = rr._Scene(face_camera(views, projs, campos, 0, f), g, _BG, "sh", grad=False)
        out.append((S.radii > 0,) + tuple(S.rect))
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def _scene(name, means, scales, rots, opac, cell, centres, **extra):
    c = lambda a, t=F32: np.ascontiguousarray(a, t)  # noqa: E731
    return types.SimpleNamespace(name=name, means=c(means), scales=c(scales), rots=c(rots), opac=c(opac), cell=c(cell, np.int32),
                                 centres=c(centres), cells=list(range(len(centres))), **extra)


def _quats(rng, P):
    q = rng.normal(0, 1, (P, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)


def _opacities(rng, P):
    """sigmoid(normal(0.5, 1.5)) with every ninth planted beside (not on) the 1/255 and 0.99 thresholds."""
    o = (1.0 / (1.0 + np.exp(-rng.normal(0.5, 1.5, P)))).astype(F32)
    for k, v in enumerate((1.02 / 255.0, 0.98 / 255.0, 0.99, 1.0)):
        o[k::9] = v
    return o


def _five_cells(name, means, scales, rots, opac):
    """The first, last and C/3, C/2, 2C/3-th occupied cells of pc_to_grid as cells 0..4; every other Gaussian is labelled 5, which
    no listed cell excludes (what the reference does for the Gaussians of foreign cells)."""
    centres, _, inv, _ = baking.pc_to_grid(torch.from_numpy(means), 10)
    C = centres.shape[0]
    chosen = [0, C // 3, C // 2, (2 * C) // 3, C - 1]
    cell = np.full(len(means), 5, np.int32)
    for i, c in enumerate(chosen):
        cell[inv.numpy() == c] = i
    return _scene(name, means, scales, rots, opac, cell, centres.numpy()[chosen], grid_cells=C, chosen=chosen)


@functools.lru_cache(maxsize=None)
def body(seed=BODY_SEED):
    rng = np.random.default_rng(seed)
    P = 4000
    means = rng.normal(0, [0.15, 0.45, 0.1], (P, 3)).astype(F32)
    scales = np.exp(rng.normal(np.log(0.03), 0.3, (P, 3))).astype(F32)
    return _five_cells("body", means, scales, _quats(rng, P), _opacities(rng, P))


@functools.lru_cache(maxsize=None)
def box(seed=BOX_SEED):
    rng = np.random.default_rng(seed)
    P = 2000
    means = rng.uniform(-1, 1, (P, 3)).astype(F32)
    scales = np.exp(rng.normal(np.log(0.04), 0.8, (P, 3))).astype(F32)
    scales[: P // 40] = 0.35  # these cover all four tiles of a face
    return _five_cells("box", means, scales, _quats(rng, P), _opacities(rng, P))


@functools.lru_cache(maxsize=None)
def lengths(seed=LENGTHS_SEED):
    """Tiny Gaussians well inside their tile (radius 2 around a centre 4..11 pixels from the tile's origin), faint enough that the
    long lists do not terminate.  All are labelled 1: cell 0 (at the origin) sees them all, cell 1 (far away) none."""
    rng = np.random.default_rng(seed)
    means, scales, opac, tile = [], [], [], []
    for t, n in enumerate(LENGTHS):
        f, ty, tx = t // 4, (t % 4) // 2, t % 2
        px, py = tx * rr.TILE + rng.uniform(4, 11, n), ty * rr.TILE + rng.uniform(4, 11, n)
        z = rng.uniform(0.5, 3, n)
        means.append(pixel_to_world(f, px, py, z))
        scales.append(np.exp(rng.normal(np.log(0.004), 0.3, (n, 3))) * z[:, None])
        opac.append(rng.uniform(0.006, 0.03, n))
        tile.append(np.full(n, t))
    order = rng.permutation(sum(LENGTHS))  # the Gaussian id carries nothing about the tile or the depth
    means, scales, opac, tile = (np.concatenate(a)[order] for a in (means, scales, opac, tile))
    P = len(means)
    return _scene("lengths", means, scales, _quats(rng, P), opac, np.ones(P, np.int32), [[0, 0, 0], [50, 50, 50]], tile=tile)


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED):
    """One camera cell at the origin; the same plants in every face's view space (depths jittered per face, so that the plants of
    different faces do not tie in depth).  `roles` maps a role to its Gaussian ids, `face_of` gives the face a plant was made for."""
    rng = np.random.default_rng(seed)
    rows, roles, face_of = [], {}, []

    def plant(role, f, view, s, o):
        roles.setdefault(role, []).append(len(rows))
        face_of.append(f)
        rows.append((np.asarray(view, np.float64) @ _origin_rotations()[f].T, np.asarray(s) * np.array([1.0, 0.8, 1.2]), o))

    def at_pixel(px, py, z):
        return [((2 * px + 1) / N - 1) * z, ((2 * py + 1) / N - 1) * z, z]

    for f in range(6):
        j = lambda z: z * rng.uniform(0.95, 1.05)  # noqa: E731
        zc, zk = 0.2 * 0.99, 0.2 * 1.01
        plant("near_culled", f, [-0.5 * zc, -0.5 * zc, zc], 0.01, 0.8)
        plant("near_kept", f, [0.5 * zk, -0.5 * zk, zk], 0.01, 0.8)
        plant("behind", f, [0.1, 0.1, -j(1.0)], 0.05, 0.8)
        plant("behind", f, [j(0.3), j(0.36), -0.05], 0.05, 0.8)
        z = j(1.0)
        plant("outside_reaching_in", f, [1.15 * z, 0.2 * z, z], 0.15 * z, 0.8)     # 1 < |x / z| < 1.3
        z = j(1.0)
        plant("clamped_x", f, [1.6 * z, -0.3 * z, z], 0.4 * z, 0.8)               # beyond the 1.3 clamp in x
        z = j(1.1)
        plant("clamped_y", f, [0.4 * z, -1.5 * z, z], 0.4 * z, 0.8)               # and in y
        plant("seam_four_tiles", f, at_pixel(15.5, 15.5, j(1.5)), 0.05, 0.7)
        plant("seam_two_tiles", f, at_pixel(15.5, 6.0, j(1.7)), 0.05, 0.7)
        z = j(1.2)
        plant("corner", f, at_pixel(-0.5, -0.5, z), 0.1 * z, 0.9)
        z = j(1.3)
        plant("corner", f, at_pixel(31.5, 31.5, z), 0.1 * z, 0.9)
        z = j(2.0)
        plant("four_tiles", f, at_pixel(20.0, 12.0, z), 0.25 * z, 0.3)
        for _ in range(60):  # a dense, nearly opaque front layer over pixels 3..10 x 19..28
            z = rng.uniform(0.5, 0.6)
            plant("dense", f, at_pixel(rng.uniform(3, 10), rng.uniform(19, 28), z), 0.125 * z, 0.9)
    means, scales, opac = (np.array([r[k] for r in rows]) for k in range(3))
    P = len(rows)
    return _scene("planted", means, scales, _quats(rng, P), opac, np.ones(P, np.int32), [[0, 0, 0]],
                  roles={k: np.array(v) for k, v in roles.items()}, face_of=np.array(face_of))


SCENES = {"body": body, "box": box, "lengths": lengths, "planted": planted}


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_visibility of a scene, computed once per process and shared: do not write to it."""
    s = SCENES[name]()
    return reference_visibility(s.means, s.scales, s.rots, s.opac, s.cell, s.centres, s.cells)


@functools.lru_cache(maxsize=None)
def box_three_cells():
    """The box scene with its first three chosen cells only (labels 3 and 4 stay: no listed cell excludes them)."""
    s = box()
    return _scene("box3", s.means, s.scales, s.rots, s.opac, s.cell, s.centres[:3])


# ---- direction sets over the full cube: (dirs [n, 3] float32 tensor, the texel of each direction or -1) ---------------------
def tile_of_texel(texel):
    """(face, tile) index face * 4 + tile_y * 2 + tile_x of texels."""
    texel = np.asarray(texel)
    f, y, x = texel // (N * N), (texel // N) % N, texel % N
    return f * 4 + (y // rr.TILE) * 2 + x // rr.TILE


def _from_texels(texel):
    texel = np.asarray(texel, np.int64)
    return full_cube_dirs()[torch.from_numpy(texel)].contiguous(), texel


@functools.lru_cache(maxsize=None)
def plan_counts(seed=0):
    """Needed pixels per (face, tile): every count of PLAN_COUNTS and 13 others, shuffled."""
    rng = np.random.default_rng(seed)
    counts = np.array(list(PLAN_COUNTS) + list(rng.integers(2, 255, 24 - len(PLAN_COUNTS))))
    rng.shuffle(counts)
    return tuple(int(c) for c in counts)


def dirs_plan(seed=0):
    rng = np.random.default_rng(seed + 1)
    texel = []
    for t, n in enumerate(plan_counts(seed)):
        f, ty, tx = t // 4, (t % 4) // 2, t % 2
        local = rng.choice(rr.TILE * rr.TILE, n, replace=False)
        texel.append(f * N * N + (ty * rr.TILE + local // rr.TILE) * N + tx * rr.TILE + local % rr.TILE)
    return _from_texels(rng.permutation(np.concatenate(texel)))


def dirs_single():
    return _from_texels([3 * N * N + 17 * N + 30])


def dirs_repeated(seed=0):
    """513 directions drawn from 200 texels."""
    rng = np.random.default_rng(seed + 2)
    return _from_texels(rng.choice(rng.choice(TEXELS, 200, replace=False), 513))


def dirs_production_and_invalid():
    """The 16 x 32 equirect directions of bake_set, a zero vector in the middle and a direction with a NaN component at the end."""
    _, d = baking.get_envmap_dirs()
    d = d.reshape(-1, 3).float()
    dirs = torch.cat([d[:100], torch.zeros((1, 3)), d[100:], torch.tensor([[0.3, float("nan"), -1.0]])]).contiguous()
    texel = baking.cube_nearest_texel(d).numpy()
    return dirs, np.concatenate([texel[:100], [-1], texel[100:], [-1]])


DIRECTION_SETS = {"plan": dirs_plan, "single": dirs_single, "repeated": dirs_repeated, "production_and_invalid": dirs_production_and_invalid}
