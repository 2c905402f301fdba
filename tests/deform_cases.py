"""Seeded inputs of the deform-path parity tests (tests/test_gpu_deform_f64.py; their promises are asserted without a GPU in
tests/test_deform_reference_host.py).  Everything is numpy float32 -- what the kernels are given -- and small: P <= 513, V <= 2049.

What a case promises (the host test asserts each in float64):
  * the world rotation R is a rotation times a mild shear and a non-uniform scale: singular values in [0.7, 1.4], not
    orthogonal (inverse(R) != R^T), Th non-zero;
  * the blended big-pose 3x3 of every point has a 2-norm condition number <= 20, except in the case "illcond", which promises
    50 .. 500.  (Two rotations an angle t apart, blended half and half, have the singular values 1, cos(t/2), cos(t/2): the
    promised range needs t between 177.7 and 179.8 degrees; the case uses joints at +89 and -89 degrees about one axis.)
  * "sparse" weights have 1 to 4 non-zero entries per row and exact zeros elsewhere, every fourth row one-hot;
  * the planted queries of the vertex-count cases have the nearest vertex they were planted for (V - 1; 1024; a tie of 1023 and
    1024 at exactly equal float32 distance, which the lower index wins);
  * in the temporal-cache case no unmoved point has a cache radius between 0 and 1e-5 (a radius is 0 or comfortably larger
    than the 1e-6 move), so the number of misses in frame 2 is known up to the zero-radius entries.
"""
import functools
import os

import numpy as np
import torch

from tests import deform_reference as dr

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARENTS_SMPL = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
BIG_POSE_ENTRIES = ((5, 45.0), (8, -45.0), (23, -30.0), (26, 30.0))   # index into the flat pose, degrees


@functools.lru_cache(maxsize=None)
def parents_smplx():
    return tuple(int(v) for v in np.load(os.path.join(GOLDEN, "lbs_smplx.npz"))["smpl_parents"])


def parents_of(J, tree="body"):
    if tree == "chain":
        return (-1,) + tuple(range(J - 1))
    if tree == "star":
        return (-1,) + (0,) * (J - 1)
    return {24: PARENTS_SMPL, 55: parents_smplx()}[J]


def big_pose(J):
    p = np.zeros(3 * J, F32)
    for k, deg in BIG_POSE_ENTRIES:
        if k < 3 * J:
            p[k] = np.deg2rad(deg)
    return p


def chain_f32(poses, joints, parents):
    """A [J,4,4] float32 of a pose: the float64 chain of the float32 inputs, rounded once (the kernels are GIVEN A)."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    return dr.pose_chain64(t(poses), t(joints), parents)[1].numpy().astype(F32)


def general_R(rng):
    """rotation x (identity + shear) x non-uniform scale."""
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    shear = np.eye(3)
    shear[0, 1], shear[1, 2] = 0.15, -0.1
    return (q @ shear @ np.diag([0.85, 1.0, 1.2])).astype(F32)


def nearest_f32(query, verts):
    """Brute-force nearest vertex in float32 by the kernels' expression (dx*dx + dy*dy) + dz*dz, first minimum wins (finite
    inputs; the host test holds it to the oracle's search)."""
    q, v = np.asarray(query, F32), np.asarray(verts, F32)
    d = q[:, None, :] - v[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return d2.argmin(1).astype(np.int32) if q.shape[0] else np.zeros(0, np.int32)


def well_scaled_g_world(rng, c):
    """The upstream gradient of the world points, chosen so that every point's contribution to d_off_pose -- g_q2 = Rp^T Rinv g,
    Rp the point's blended pose rotation -- has all three components between 0.5 and 1.5 in magnitude: a contribution is accurate
    relative to its vector, and an element of d_off_pose is the sum of only a few of them, so a component that happens to be tiny
    would put float32 noise of the whole vector on a scale (S_abs) of next to nothing."""
    P = c["query"].shape[0]
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    ids = torch.from_numpy(nearest_f32(c["query"], c["verts"]).astype(np.int64))
    Rp = dr.deform64(*[t(c[k]) for k in dr.LBS_INPUTS], ids, t(c["weights"]))["Ap"][:, :3, :3].numpy()
    g_q2 = rng.uniform(0.5, 1.5, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))
    g_src = np.linalg.solve(Rp.transpose(0, 2, 1), g_q2[..., None])[..., 0] if P else g_q2
    return (g_src @ np.asarray(c["R"], np.float64).T).astype(F32)


def _weights(rng, kind, V, J):
    if kind == "dense":
        w = rng.uniform(0, 1, (V, J)) ** 4
    elif kind == "sparse":
        w = np.zeros((V, J))
        for v in range(V):
            k = 1 if v % 4 == 0 else int(rng.integers(2, 5))
            w[v, rng.choice(J, k, replace=False)] = rng.uniform(0.05, 1, k)
    elif kind == "one_joint":
        w = np.zeros((V, J))
        w[:, 3] = 1.0
    elif kind == "twohot":      # joints 1 and 2, near-equal
        w = np.zeros((V, J))
        delta = rng.uniform(-0.002, 0.002, V)
        w[:, 1], w[:, 2] = 0.5 + delta, 0.5 - delta
    else:
        raise KeyError(kind)
    w = (w / w.sum(1, keepdims=True)).astype(F32)
    if kind in ("sparse", "one_joint"):   # a one-hot row is exactly 1
        single = (w != 0).sum(1) == 1
        w[single] = (w[single] != 0).astype(F32)
    return w


def _offsets(rng, kind, P, J):
    if kind is None:
        return None
    if kind == "small":
        return rng.normal(0, 0.002, (P, J)).astype(F32)
    off = rng.normal(0, 0.5, (P, J)).astype(F32)
    if kind == "saturated" and P:
        rows = np.arange(0, P, 2)   # every other row: the saturated rows are near zero ON THE SCALE of the ordinary rows' gradient
        off[rows, rng.integers(0, J, len(rows))] = 30.0
    elif kind == "equal":
        off[:] = rng.normal(0, 1, (P, 1)).astype(F32)
    return off


def make_lbs(J, P, V, seed, weights="dense", offsets="normal", normals=True, big="standard", queries="near"):
    rng = np.random.default_rng(seed)
    parents = parents_of(J)
    joints = rng.normal(0, 0.3, (J, 3)).astype(F32)
    bp = big_pose(J)
    if big == "opposed":           # joints 1 and 2 (both children of the root) at +89 and -89 degrees about z
        bp = np.zeros(3 * J, F32)
        bp[5], bp[8] = np.deg2rad(89.0), -np.deg2rad(89.0)
    pose = rng.normal(0, 0.2, 3 * J).astype(F32)
    verts = (rng.uniform(-1, 1, (V, 3)) * np.array([0.9, 0.9, 0.15])).astype(F32)
    if queries == "near":
        query = verts[rng.integers(0, V, P)] + rng.normal(0, 0.02, (P, 3))
    elif queries == "three":       # every point next to one of three vertices
        query = verts[np.array([3, 30, V - 1])[rng.integers(0, 3, P)]] + rng.normal(0, 0.002, (P, 3))
    else:
        raise KeyError(queries)
    c = dict(J=J, parents=parents, query=query.astype(F32), normals=rng.normal(0, 1, (P, 3)).astype(F32) if normals else None,
                loff=_offsets(rng, offsets, P, J), A_big=chain_f32(bp, joints, parents), A_pose=chain_f32(pose, joints, parents),
                off_big=rng.normal(0, 0.01, (V, 3)).astype(F32), off_shape=rng.normal(0, 0.01, (V, 3)).astype(F32),
                off_pose=rng.normal(0, 0.01, (V, 3)).astype(F32), R=general_R(rng), Th=np.array([0.1, -0.3, 2.5], F32),
                verts=verts, weights=_weights(rng, weights, V, J), g_world=rng.normal(0, 1, (P, 3)).astype(F32),
                g_transforms=rng.normal(0, 1, (P, 3, 3)).astype(F32), g_normals=rng.normal(0, 1, (P, 3)).astype(F32))
    c["g_world"] = well_scaled_g_world(rng, c)
    return c


P_TAILS = (0, 1, 63, 64, 65, 255, 256, 257, 513)      # LBS_BLOCK = 256, wave 64
V_TAILS = (1, 2, 1023, 1024, 1025, 2049)              # VTILE = 1024
JOINTS = (24, 55)

# name -> keyword arguments of make_lbs (J and the seed are added by lbs_case)
LBS_CASES = {f"P{P}": dict(P=P, V=97) for P in P_TAILS}
LBS_CASES.update({
    "no_offsets": dict(P=257, V=97, offsets=None),
    "no_normals": dict(P=257, V=97, normals=False),
    "bare": dict(P=257, V=97, offsets=None, normals=False),
    "sparse": dict(P=257, V=97, weights="sparse"),
    "sparse_no_offsets": dict(P=257, V=97, weights="sparse", offsets=None),
    "saturated": dict(P=257, V=97, weights="sparse", offsets="saturated"),
    "equal_offsets": dict(P=257, V=97, weights="sparse", offsets="equal"),
    "illcond": dict(P=257, V=97, weights="twohot", offsets="small", big="opposed"),
    "single_vertex": dict(P=257, V=1),
    "clustered": dict(P=257, V=65, queries="three"),
    # (no offsets: with every weight on one joint the softmax adjoint bw (g - <bw, g>) is zero up to the 1e-9 of the logarithm, a
    # tensor of float32 noise around 1e-9 of the incoming gradient; one-hot rows WITH offsets are part of "sparse")
    "one_joint": dict(P=257, V=97, weights="one_joint", offsets=None),
})
SWITCH_CASES = {(True, True): "P257", (True, False): "no_offsets", (False, True): "no_normals", (False, False): "bare"}  # (normals, offsets)


@functools.lru_cache(maxsize=None)
def lbs_case(name, J):
    """Built once and shared: callers must not write to it."""
    seed = 1000 * J + sorted(LBS_CASES).index(name)
    return make_lbs(J=J, seed=seed, **LBS_CASES[name])


_REFERENCES = {}


def reference(oracle, c, key, loss="all"):
    """(ids, float64 (outputs, grads, s_abs), float32 (outputs, grads, s_abs)) of a case, computed once per `key` and shared.
    ids = the exact float32 search of the oracle."""
    key = (key, loss)
    if key not in _REFERENCES:
        ids = oracle.nearest_vertex(c["query"], c["verts"]) if c["query"].shape[0] else np.zeros(0, np.int32)
        _REFERENCES[key] = (ids, dr.deform_reference(c, ids, torch.float64, loss), dr.deform_reference(c, ids, torch.float32, loss))
    return _REFERENCES[key]


def blended_big_condition(c, ids):
    """2-norm condition number of every point's blended big-pose 3x3, float64."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    bw = dr.deform64(*[t(c[k]) for k in dr.LBS_INPUTS], torch.as_tensor(np.asarray(ids, np.int64)), t(c["weights"]))["bweights"].numpy()
    Rb = np.einsum("pj,jrc->prc", bw, np.asarray(c["A_big"], np.float64)[:, :3, :3])
    s = np.linalg.svd(Rb, compute_uv=False)
    return s[:, 0] / s[:, -1]


# ------------------------------------------------------------------------------------------------------ vertex-count tails
@functools.lru_cache(maxsize=None)
def vtail_case(J, V):
    """P = 257 queries against V vertices with planted answers: c["planted"] = {"last": rows whose nearest vertex is V - 1,
    "first_of_tile": rows whose nearest vertex is 1024, "tie": rows at exactly equal float32 distance from 1023 and 1024}."""
    c = dict(make_lbs(J, 257, V, seed=7000 + 10 * V + J))
    rng = np.random.default_rng(V)
    verts, query = c["verts"].copy(), c["query"].copy()
    planted = {"last": np.arange(0, 12), "first_of_tile": np.zeros(0, np.int64), "tie": np.zeros(0, np.int64)}
    if V >= 1025:   # the pair sits outside the box of the other vertices; x = +-a is exact, the queries of the tie have x = 0
        a = F32(0.0625)
        verts[1023], verts[1024] = (a, 2.0, 0.05), (-a, 2.0, 0.05)
        planted["first_of_tile"], planted["tie"] = np.arange(12, 24), np.arange(24, 40)
        query[planted["first_of_tile"]] = verts[1024] + np.array([-0.01, 0, 0]) + rng.normal(0, 0.003, (12, 3))
        query[planted["tie"]] = np.array([0, 2.0, 0.05]) + rng.normal(0, 0.02, (16, 3)) * np.array([0, 1, 1])
    last = verts[V - 1] + (np.array([-0.01, 0, 0]) if V == 1025 else 0) + rng.normal(0, 1e-4, (12, 3))
    query[planted["last"]] = last
    c.update(verts=verts, query=query.astype(F32), planted=planted)
    return c


# ------------------------------------------------------------------------------------------------------ temporal cache
CACHE_MOVED = (0, 63, 64, 255, 256)
GRID_RES = 48   # csrc/lbs.hip: cells along the longest bounding-box axis


@functools.lru_cache(maxsize=None)
def cache_case(J):
    """P = 257, V = 300 with one duplicated vertex (10 == 200) and three queries (5, 6, 7) next to it: their entries have radius
    0.  c["query2"]: frame 2 -- the points CACHE_MOVED moved by several vertex spacings, every other point by 1e-6."""
    c = dict(make_lbs(J, 257, 300, seed=8000 + J))
    rng = np.random.default_rng(81)
    verts, query = c["verts"].copy(), c["query"].copy()
    verts[200] = verts[10]
    query[5:8] = verts[10] + rng.normal(0, 0.005, (3, 3))
    query = query.astype(F32)
    query2 = query + F32(1e-6)
    query2[list(CACHE_MOVED)] = query[list(CACHE_MOVED)] + np.array([0.5, -0.4, 0.1], F32)
    c.update(verts=verts, query=query, query2=query2.astype(F32))
    return c


def cache_radii(c):
    """Per point of frame 1, float64: (rho from the two nearest distances, rho with the bound of the unexamined rings in place of
    the second distance where that is smaller -- what the search may report instead)."""
    q, v = np.asarray(c["query"], np.float64), np.asarray(c["verts"], np.float64)
    d = np.sqrt(((q[:, None, :] - v[None, :, :]) ** 2).sum(-1))
    d.sort(axis=1)
    d1, D2 = d[:, 0], d[:, 1]
    h = (v.max(0) - v.min(0)).max() / GRID_RES
    rings = (np.arange(1, GRID_RES + 2) - 1e-3) * h                  # (r - 1) h - 1e-3 h for r = 2 ..
    ring = np.array([rings[rings > x].min() for x in d1])
    rho = lambda other: np.maximum(0.49 * (other - d1) - 4e-6 * other - 1e-12, 0.0)  # noqa: E731
    return rho(D2), rho(np.minimum(D2, ring))


# ------------------------------------------------------------------------------------------------------ non-finite points
NONFINITE_ROWS = {0: np.nan, 100: np.inf, 256: 3e19}


@functools.lru_cache(maxsize=None)
def nonfinite_case(J):
    """(the case with rows 0 / 100 / 256 of query NaN / +inf / 3e19, the same case with those rows ordinary)."""
    fin = lbs_case("P257", J)
    bad = dict(fin)
    q = fin["query"].copy()
    for row, val in NONFINITE_ROWS.items():
        q[row] = val
    bad["query"] = q
    return bad, fin


# ------------------------------------------------------------------------------------------------------ pose chain
POSE_TREES = (("smpl", 24), ("smplx", 55), ("chain", 64), ("star", 64), ("pair", 2))
POSE_KINDS = ("zero", "big", "tiny7", "tiny4", "axis", "near_pi", "normal")
NEAR_PI = (np.pi - 1e-3, np.pi + 1e-3, 2 * np.pi - 0.1)


@functools.lru_cache(maxsize=None)
def pose_case(tree, J, kind):
    rng = np.random.default_rng(100 * J + POSE_KINDS.index(kind) + (7 if tree == "star" else 0))
    parents = parents_of(J, tree if tree in ("chain", "star") else "body") if J != 2 else (-1, 0)
    unit = rng.normal(0, 1, (J, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    if kind == "zero":
        poses = np.zeros((J, 3))
    elif kind == "big":
        poses = big_pose(J).reshape(J, 3)
    elif kind in ("tiny7", "tiny4"):   # odd joints tiny, even joints ordinary: with EVERY rotation the identity to 1e-7, d_joints
        poses = rng.normal(0, 0.4, (J, 3))   # is zero up to float32 noise (A.t = G.t - G.R J cancels) and has no scale to be held to
        poses[1::2] = unit[1::2] * (1e-7 if kind == "tiny7" else 1e-4)
    elif kind == "axis":
        poses = np.zeros((J, 3))
        poses[np.arange(J), np.arange(J) % 3] = rng.normal(0, 0.4, J)
    elif kind == "near_pi":
        poses = unit * np.array(NEAR_PI)[np.arange(J) % 3][:, None]
    else:
        poses = rng.normal(0, 0.4, (J, 3))
    return dict(J=J, parents=parents, poses=poses.astype(F32), joints=rng.normal(0, 0.3, (J, 3)).astype(F32),
                correct_Rs=(np.eye(3) + rng.normal(0, 0.1, (J - 1, 3, 3))).astype(F32),
                wA=rng.normal(0, 1, (J, 4, 4)).astype(F32), wR=rng.normal(0, 1, (J, 3, 3)).astype(F32))


_POSE_REFERENCES = {}


def pose_reference(tree, J, kind, with_correct, loss):
    """(float64, float32) results of dr.pose_reference, computed once and shared."""
    key = (tree, J, kind, with_correct, loss)
    if key not in _POSE_REFERENCES:
        c = pose_case(tree, J, kind)
        _POSE_REFERENCES[key] = (dr.pose_reference(c, torch.float64, with_correct, loss), dr.pose_reference(c, torch.float32, with_correct, loss))
    return _POSE_REFERENCES[key]
