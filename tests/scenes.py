"""Seeded rasterizer scenes under general cameras and at the edges of projection and blending.

Every family is drawn in camera space -- pixel position, view depth, scale, orientation -- and then moved to world space
with the camera's pose, so what a family covers does not depend on the pose.  The camera (`general_camera`) has pitch, roll
and yaw, a translation, a principal point off the image centre by more than 10 % of W and H, fy != fx, and optionally skew:
every entry of the view and projection matrices is driven.

  general       Gaussians spread over the image and a little beyond it
  general_skew  the same with K[0,1] != 0
  frustum       means beyond +-1.3 tan(fov/2) on each of the four sides (the clamp of the EWA Jacobian) with splats large
                enough to reach the image, plus an interior population
  near          visible Gaussians at view z in (0.25, 0.6] whose radii exceed half the image, Gaussians at z < 0.17 (culled
                by the z <= 0.2 test) and a background population
  opaque        opacities in [0.99, 0.9999] in deep stacks: the 0.99 alpha clamp is active and lists end at T < 1e-4
  needle        scale ratios >= 1e3

Each scene returns (cam, g) in the layout of mygauhuman_amd.synthetic (g also holds cov3D / colors for the precomp mode).
"""
import math

import numpy as np

from mygauhuman_amd import cameras

FAMILIES = ("general", "general_skew", "frustum", "near", "opaque", "needle")
W_DEFAULT, H_DEFAULT = 128, 96


def _euler(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def general_K(W, H, skew=False):
    """fx for a 50 degree horizontal field, fy = 1.08 fx, principal point at (0.63 W, 0.38 H), skew 0.04 fx."""
    fx = W / (2.0 * math.tan(math.radians(25.0)))
    fy = 1.08 * fx
    return np.array([[fx, 0.04 * fx if skew else 0.0, 0.63 * W], [0, fy, 0.38 * H], [0, 0, 1]], np.float32)


def general_camera(W=W_DEFAULT, H=H_DEFAULT, seed=0, skew=False):
    """Camera-to-world rotation with yaw, pitch and roll of at least 15 degrees each, a world-to-camera translation of about
    one unit per axis."""
    rng = np.random.default_rng(seed + 500)
    ang = [s * math.radians(rng.uniform(15, 40)) for s in rng.choice([-1.0, 1.0], 3)]
    R = _euler(*ang)
    T = rng.uniform(0.5, 1.5, 3) * rng.choice([-1.0, 1.0], 3)
    return cameras.camera_from_K(W, H, general_K(W, H, skew), R, T), R, T


def _quat_of(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix."""
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = math.copysign(math.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = math.copysign(math.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = math.copysign(math.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    return np.array([w, x, y, z])


def _qmul(a, b):
    w1, x1, y1, z1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    w2, x2, y2, z2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_to_matrix(q):
    """Rotation matrices of unit quaternions (w, x, y, z), float64."""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                     1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                     1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


class _Builder:
    """Collects camera-space Gaussians: pixel (u, v) of the mean, view depth z, scales, opacity."""

    def __init__(self, cam, rng):
        self.cam, self.rng = cam, rng
        self.parts = []

    def add(self, u, v, z, scales, opac):
        self.parts.append((np.asarray(u, np.float64), np.asarray(v, np.float64), np.asarray(z, np.float64),
                           np.asarray(scales, np.float64), np.asarray(opac, np.float64)))

    def add_ratio(self, tx_over_z, ty_over_z, z, scales, opac):
        """Means given as t.x / t.z and t.y / t.z (what the frustum clamp tests) instead of pixels."""
        K = self.cam["K"].astype(np.float64)
        y = ty_over_z
        u = K[0, 0] * tx_over_z + K[0, 1] * y + K[0, 2]
        v = K[1, 1] * y + K[1, 2]
        self.add(u, v, z, scales, opac)

    def finish(self, R, T, deg=3):
        rng, K = self.rng, self.cam["K"].astype(np.float64)
        u, v, z, s, o = (np.concatenate([p[k] for p in self.parts]) for k in range(5))
        P = len(z)
        yz = (v - K[1, 2]) / K[1, 1]
        xz = (u - K[0, 2] - K[0, 1] * yz) / K[0, 0]
        t_cam = np.stack([xz * z, yz * z, z], 1)
        means = (R @ (t_cam - T).T).T  # t_cam = R^T p + T (getWorld2View2 with R = camera-to-world rotation)
        qc = rng.normal(0, 1, (P, 4))
        qc /= np.linalg.norm(qc, axis=1, keepdims=True)
        q = _qmul(_quat_of(R)[None], qc)  # camera-space orientation carried to world space
        Rq = quat_to_matrix(q)
        cov = Rq @ (s[:, :, None] ** 2 * np.swapaxes(Rq, 1, 2))
        M = (deg + 1) ** 2
        shs = rng.normal(0, 0.1, (P, M, 3))
        shs[:, 0, :] = rng.normal(0, 1.0, (P, 3))
        return dict(means3D=means.astype(np.float32), scales=s.astype(np.float32), rotations=q.astype(np.float32),
                    opacities=o.reshape(P, 1).astype(np.float32), shs=shs.astype(np.float32),
                    colors=rng.uniform(0, 1, (P, 3)).astype(np.float32), sh_degree=deg,
                    cov3D=np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]],
                                   1).astype(np.float32))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def make(family, seed=0, W=W_DEFAULT, H=H_DEFAULT):
    """(cam, g) of one family; `seed` varies everything but the family's purpose."""
    assert family in FAMILIES, family
    cam, R, T = general_camera(W, H, seed, skew=family == "general_skew")
    rng = np.random.default_rng(seed * 31 + FAMILIES.index(family))
    b = _Builder(cam, rng)

    def spread(n, zlo, zhi, logs, sd=0.3, pad=0.1, op=None):
        b.add(rng.uniform(-pad * W, (1 + pad) * W, n), rng.uniform(-pad * H, (1 + pad) * H, n), rng.uniform(zlo, zhi, n),
              np.exp(rng.normal(logs, sd, (n, 3))), _sigmoid(rng.normal(0, 1.5, n)) if op is None else op)

    if family in ("general", "general_skew"):
        spread(300, 1.5, 4.5, math.log(0.04), 0.4)
    elif family == "frustum":
        tx, ty = cam["tanfovx"], cam["tanfovy"]
        n = 40
        for axis in (0, 1):
            for sign in (-1.0, 1.0):
                r_out = sign * rng.uniform(1.35, 2.0, n) * (tx if axis == 0 else ty)
                r_in = rng.uniform(-0.6, 0.6, n) * (ty if axis == 0 else tx)
                b.add_ratio(r_out if axis == 0 else r_in, r_in if axis == 0 else r_out, rng.uniform(2.0, 4.0, n),
                            np.exp(rng.normal(math.log(0.3), 0.25, (n, 3))), _sigmoid(rng.normal(1.0, 1.0, n)))
        spread(80, 2.0, 4.0, math.log(0.05))
    elif family == "near":
        n = 24
        b.add(rng.uniform(0.2 * W, 0.8 * W, n), rng.uniform(0.2 * H, 0.8 * H, n), rng.uniform(0.25, 0.6, n),
              np.exp(rng.normal(math.log(0.08), 0.2, (n, 3))), _sigmoid(rng.normal(-1.0, 1.0, n)))
        b.add(rng.uniform(0, W, 16), rng.uniform(0, H, 16), rng.uniform(0.02, 0.17, 16),
              np.exp(rng.normal(math.log(0.05), 0.2, (16, 3))), _sigmoid(rng.normal(0, 1.0, 16)))
        spread(160, 1.5, 4.0, math.log(0.04))
    elif family == "opaque":
        spread(300, 2.0, 4.0, math.log(0.15), 0.2, pad=0.0, op=rng.uniform(0.99, 0.9999, 300))
    elif family == "needle":
        n = 250
        long_ = np.exp(rng.normal(math.log(0.2), 0.3, n))
        s = long_[:, None] * 10.0 ** -rng.uniform(3.0, 3.5, (n, 3))
        s[np.arange(n), rng.integers(0, 3, n)] = long_
        b.add(rng.uniform(-0.1 * W, 1.1 * W, n), rng.uniform(-0.1 * H, 1.1 * H, n), rng.uniform(1.5, 4.0, n), s,
              _sigmoid(rng.normal(0.5, 1.5, n)))
    return cam, b.finish(R, T)


def view_space(cam, g):
    """Camera-space means (float64) as the rasterizer computes them from viewmatrix."""
    vm = cam["viewmatrix"].astype(np.float64).reshape(4, 4)
    return g["means3D"].astype(np.float64) @ vm[:3, :3] + vm[3, :3]
