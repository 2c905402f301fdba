"""Seeded synthetic ARTICULATED scene ("S-human") for the render() workloads of bench.py, the tools and the
view-parallel tests: an SMPL-shaped body model (random template / blend shapes / regressor / skinning weights with the
standard 24-joint tree -- the real SMPL_NEUTRAL.pkl needs a registration download and is not in the reference tree), P canonical
Gaussians scattered around its vertices, ring cameras at 2.4 m looking at the body (BASELINE configs[3]: "8 ZJU-MoCap views per
step"), one target pose per view, and -- for motion_offset_flag models -- two small MLPs with the call surface of the
reference's decoders (nets/mlp_delta_body_pose.py: pose_decoder(posevec)["Rs"] [1,23,3,3]; nets/mlp_delta_weight_lbs.py:
lweight_offset_decoder(xyz[1,P,3]) -> [1,24,P]).  Everything is generated on the CPU from numpy's default_rng: all ranks and
all devices see the same bits.

body="smplx" makes an SMPL-X-shaped body instead (the reference's default smpl_type): V = 10,475 vertices, the 55-joint tree
(22 body + jaw + 2 eyes + 2 x 15 hand), 20 shape columns (betas + expression), posedirs [V, 3, 486], poses [1, 165], shapes [1, 20], a
refiner mapping the 162-d pose vector to Rs [1, 54, 3, 3] and an offset stand-in with 55 outputs.  The "smpl" body (the default) and
its random streams are unchanged."""
import math

import numpy as np
import torch

from . import cameras
from .lbs import batch_rodrigues
from .scene_model import HumanGaussianModel

PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int64)
PARENTS_SMPLX = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15, 20, 25, 26, 20, 28,
                          29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53], np.int64)
# body -> (vertices, joints, shape columns, parents)
BODIES = {"smpl": (6890, 24, 10, PARENTS), "smplx": (10475, 55, 20, PARENTS_SMPLX)}


class PoseRefiner(torch.nn.Module):
    """posevec [1,3(J-1)] -> {"Rs": [1,J-1,3,3]}: a small MLP whose output (J - 1 axis-angle corrections, initialised near zero) goes
    through rodrigues, like BodyPoseRefiner.  J = 24: 69 -> 23; J = 55 (SMPL-X): 162 -> 54."""

    def __init__(self, width=128, seed=0, joints=24):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        n = 3 * (joints - 1)
        self.n = n
        self.w1 = torch.nn.Parameter(torch.randn((n, width), generator=g) / math.sqrt(float(n)))
        self.b1 = torch.nn.Parameter(torch.zeros(width))
        self.w2 = torch.nn.Parameter(1e-2 * torch.randn((width, n), generator=g) / math.sqrt(width))
        self.b2 = torch.nn.Parameter(torch.zeros(n))

    def forward(self, posevec):
        h = torch.relu(posevec.reshape(1, self.n) @ self.w1 + self.b1)
        rv = (h @ self.w2 + self.b2).reshape(self.n // 3, 3)
        return {"Rs": batch_rodrigues(rv).reshape(1, self.n // 3, 3, 3)}


class LbsOffsetDecoder(torch.nn.Module):
    """xyz [1,P,3] -> skinning-weight logit offsets [1,24,P] (LBSOffsetDecoder's call surface).  A STAND-IN, not the reference's
    network: an AFFINE map of the position -- offsets[j] = b[j] + A[:, j] . xyz, 96 parameters, three broadcast multiply-adds.
    The reference runs its real decoder EVERY frame when motion_offset_flag is set (gaussian_renderer/__init__.py:100-106 calls
    pc.lweight_offset_decoder(means3D)): a 63-d positional embedding through four 128-wide Conv1d layers on every Gaussian
    (nets/mlp_delta_weight_lbs.py), i.e. ~2 x (63 x 128 + 3 x 128 x 128 + 128 x 24) = 120 kFLOP per Gaussian per frame forward,
    a 200k x 128 GEMM chain that is likely the largest single cost of the reference's own step.  That network is outside SURVEY.md
    section 8 (render() calls whatever `pc.lweight_offset_decoder` is), so every figure measured with this stand-in -- `bench.py
    --workload render`, the view-parallel payload -- OMITS it, and the bench line says so in config.workload.  (A stand-in MLP with
    a 3- or 24-wide side spends the frame in rocBLAS' skinny-GEMM kernels: a 3-64-24 MLP on 200k points measured 1.2 ms of two
    rocBLAS launches per frame, more than the whole render() frame -- which is why the stand-in is affine.)"""

    def __init__(self, seed=1, joints=24):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.A = torch.nn.Parameter(0.05 * torch.randn((3, joints), generator=g))
        self.b = torch.nn.Parameter(torch.zeros(joints))

    def forward(self, xyz):
        x = xyz[0]
        out = self.b + x[:, 0:1] * self.A[0] + x[:, 1:2] * self.A[1] + x[:, 2:3] * self.A[2]   # [P, J]
        return out.t()[None]


def body_arrays(V=None, seed=0, body="smpl"):
    """The body tables as numpy arrays (posedirs in gaussian_model.py's [V, 3, 9(J-1)] layout); V = None: the body's own count."""
    nv, nj, ns, _ = BODIES[body]
    V = nv if V is None else V
    rng = np.random.default_rng(seed)
    vt = rng.uniform(-1, 1, (V, 3)).astype(np.float32) * np.array([0.45, 0.9, 0.15], np.float32)
    J = rng.uniform(0, 1, (nj, V)).astype(np.float32)
    w = rng.uniform(0, 1, (V, nj)).astype(np.float32) ** 4
    return dict(v_template=vt, shapedirs=rng.normal(0, 0.01, (V, 3, ns)).astype(np.float32),
                posedirs=rng.normal(0, 0.001, (V, 3, 9 * (nj - 1))).astype(np.float32), J_regressor=J / J.sum(1, keepdims=True),
                weights=(w / w.sum(1, keepdims=True)).astype(np.float32))


def kintree_table(body="smpl"):
    """[2, J] int64: parents (entry 0 = -1) over joint indices, the layout of the SMPL / SMPL-X model files."""
    parents = BODIES[body][3]
    return np.stack([parents, np.arange(parents.shape[0])])


def gaussian_arrays(body, P, seed=0, scale=0.006):
    rng = np.random.default_rng(seed + 1)
    vt = body["v_template"]
    pts = (vt[rng.integers(0, vt.shape[0], P)] + rng.normal(0, 0.01, (P, 3))).astype(np.float32)
    return dict(means3D=pts, scales=np.exp(rng.normal(np.log(scale), 0.3, (P, 3))).astype(np.float32),
                rotations=rng.normal(0, 1, (P, 4)).astype(np.float32),
                opacities=(1 / (1 + np.exp(-rng.normal(0, 1.5, (P, 1))))).astype(np.float32),
                shs=np.concatenate([rng.normal(0, 1, (P, 1, 3)), rng.normal(0, 0.1, (P, 15, 3))], 1).astype(np.float32))


def view_camera(body, W, H, view, n_views=8, device="cuda", radius=2.4, fov_deg=50.0, pose_scale=0.15):
    """Ring camera `view` of n_views (view 0 looks along +z from z = -radius, like tools/render_bench.py) with ITS OWN target pose
    and shape (seeded by the view index) and the shared big pose.  poses [1, 3J] and shapes [1, shape columns] follow `body`."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)  # noqa: E731
    cam_np = cameras.ring_camera(W, H, view % n_views, n_views, radius=radius, fov_deg=fov_deg)
    nj, ns = body["weights"].shape[1], body["shapedirs"].shape[2]
    rng = np.random.default_rng(1000 + view)
    sp = dict(poses=d(rng.normal(0, pose_scale, (1, 3 * nj))), shapes=d(rng.normal(0, 0.5, (1, ns))), R=d(np.eye(3)),
              Th=d(np.zeros((1, 3))))
    bp = dict(poses=d(np.zeros((1, 3 * nj))), shapes=d(np.zeros((1, ns))), R=d(np.eye(3)), Th=d(np.zeros((1, 3))))
    cam = cameras.ViewCamera(cam_np, device, sp, bp, d(body["v_template"]))
    cam.cam_np = cam_np
    return cam


def build(P, V=None, device="cuda", seed=0, motion=False, sh_degree=3, decoder="affine", body="smpl", pose_decoder="stand_in"):
    """(model, body arrays).  model.SMPL_NEUTRAL holds the body tables as device tensors; motion=True attaches the two decoders
    (decoder = "affine": the 3 x J stand-in; "reference_size": nets.FusedLBSOffsetDecoder -- the reference network's layers,
    random init -- on the fused kernels (at both J = 24 and 55); "reference_size_torch": the same module in torch ops).
    body: "smpl" (default, 24 joints) or "smplx" (55 joints); V = None: the body's own vertex count.  pose_decoder = "stand_in" (the
    PoseRefiner above), "reference_size" (nets_pose.FusedBodyPoseRefiner as scene/gaussian_model.py:95 builds it -- width 128, depth 2,
    the reference's initialisation under torch.manual_seed(seed + 5) -- on the fused kernels) or "reference_size_torch" (the same module
    in torch ops)."""
    if pose_decoder not in ("stand_in", "reference_size", "reference_size_torch"):
        raise ValueError(f"human_synth.build: pose_decoder = {pose_decoder!r}")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    kind = body
    body = body_arrays(V, seed, kind)
    nj = BODIES[kind][1]
    smpl = {k: d(v) for k, v in body.items()}
    smpl["kintree_table"] = torch.from_numpy(kintree_table(kind)).to(device)
    model = HumanGaussianModel.from_arrays(gaussian_arrays(body, P, seed), sh_degree, smpl=smpl, motion_offset_flag=motion,
                                           device=device, seed=seed)
    if motion:
        if pose_decoder == "stand_in":
            model.pose_decoder = PoseRefiner(joints=nj).to(device)
        else:
            from .nets_pose import FusedBodyPoseRefiner
            torch.manual_seed(seed + 5)
            ref = FusedBodyPoseRefiner(total_bones=nj, embedding_size=3 * (nj - 1), mlp_width=128, mlp_depth=2).to(device)
            ref.use_fused = pose_decoder == "reference_size"
            model.pose_decoder = ref
        if decoder in ("reference_size", "reference_size_torch"):
            from .nets import FusedLBSOffsetDecoder
            torch.manual_seed(seed + 7)
            net = FusedLBSOffsetDecoder(nj).to(device)
            with torch.no_grad():
                net.bw_fc.weight.mul_(0.05)      # small offsets around the SMPL weights, like a network early in training
            net.use_fused = decoder == "reference_size"   # (nj is 24 or 55: both in nets.FUSED_BONE_COUNTS)
            model.lweight_offset_decoder = net
        else:
            model.lweight_offset_decoder = LbsOffsetDecoder(joints=nj).to(device)
    return model, body
