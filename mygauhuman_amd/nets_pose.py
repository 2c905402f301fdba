"""The pose-correction network of render() with fused HIP kernels (csrc/pose_refiner.hip).

    net = FusedBodyPoseRefiner(total_bones=J, embedding_size=3 * (J - 1), mlp_width=128, mlp_depth=2)   # scene/gaussian_model.py:95
    net.load_state_dict(reference_module.state_dict())     # block_mlps.{0,2,4}.{weight,bias}
    pc.pose_decoder = net                                   # render(): correct_Rs = pc.pose_decoder(poses[:, 3:])["Rs"]

The reference's BodyPoseRefiner (nets/mlp_delta_body_pose.py) maps the pose vector through a Linear / ReLU stack to J - 1 axis-angle
corrections and turns them into rotations with its RodriguesModule (theta = sqrt(1e-5 + |r|^2): not the SMPL batch_rodrigues of the
pose chain).  render() runs it every frame when motion_offset_flag is set (gaussian_renderer/__init__.py:100-106).  As torch ops that
is three addmm, two ReLU and some forty elementwise kernels forward and about twice as many backward, for 35k multiply-adds at one pose
row: here forward and backward are one launch each (the backward recomputes the forward and writes every parameter gradient and,
when the input requires grad, the input gradient).

The kernels are built for the reference's own construction -- width 128, depth 2 -- at J = 24 (SMPL) and 55 (SMPL-X), 1 to 16 pose
rows of float32 on a HIP device (a strided view such as poses[:, 3:] is read in place).  Every other configuration, a CPU input and
use_fused = False take forward_torch: the same arithmetic in torch ops, which raises only where the reference would.

This module also answers to the reference's import path (install_dropin(pose_refiner=True) registers it as nets.mlp_delta_body_pose),
so BodyPoseRefiner and RodriguesModule are the reference's names, with its constructor, attributes, state_dict keys and
initialisation (bit for bit under the same torch.manual_seed).  A BodyPoseRefiner pickled by the reference (GaussianModel.capture())
unpickles into this class and runs: use_fused has a class-level default.
"""
import ctypes as C
import math

import torch
from torch import nn

from ._lib import call

FUSED_JOINTS = (24, 55)     # the joint counts csrc/pose_refiner.hip is compiled for
FUSED_WIDTH = 128
FUSED_DEPTH = 2
FUSED_MAX_ROWS = 16


def _init_stack(seq):
    """The reference's initialisation of a Linear / ReLU stack, in module order: every Linear's weight uniform in +-std sqrt(3) with
    std = gain sqrt(2 / (fan_in + fan_out)) -- gain sqrt(2) (ReLU) when a ReLU follows it, 1 otherwise -- and its bias zero."""
    mods = list(seq)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Linear):
            relu_next = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            gain = nn.init.calculate_gain("relu") if relu_next else 1.0
            std = gain * math.sqrt(2.0 / (m.in_features + m.out_features))
            m.weight.data.uniform_(-(std * math.sqrt(3.0)), std * math.sqrt(3.0))
            m.bias.data.zero_()


class RodriguesModule(nn.Module):
    """rvec [N, 3] -> [N, 3, 3]: cos(t) I + (1 - cos t) n n^T + sin(t) [n]x with t = sqrt(1e-5 + |rvec|^2), n = rvec / t, written
    entry by entry as the reference writes it (a zero rvec gives the identity)."""

    def forward(self, rvec):
        theta = torch.sqrt(1e-5 + torch.sum(rvec ** 2, dim=1))
        n = rvec / theta[:, None]
        c, s = torch.cos(theta), torch.sin(theta)
        omc = 1.0 - c
        n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
        rows = (n0 ** 2 + (1.0 - n0 ** 2) * c, n0 * n1 * omc - n2 * s, n0 * n2 * omc + n1 * s,
                n0 * n1 * omc + n2 * s, n1 ** 2 + (1.0 - n1 ** 2) * c, n1 * n2 * omc - n0 * s,
                n0 * n2 * omc - n1 * s, n1 * n2 * omc + n0 * s, n2 ** 2 + (1.0 - n2 ** 2) * c)
        return torch.stack(rows, dim=1).view(-1, 3, 3)


class FusedBodyPoseRefiner(nn.Module):
    # class-level: an object restored by pickle without it (the reference's BodyPoseRefiner has no such attribute) still runs fused
    use_fused = True

    def __init__(self, total_bones=24, embedding_size=69, mlp_width=256, mlp_depth=4, **_):
        super().__init__()
        layers = [nn.Linear(embedding_size, mlp_width), nn.ReLU()]
        for _ in range(mlp_depth - 1):
            layers += [nn.Linear(mlp_width, mlp_width), nn.ReLU()]
        self.total_bones = total_bones - 1          # the reference's meaning: the number of corrected joints
        layers.append(nn.Linear(mlp_width, 3 * self.total_bones))
        self.block_mlps = nn.Sequential(*layers)
        _init_stack(self.block_mlps)
        last = self.block_mlps[-1]                  # near-identity rotations at the start
        last.weight.data.uniform_(-1e-5, 1e-5)
        last.bias.data.zero_()
        self.rodriguez = RodriguesModule()
        # False: forward_torch everywhere (comparisons); the fused kernels run only where fused_params() accepts the call
        self.use_fused = True

    def forward_torch(self, pose_input):
        """The reference's forward in torch ops (any configuration, any device; differentiable)."""
        rvec = self.block_mlps(pose_input).view(-1, 3)
        return {"Rs": self.rodriguez(rvec).view(-1, self.total_bones, 3, 3)}

    def fused_params(self, x):
        """[w0, b0, w2, b2, w4, b4] when the fused kernels can run this call, else None."""
        m = self.block_mlps
        J, E = self.total_bones + 1, 3 * self.total_bones
        if J not in FUSED_JOINTS or len(m) != 2 * FUSED_DEPTH + 1:
            return None
        kinds = (nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear)
        if any(type(mod) is not k for mod, k in zip(m, kinds)):
            return None
        shapes = ((FUSED_WIDTH, E), (FUSED_WIDTH, FUSED_WIDTH), (E, FUSED_WIDTH))
        if any(tuple(m[2 * i].weight.shape) != shp or m[2 * i].bias is None for i, shp in enumerate(shapes)):
            return None
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == E
                and 1 <= x.shape[0] <= FUSED_MAX_ROWS):
            return None
        params = [t for i in (0, 2, 4) for t in (m[i].weight, m[i].bias)]
        if not all(p.device == x.device and p.dtype == torch.float32 and p.is_contiguous() for p in params):
            return None
        return params

    def forward(self, pose_input):
        """pose_input [B, 3(J-1)] -> {"Rs": [B, J-1, 3, 3]}."""
        params = self.fused_params(pose_input) if self.use_fused else None
        if params is None:
            return self.forward_torch(pose_input)
        return {"Rs": _FusedPoseRefiner.apply(pose_input, self.total_bones + 1, *params)}


BodyPoseRefiner = FusedBodyPoseRefiner      # the reference's class name (scene/gaussian_model.py imports it)


def _ptrs(ts):
    return (C.c_void_p * 3)(*[t.data_ptr() for t in ts])   # a host array of device pointers


class _FusedPoseRefiner(torch.autograd.Function):
    """x [B, 3(J-1)] (any strides), J, the six parameters -> Rs [B, J-1, 3, 3]; backward = gsr_pose_refiner_backward."""

    @staticmethod
    def forward(ctx, x, J, w0, b0, w2, b2, w4, b4):
        ps = [t.detach() for t in (w0, b0, w2, b2, w4, b4)]
        B, dev = x.shape[0], x.device
        Rs = torch.empty((B, J - 1, 3, 3), dtype=torch.float32, device=dev)
        call("gsr_pose_refiner_forward", dev, J, B, FUSED_WIDTH, x.data_ptr(), x.stride(0), x.stride(1), _ptrs(ps[0::2]),
             _ptrs(ps[1::2]), Rs.data_ptr())
        ctx.save_for_backward(x, *ps)
        ctx.J = J
        return Rs

    @staticmethod
    def backward(ctx, g):
        x, *ps = ctx.saved_tensors
        B, dev = x.shape[0], x.device
        g = g.contiguous()
        grads = [torch.empty_like(p) for p in ps]
        dx = torch.empty((B, x.shape[1]), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        call("gsr_pose_refiner_backward", dev, ctx.J, B, FUSED_WIDTH, x.data_ptr(), x.stride(0), x.stride(1), _ptrs(ps[0::2]),
             _ptrs(ps[1::2]), g.data_ptr(), _ptrs(grads[0::2]), _ptrs(grads[1::2]), None if dx is None else dx.data_ptr())
        return (dx, None, *[gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[2:])])
